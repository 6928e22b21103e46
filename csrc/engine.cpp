// Decoder executor: the time loops of the caption decoder in C++.
//
// The reference runs its time loops in Python (model.py:234-289 forward,
// 319-367 sample), one ATen/cuDNN call at a time, with a device->host sync per
// step (`it.sum() == 0`, model.py:269) and multinomial sampling on the CPU
// (model.py:331-337).  Here each step is three async launches -- fused LSTM
// step, fused vocab projection + statistics, row combine -- enqueued on the
// current HIP stream from C++; the end-of-sequence rules are evaluated on
// the device, so a whole rollout is enqueued without a single host sync (and
// is capturable in a HIP graph).
//
// decoder_forward : teacher forcing / scheduled sampling / MIXER rollout /
//                   greedy or multinomial sample(), optionally saving what the
//                   backward needs (the exp store E = exp(logit - previous
//                   LSE) in bf16, dropped h, gates, c, [x;h]).
// decoder_backward: batched vocab-head backward without forming dS (two
//                   hipBLASLt GEMMs over all T*R rows of E at once, row scales
//                   and one-hot terms in kernels/vocab_grad.hip), then the
//                   reverse LSTM recurrence (one fused kernel per step), then
//                   the weight-gradient GEMMs (input-token ones over per-token
//                   sums, V rows instead of T*R).
//
// This file holds the state the executor's units share (engine_internal.h):
// stamps, per-device streams / events / error word / loop scratch, the modes
// set from Python and the grad events.  The entry points (engine.h) live in
// decoder_forward.cpp, decoder_backward.cpp, beam_search.cpp, train_ops.cpp
// and dev_entries.cpp.
#include "engine_internal.h"

namespace cst {

// Device timeline stamps (kernels/stamp.hip): the caller picks the base slot
// of the next decoder_forward / decoder_backward call (sample and greedy
// decodes of one step use different bases); -1 = no stamps from the executor.
static int g_stamp_base = -1;
void set_stamp_base(int64_t base) { g_stamp_base = (int)base; }
void stamp(int rel, hipStream_t s) {
  if (g_stamp_base >= 0) launch_stamp(g_stamp_base + rel, s);
}
void stamp_buffer(at::Tensor buf) {
  if (!buf.defined() || buf.numel() == 0) {
    set_stamp_buffer(nullptr, 0);
    return;
  }
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == at::kLong && buf.is_contiguous(),
              "stamp buffer must be a contiguous int64 GPU tensor");
  set_stamp_buffer(buf.data_ptr<int64_t>(), (int)buf.numel());
}
void stamp_now(int64_t slot) { launch_stamp((int)slot, cur_stream()); }

// X = E W of a training forward's exp store (n, R, ldl) bf16 -> out (n, R, H)
// fp32, on the current stream (engine.launch_x; the same GEMM as the
// backward's dHd chunks), through hipBLASLt's measured algorithm choice
// (host/blaslt_tuned.cpp: the heuristic's 32 candidates timed once on an idle
// device, or pinned by CSTCAP_BLASLT_ALGO): interleaved A/B 3.503-3.505 vs
// 3.562-3.574 ms per step against PyTorch's first choice, profiles/r4.
// (A 3-way split-K batch measured slower: 3.74 vs 3.67-3.73 ms per step,
// profiles/r3/ab_xsplitk.txt; the round-4 hand-written persistent GEMM was
// correct but slower in the step, 3.80 vs 3.68 ms, and was removed.)
void vocab_x(at::Tensor logits16, at::Tensor wlog, at::Tensor out) {
  TORCH_CHECK(logits16.is_cuda() && logits16.scalar_type() == at::kBFloat16 &&
                  logits16.dim() == 3 && logits16.is_contiguous(),
              "vocab_x: exp store must be a contiguous bf16 (n, R, ldl) GPU tensor");
  const int64_t NR = logits16.size(0) * logits16.size(1), V = wlog.size(0), H = wlog.size(1);
  TORCH_CHECK(out.is_contiguous() && out.scalar_type() == at::kFloat && out.numel() == NR * H &&
                  logits16.size(2) >= V,
              "vocab_x: out must be a contiguous fp32 (n, R, H) tensor");
  const int64_t ldl = logits16.size(2);
  gemm_bf16_tuned(out.view({NR, H}), logits16.view({NR, ldl}).narrow(1, 0, V), false, wlog, false,
                  32);
}
int64_t wall_clock_khz() {
  int dev = 0, khz = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  return khz;
}

// Events and side streams are created once per device and reused: nothing
// is created or destroyed while a HIP graph is being captured.
DeviceAux& device_aux(int dev_index) {
  static std::map<int, DeviceAux*> aux;
  auto it = aux.find(dev_index);
  if (it == aux.end()) {
    auto* a = new DeviceAux{{}, {c10::hip::getStreamFromPool(false, dev_index),
                                 c10::hip::getStreamFromPool(false, dev_index)}};
    a->ev.resize(EV_COUNT);
    for (auto& e : a->ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    for (auto& e : a->grad_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    for (auto& e : a->fwd_ev) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    it = aux.emplace(dev_index, a).first;
  }
  return *it->second;
}

// Device error word (one int32 per device, zero until a kernel reports a
// failed cross-workgroup hand-off): a bounded flag poll that runs out of polls
// (lstm.hip att_fuse_wait) adds 1 instead of silently reading operands that
// may not be written yet.  The trainer reads it at log time and raises; the
// bench reports it.  set_poll_bound(0) forces every such wait to give up
// (tests of the counter).
static int g_poll_bound = 1 << 20;
int* device_err_word(int dev_index) {
  static std::map<int, int*> words;
  auto it = words.find(dev_index);
  if (it == words.end()) {
    int* p = nullptr;
    c10::hip::HIPGuard guard(dev_index);
    TORCH_CHECK(hipMalloc(&p, sizeof(int)) == hipSuccess, "device error word: hipMalloc");
    TORCH_CHECK(hipMemset(p, 0, sizeof(int)) == hipSuccess, "device error word: hipMemset");
    it = words.emplace(dev_index, p).first;
  }
  return it->second;
}
// persistent reverse loop on (default; CSTCAP_BWD_LOOP=0 or set_bwd_loop(false):
// one launch per step)
// (CSTCAP_BWD_LOOP=1: the persistent form whose workgroups read their rows'
// whole dG_{t+1} -- the default; 2: the K-split form that exchanges fp32
// partials instead, measured slower: 361.8 vs 331.6 us per loop alone,
// 3.359-3.371 vs 3.338-3.345 ms per step, profiles/r6/README_r6.md)
static int g_bwd_loop = [] {
  const char* e = getenv("CSTCAP_BWD_LOOP");
  return e == nullptr ? 1 : atoi(e);
}();
void set_bwd_loop(int64_t mode) { g_bwd_loop = (int)mode; }
int bwd_loop_mode() { return g_bwd_loop; }
// fused attention backward (lstm.hip att_bwd_fused_wg, the fp16 scorer values
// of the forward) on; off: the separate att_bwd_mfma launch per step, which
// recomputes tanh(P + q) in fp32 (tests of the fp16 encoding)
static bool g_att_fuse = true;
void set_att_fuse(bool on) { g_att_fuse = on; }
bool att_fuse_on() { return g_att_fuse; }
// exchange slabs of the K-split persistent loop, per device (grown on demand
// outside graph capture)
float* loop_xb(int dev_index, int64_t floats) {
  static std::map<int, std::pair<float*, int64_t>> bufs;
  auto it = bufs.find(dev_index);
  if (it != bufs.end() && it->second.second >= floats) return it->second.first;
  c10::hip::HIPGuard guard(dev_index);
  if (it != bufs.end()) {
    (void)hipDeviceSynchronize();
    (void)hipFree(it->second.first);
    bufs.erase(it);
  }
  float* p = nullptr;
  TORCH_CHECK(hipMalloc(&p, sizeof(float) * floats) == hipSuccess, "loop exchange slabs: hipMalloc");
  bufs.emplace(dev_index, std::make_pair(p, floats));
  return p;
}
void set_poll_bound(int64_t n) { g_poll_bound = (int)std::max<int64_t>(0, n); }
int poll_bound() { return g_poll_bound; }
// team counters of the persistent reverse loop (lstm_loop.hip), per device;
// the launcher zeroes the used prefix before every launch
int* loop_counters(int dev_index, int ints) {
  static std::map<int, std::pair<int*, int>> bufs;
  auto it = bufs.find(dev_index);
  if (it == bufs.end() || it->second.second < ints) {
    TORCH_CHECK(it == bufs.end(), "persistent reverse loop: counter block too small");
    int* p = nullptr;
    c10::hip::HIPGuard guard(dev_index);
    const int n = std::max(ints, 4096);
    TORCH_CHECK(hipMalloc(&p, sizeof(int) * n) == hipSuccess, "loop counters: hipMalloc");
    TORCH_CHECK(hipMemset(p, 0, sizeof(int) * n) == hipSuccess, "loop counters: hipMemset");
    it = bufs.emplace(dev_index, std::make_pair(p, n)).first;
  }
  return it->second.first;
}
int64_t device_errors(int64_t dev_index) {
  int* p = device_err_word((int)dev_index);
  int v = 0;
  c10::hip::HIPGuard guard((int)dev_index);
  TORCH_CHECK(hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess,
              "device error word: read");
  return v;
}
void reset_device_errors(int64_t dev_index) {
  int* p = device_err_word((int)dev_index);
  c10::hip::HIPGuard guard((int)dev_index);
  TORCH_CHECK(hipMemset(p, 0, sizeof(int)) == hipSuccess, "device error word: reset");
}

// Data parallelism, communication overlapped with the backward: with
// set_grad_events(true) decoder_backward records grad_ev[0] once the vocab
// head's gradients (logit W, b) are final (side stream, after dW_logit, which
// then runs under the reverse loop) and grad_ev[1] once the embedding
// gradient is (main stream, after its GEMM).  Inside a graph capture they are
// event-record NODES of the captured graph (record_grad_event), so after each replay
// the trainer's comm stream waits on them (grad_event_wait) and all-reduces
// those bucket slices while the rest of the replayed backward still runs --
// eager RCCL between replays, no collective inside the graph.
static bool g_grad_events_on = false;
void set_grad_events(bool on) { g_grad_events_on = on; }
bool grad_events_on() { return g_grad_events_on; }
// host-side count of record calls per group (inline records and captured
// record nodes): the trainer checks that a step (or the capture of one)
// recorded both events before its comm stream relies on them -- a wait on an
// event this step never recorded would order nothing
static int64_t g_grad_ev_count[3] = {0, 0, 0};
int64_t grad_event_count(int64_t k) {
  TORCH_CHECK(k >= 0 && k < 3, "grad_event_count: group 0, 1 or 2");
  return g_grad_ev_count[k];
}
void record_grad_event(hipEvent_t ev, hipStream_t s, int k) {
  g_grad_ev_count[k]++;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  unsigned long long id = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(s, &cs, &id, &graph, &deps, &nd);
  TORCH_CHECK(e == hipSuccess, "grad event: capture info: ", hipGetErrorString(e));
  if (cs != hipStreamCaptureStatusActive) {
    e = hipEventRecord(ev, s);
    TORCH_CHECK(e == hipSuccess, "grad event: record: ", hipGetErrorString(e));
    return;
  }
  // an event-record node of the graph being captured, after the stream's
  // current dependencies; the stream's later work then follows the node
  // (hipEventRecordWithFlags(hipEventRecordExternal) failed with "invalid
  // argument" inside a capture on this ROCm)
  hipGraphNode_t node = nullptr;
  e = hipGraphAddEventRecordNode(&node, graph, deps, nd, ev);
  TORCH_CHECK(e == hipSuccess, "grad event: record node: ", hipGetErrorString(e));
  e = hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies);
  TORCH_CHECK(e == hipSuccess, "grad event: capture dependencies: ", hipGetErrorString(e));
}
void grad_event_record(int64_t k, int64_t stream) {
  TORCH_CHECK(k >= 0 && k < 3, "grad_event_record: group 0, 1 or 2");
  int dev = 0;
  (void)hipGetDevice(&dev);
  record_grad_event(device_aux(dev).grad_ev[k], reinterpret_cast<hipStream_t>(stream), (int)k);
}
void grad_event_wait(int64_t k, int64_t stream) {
  TORCH_CHECK(k >= 0 && k < 3, "grad_event_wait: group 0, 1 or 2");
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), device_aux(dev).grad_ev[k], 0);
}

// Read-only zeros of at least n elements (initial decoder states): one
// persistent buffer per (device, dtype), so a decode does not launch a fill
// kernel per call.  Grown only outside graph capture; replaced buffers stay
// alive (a captured graph may still read them).
at::Tensor zeros_view(const at::Device& dev, int64_t n, at::ScalarType dtype) {
  static std::map<std::pair<int, int>, std::vector<at::Tensor>> bufs;
  auto& v = bufs[std::make_pair((int)dev.index(), (int)dtype)];
  if (v.empty() || v.back().numel() < n) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(cur_stream(), &cs);
    auto opts = at::TensorOptions().dtype(dtype).device(dev);
    if (cs != hipStreamCaptureStatusNone) return at::zeros({n}, opts);
    v.push_back(at::zeros({std::max<int64_t>(n, 1 << 20)}, opts));
  }
  return v.back().narrow(0, 0, n);
}

// C = A^T B over the first K rows of the bf16 row-major operands A (K x >= M)
// and B (K x >= N) through the hand-written split-K kernel (kernels/wgrad.hip):
// rows [0, M0) of C into C0 (row stride ldc0), rows [M0, M) into C1.  Returns
// false (nothing launched) when the shapes do not fit the kernel.
// al / db (optional, N = 512): also db[m] = sum_k al[k] A[k][m] (fused column
// sums of the A tiles in LDS)
// rmap (optional, M0 ints on the device): row m < M0 is stored as row rmap[m]
// of C0 (< 0: dropped) -- the packed -> PyTorch gate order of a weight slot
bool wgrad_tn_into(const at::Tensor& A, int64_t lda, const at::Tensor& B, int64_t ldb, int64_t M,
                   int64_t N, int64_t K, float* C0, int64_t ldc0, int64_t M0, float* C1,
                   int64_t ldc1, hipStream_t st, const float* al, float* db, const int* rmap) {
  if (A.scalar_type() != at::kBFloat16 || B.scalar_type() != at::kBFloat16 ||
      !wgrad_tn_ok(M, N, K, lda, ldb, A.data_ptr(), B.data_ptr()) || (db != nullptr && N != 512))
    return false;
  const int S = wgrad_tn_splits(M, N, K);
  at::Tensor ws, ws_db;
  if (S > 1) ws = at::empty({S, M, N}, A.options().dtype(at::kFloat));
  if (S > 1 && db != nullptr) ws_db = at::empty({S, M}, A.options().dtype(at::kFloat));
  WgradArgs g{reinterpret_cast<const uint16_t*>(A.data_ptr()), lda,
              reinterpret_cast<const uint16_t*>(B.data_ptr()), ldb, (int)M, (int)N, (int)K, S, 0,
              S > 1 ? ws.data_ptr<float>() : nullptr, C0, ldc0, (int)M0, C1, ldc1,
              db != nullptr ? al : nullptr, db, ws_db.defined() ? ws_db.data_ptr<float>() : nullptr,
              rmap};
  launch_wgrad_tn(g, st);
  return true;
}

}  // namespace cst
