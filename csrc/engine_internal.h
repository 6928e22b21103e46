// Shared state and helpers of the decoder executor's translation units
// (engine.cpp defines them; decoder_forward.cpp, decoder_backward.cpp,
// beam_search.cpp, train_ops.cpp and dev_entries.cpp use them).
#pragma once
#include <torch/extension.h>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "engine.h"
#include "launchers.h"

namespace cst {

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

template <class T>
inline T* ptr_or_null(const at::Tensor& t) {
  return t.defined() && t.numel() > 0 ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

inline void check_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// rng: int32[2] device tensor {dropout seed, sampling seed} (or undefined /
// empty: seeds 0).  Kernels read it from device memory, so a captured HIP
// graph draws fresh masks and samples on every replay.
inline const uint32_t* rng_ptr(const at::Tensor& rng) {
  if (!rng.defined() || rng.numel() == 0) return nullptr;
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == at::kInt && rng.numel() >= 2 &&
                  rng.is_contiguous(),
              "rng must be a contiguous int32[2] GPU tensor");
  return reinterpret_cast<const uint32_t*>(rng.data_ptr());
}

// device timeline stamp at base + rel on s (no-op without set_stamp_base)
void stamp(int rel, hipStream_t s);

// Events and side streams are created once per device and reused: nothing
// is created or destroyed while a HIP graph is being captured.
constexpr int MAX_DHD_CHUNKS = 32;  // per-chunk events of the vocab-head dHd GEMM
constexpr int XE_MAX_STEPS = 64;  // XE all rows: decode steps per forward
// slots of DeviceAux::ev (decoder_backward; "side" / "side2" = side[0] / side[1]).
// Two pairs of names share an event, as the schedule always has: their uses
// never overlap (each is recorded and waited on in one place at a time), and
// the runtime sees the same event objects as before the names existed.
enum BwdEvent {
  EV_ROWS_READY = 0,  // main -> side: the loop's preparation (and, with a forward X, the
                      // one-hot pass) is enqueued; the side stream's vocab-head work may start
  EV_LOOP_DONE = 1,   // main -> side2: the reverse loop's dG rows (dGv / video-gate sums)
  EV_SIDE_DONE = 2,   // side -> main (and the comm stream): dW_logit + bias sums, then again
                      // the recurrent-weight gradients; the final join
  EV_TOK_SORTED = 3,  // side2 -> main: the token sort, before the per-token sums
  EV_DW_START = 4,    // main -> side: the persistent loop's vocab-head weight gradients may
                      // start (after the loop, the token sums or the d_emb GEMM)
  EV_DG_ROWS = 4,     // main -> side: the loop's dG rows, for the recurrent-weight gradients
  EV_DGV_DONE = 5,    // side2 -> main: attention's dGv
  EV_DVG_DONE = 5,    // side2 -> main: the video-gate (and FeatPool) gradients (no attention)
  EV_DHD_CHUNK0 = 6,  // side -> main: dHd chunk ci is EV_DHD_CHUNK0 + ci
  EV_PRE_X = EV_DHD_CHUNK0 + MAX_DHD_CHUNKS,  // main -> side2: decoder_backward's pre-X point
  EV_COUNT
};
struct DeviceAux {
  std::vector<hipEvent_t> ev;
  c10::hip::HIPStream side[2];
  hipEvent_t grad_ev[3];  // data parallelism: gradient groups final (set_grad_events)
  hipEvent_t fwd_ev[2];   // decoder_forward: step 0's exp-store conversion fork / join
};
DeviceAux& device_aux(int dev_index);
// one edge between two streams: work enqueued on `to` after this call runs
// after everything enqueued on `from` before it
inline void fork(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  (void)hipEventRecord(ev, from);
  (void)hipStreamWaitEvent(to, ev, 0);
}

// the device error word, team counters and exchange slabs (per device), and
// the modes the Python side sets (engine.cpp)
int* device_err_word(int dev_index);
float* loop_xb(int dev_index, int64_t floats);
int* loop_counters(int dev_index, int ints);
int poll_bound();
int bwd_loop_mode();  // 0 one launch per step, 1 persistent (row-read), 2 persistent (K-split)
bool att_fuse_on();
bool grad_events_on();
void record_grad_event(hipEvent_t ev, hipStream_t s, int k);
at::Tensor zeros_view(const at::Device& dev, int64_t n, at::ScalarType dtype);
bool wgrad_tn_into(const at::Tensor& A, int64_t lda, const at::Tensor& B, int64_t ldb, int64_t M,
                   int64_t N, int64_t K, float* C0, int64_t ldc0, int64_t M0, float* C1,
                   int64_t ldc1, hipStream_t st, const float* al = nullptr, float* db = nullptr,
                   const int* rmap = nullptr);

// Dropout between layers (nn.LSTM's inter-layer dropout) and before the vocab
// projection share the counter hash, keyed by step + 65536 * (layers above).
inline int drop_key(int64_t NL, int64_t l, int64_t t) { return (int)(t + 65536 * (NL - 1 - l)); }

// The packed list arguments of decoder_forward / decoder_backward /
// beam_search, parsed and checked in one place each; `site` selects the
// conditions (and the list layout) of the calling entry point.
enum class Site { Forward, Backward, Beam };

// temporal attention (num_chunks > 1): att = {Gv (Bv, C, 4H) f32 packed gates,
// P (Bv, C, A) f32, W_q (A, H) bf16, w_a (A) f32, b_a (1) f32}; vgate unused.
// MANet (modal attention over the C modality blocks): w_a (C, A), b_a (C).
// Backward: att = {Gv, P, W_q, w_a, alpha_all (n, R, C), q_all (n, R, A)[, u_all]}.
struct AttOperands {
  bool on = false;
  at::Tensor gv, pre, wq, wa;
  at::Tensor ba;                      // forward / beam search
  at::Tensor alpha_all, q_all, u_all;  // backward (u_all: optional, the fused backward's)
  int64_t Bv = 0, C = 0, A = 0;
  int64_t vdiv = 1;   // rows per video
  int per_frame = 0;  // scorer weights per frame (MANet)
  int CPAD = 8;       // frames padded for the MFMA path
  // R rows; vdiv: rows per video (0: R / Bv); n_steps: backward only
  static AttOperands parse(const std::vector<at::Tensor>& att, Site site, int64_t H, int64_t R,
                           int64_t vdiv, int64_t n_steps);
};

// stacked layers: `per` tensors per upper layer -- forward / beam search
// {[W_ih | W_hh] (4H, 2H), W_hh (4H, H)}; backward {[W_ih | W_hh] bf16, h_all,
// c_all, gates_all of layer l, hd_all of layer l-1}
struct UpperLayers {
  const std::vector<at::Tensor>* up = nullptr;
  int64_t per = 2, NL = 1;
  const at::Tensor& operator()(int64_t l, int k) const { return (*up)[per * (l - 1) + k]; }
  static UpperLayers parse(const std::vector<at::Tensor>& up, Site site, bool has_att,
                           bool has_s0, int64_t H, int64_t n_steps);
};

// initial state (model_type 'standard': the state after the video step):
// state0 = {h0 bf16 (rows, H), c0 fp32 (rows, H)}; empty: `on` is false
struct InitState {
  bool on = false;
  at::Tensor h0, c0;
  static InitState parse(const std::vector<at::Tensor>& state0, Site site, bool has_att,
                         int64_t rows, int64_t H);
};

// The packed operand lists.  Each entry point keeps the conditions it always
// had (the three pass different lists: the backward's carries the forward's
// saved alpha / q / u instead of b_a, beam search takes per-video states);
// the derived sizes are computed here only.
inline AttOperands AttOperands::parse(const std::vector<at::Tensor>& att, Site site, int64_t H, int64_t R,
                               int64_t vdiv, int64_t n_steps) {
  AttOperands a;
  if (att.empty()) return a;
  a.on = true;
  const int64_t H4 = 4 * H;
  if (site == Site::Backward) {
    TORCH_CHECK(att.size() == 6 || att.size() == 7,
                "att = {Gv, P, W_q, w_a, alpha_all, q_all[, u_all]}");
    a.alpha_all = att[4], a.q_all = att[5];
    if (att.size() == 7 && att[6].numel() > 0) a.u_all = att[6];
  } else {
    TORCH_CHECK(att.size() == 5, "att = {Gv, P, W_q, w_a, b_a}");
    a.ba = att[4];
  }
  a.gv = att[0], a.pre = att[1], a.wq = att[2], a.wa = att[3];
  if (site == Site::Forward)
    for (auto* t : {&a.gv, &a.pre, &a.wq, &a.wa, &a.ba}) check_cuda(*t, "attention operand");
  a.Bv = a.gv.size(0), a.C = a.gv.size(1), a.A = a.pre.size(2);
  a.vdiv = vdiv > 0 ? vdiv : R / a.Bv;
  const int64_t Bv = a.Bv, C = a.C, A = a.A;
  switch (site) {
    case Site::Forward:
      TORCH_CHECK(a.gv.scalar_type() == at::kFloat && a.gv.dim() == 3 && a.gv.size(2) == H4,
                  "Gv must be fp32 (Bv, C, 4H)");
      TORCH_CHECK(a.pre.scalar_type() == at::kFloat && a.pre.dim() == 3 && a.pre.size(0) == Bv &&
                      a.pre.size(1) == C, "P must be fp32 (Bv, C, A)");
      TORCH_CHECK(A % 64 == 0 && C >= 1 && C <= 32, "attention: A % 64 == 0 and C <= 32");
      TORCH_CHECK(a.wq.scalar_type() == at::kBFloat16 && a.wq.size(0) == A && a.wq.size(1) == H,
                  "W_q must be bf16 (A, H)");
      TORCH_CHECK(a.wa.scalar_type() == at::kFloat && a.ba.scalar_type() == at::kFloat &&
                      ((a.wa.numel() == A && a.ba.numel() == 1) ||
                       (C > 1 && C <= 8 && a.wa.numel() == C * A && a.ba.numel() == C)),
                  "w_a (A) / b_a (1), or per frame (C, A) / (C), fp32");
      TORCH_CHECK(Bv * a.vdiv == R, "attention needs R == videos x rows per video");
      break;
    case Site::Backward:
      TORCH_CHECK(Bv * a.vdiv == R && a.alpha_all.size(0) == n_steps && a.alpha_all.size(2) == C &&
                      a.q_all.size(2) == A && a.wq.size(0) == A && a.wq.size(1) == H,
                  "attention operand shapes");
      TORCH_CHECK(a.wa.numel() == A || (C > 1 && a.wa.numel() == C * A), "w_a shape");
      break;
    case Site::Beam:
      TORCH_CHECK(Bv * a.vdiv == R && a.gv.size(2) == H4,
                  "att = {Gv (B, C, 4H), P, W_q, w_a, b_a}");
      TORCH_CHECK(A % 64 == 0 && C >= 1 && C <= 32 && a.wq.size(0) == A && a.wq.size(1) == H,
                  "attention shapes");
      TORCH_CHECK(a.wa.numel() == A ||
                      (C > 1 && C <= 8 && a.wa.numel() == C * A && a.ba.numel() == C),
                  "w_a / b_a shapes");
      break;
  }
  a.per_frame = C > 1 && a.wa.numel() == C * A ? 1 : 0;
  a.CPAD = C <= 8 ? 8 : 16;
  return a;
}

inline UpperLayers UpperLayers::parse(const std::vector<at::Tensor>& up, Site site, bool has_att,
                               bool has_s0, int64_t H, int64_t n_steps) {
  UpperLayers u;
  u.up = &up;
  u.per = site == Site::Backward ? 5 : 2;
  TORCH_CHECK(up.size() % u.per == 0,
              site == Site::Backward
                  ? "up = {W, h_all, c_all, gates_all, hd_in} per upper layer"
                  : "up = {[W_ih | W_hh] (4H, 2H), W_hh (4H, H)} per upper layer");
  u.NL = 1 + (int64_t)up.size() / u.per;
  if (u.NL > 1) TORCH_CHECK(!has_att && !has_s0, "stacked layers: no attention / initial state");
  const int64_t H4 = 4 * H;
  for (int64_t l = 1; l < u.NL; ++l) {
    if (site == Site::Forward) {
      const at::Tensor &wu = u(l, 0), &wh = u(l, 1);
      check_cuda(wu, "upper-layer weights");
      check_cuda(wh, "upper-layer W_hh");
      TORCH_CHECK(wu.scalar_type() == at::kBFloat16 && wu.is_contiguous() && wu.size(0) == H4 &&
                      wu.size(1) == 2 * H && wh.scalar_type() == at::kBFloat16 &&
                      wh.is_contiguous() && wh.size(0) == H4 && wh.size(1) == H,
                  "upper layer: [W_ih | W_hh] bf16 (4H, 2H) and W_hh bf16 (4H, H)");
    } else if (site == Site::Backward) {
      TORCH_CHECK(u(l, 0).size(0) == H4 && u(l, 0).size(1) == 2 * H &&
                      u(l, 1).size(0) == n_steps && u(l, 2).size(0) == n_steps &&
                      u(l, 3).size(0) == n_steps && u(l, 4).size(0) == n_steps,
                  "upper-layer operand shapes");
    }
  }
  return u;
}

inline InitState InitState::parse(const std::vector<at::Tensor>& state0, Site site, bool has_att,
                           int64_t rows, int64_t H) {
  InitState s;
  if (state0.empty()) return s;
  s.on = true;
  TORCH_CHECK(state0.size() == 2 && !has_att, "state0 = {h0, c0}, without attention");
  s.h0 = state0[0], s.c0 = state0[1];
  const at::Tensor &h0 = s.h0, &c0 = s.c0;
  switch (site) {
    case Site::Forward:
      check_cuda(h0, "h0");
      check_cuda(c0, "c0");
      TORCH_CHECK(h0.scalar_type() == at::kBFloat16 && h0.is_contiguous() && h0.size(0) == rows &&
                      h0.size(1) == H && c0.scalar_type() == at::kFloat && c0.is_contiguous() &&
                      c0.size(0) == rows && c0.size(1) == H,
                  "h0 bf16 / c0 fp32, contiguous (R, H)");
      break;
    case Site::Backward:
      TORCH_CHECK(h0.size(0) == rows && h0.scalar_type() == at::kBFloat16 && c0.size(0) == rows &&
                      c0.scalar_type() == at::kFloat,
                  "state0 = {h0 bf16, c0 fp32} (R, H)");
      break;
    case Site::Beam:  // per-video state {h0 (B, H), c0 (B, H)}, one copy per beam
      TORCH_CHECK(h0.size(0) == rows && c0.size(0) == rows && h0.size(1) == H && c0.size(1) == H,
                  "state0 = {h0, c0} (B, H), without attention");
      break;
  }
  return s;
}

}  // namespace cst
