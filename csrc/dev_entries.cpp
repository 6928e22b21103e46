// Entries that exist only for tests and microbenchmarks.
#include "engine_internal.h"

namespace cst {

// microbenchmark of the persistent reverse loop alone (random operands of the
// given shape): mean us per launch over `iters` launches; `phases` (int64,
// grid x T x 4, nullable-empty) receives the last launch's per-step stamps
// (step start, team wait done, operands + GEMM done, step published)
double lstm_bwd_loop_bench(int64_t R, int64_t H, int64_t T, int64_t iters, at::Tensor phases,
                           int64_t dbg) {
  TORCH_CHECK(lstm_bwd_loop_ok((int)R, (int)H, (int)T), "lstm_bwd_loop_bench: unsupported shape");
  auto dev = at::Device(at::kCUDA, at::hip::getCurrentHIPStream().device_index());
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  auto b16 = at::TensorOptions().dtype(at::kBFloat16).device(dev);
  at::Tensor dG = at::empty({T, R, 4 * H}, b16);
  at::Tensor whhT = (at::randn({H, 4 * H}, f32) * 0.05).to(at::kBFloat16);
  at::Tensor dh = at::randn({T, R, H}, f32) * 0.01;
  at::Tensor gates = at::rand({T, R, 4 * H}, f32).to(at::kBFloat16);
  at::Tensor c_all = at::randn({T, R, H}, f32);
  at::Tensor dc = at::empty({R, H}, f32);
  at::Tensor rng = at::zeros({2}, at::TensorOptions().dtype(at::kInt).device(dev));
  BwdLoopArgs la{};
  la.dG = reinterpret_cast<uint16_t*>(dG.data_ptr());
  la.whhT = reinterpret_cast<const uint16_t*>(whhT.data_ptr());
  la.dh = dh.data_ptr<float>();
  la.gates = reinterpret_cast<const uint16_t*>(gates.data_ptr());
  la.c_all = c_all.data_ptr<float>();
  la.dc_out = dc.data_ptr<float>();
  la.R = (int)R;
  la.H = (int)H;
  la.T = (int)T;
  la.drop_p = 0.5f;
  la.rng = reinterpret_cast<const uint32_t*>(rng.data_ptr());
  la.cnt = loop_counters(dev.index(), lstm_bwd_loop_counter_ints((int)R, (int)H));
  la.err = device_err_word(dev.index());
  la.poll_bound = poll_bound();
  la.dbg = (int)dbg;
  la.form = dbg >= 8 ? 0 : 1;  // (dbg 8: the K-split form; 0-7: the row-read form's variants)
  if (dbg >= 8) la.dbg = 0;
  if (la.form == 0) la.xb = loop_xb(dev.index(), lstm_bwd_loop_xb_floats((int)R, (int)H));
  hipStream_t st = cur_stream();
  for (int i = 0; i < 3; ++i) launch_lstm_bwd_loop(la, st);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, st);
  for (int64_t i = 0; i < iters; ++i) launch_lstm_bwd_loop(la, st);
  (void)hipEventRecord(e1, st);
  if (phases.defined() && phases.numel() > 0) {
    TORCH_CHECK(phases.scalar_type() == at::kLong && phases.is_cuda() && phases.is_contiguous(),
                "phases: int64 GPU tensor");
    la.phases = phases.data_ptr<int64_t>();
    launch_lstm_bwd_loop(la, st);
  }
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipStreamSynchronize(st);
  return ms * 1e3 / std::max<int64_t>(iters, 1);
}

// the reverse recurrence's kernels one by one (tests/test_gpu_lstm_bwd.py);
// absent optional operands: nullopt or an empty tensor
static bool given(const c10::optional<at::Tensor>& t) {
  return t.has_value() && t->defined() && t->numel() > 0;
}
static bool f32_rows(const at::Tensor& t, int64_t n) {
  return t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n;
}
static bool i32_rows(const at::Tensor& t, int64_t n) {
  return t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() == n;
}
// one-hot operands of NR rows -> DhOneHot (all null when W is absent); the
// tokens of a given weight vector are required and stay below the rows of W
static DhOneHot onehot_operands(const char* who, int64_t NR, int64_t H,
                                const c10::optional<at::Tensor>& W,
                                const c10::optional<at::Tensor>& a,
                                const c10::optional<at::Tensor>& ys,
                                const c10::optional<at::Tensor>& b,
                                const c10::optional<at::Tensor>& yx) {
  DhOneHot oh{};
  if (!given(W)) {
    TORCH_CHECK(!given(a) && !given(b) && !given(ys) && !given(yx), who,
                ": one-hot weights / tokens without oh_W");
    return oh;
  }
  TORCH_CHECK(W->is_cuda() && W->scalar_type() == at::kBFloat16 && W->dim() == 2 &&
                  W->is_contiguous() && W->size(1) == H && W->size(0) > 0,
              who, ": oh_W (V, H) bf16");
  TORCH_CHECK(given(a) || given(b), who, ": oh_W without oh_a / oh_b");
  TORCH_CHECK(given(a) == given(ys) && given(b) == given(yx), who,
              ": oh_a with oh_ys, oh_b with oh_yx");
  oh.W = reinterpret_cast<const uint16_t*>(W->data_ptr());
  if (given(a)) {
    TORCH_CHECK(f32_rows(*a, NR) && i32_rows(*ys, NR) && ys->max().item<int>() < W->size(0), who,
                ": oh_a fp32 / oh_ys int32 (rows), tokens < V");
    oh.a = a->data_ptr<float>();
    oh.ys = ys->data_ptr<int>();
  }
  if (given(b)) {
    TORCH_CHECK(f32_rows(*b, NR) && i32_rows(*yx, NR) && yx->max().item<int>() < W->size(0), who,
                ": oh_b fp32 / oh_yx int32 (rows), tokens < V");
    oh.b = b->data_ptr<float>();
    oh.yx = yx->data_ptr<int>();
  }
  return oh;
}

// ONE launch_lstm_step_bwd on the caller's operands: dg_next (R, KD) bf16 or
// empty (last step: no GEMM), whhT (H, KD) bf16, dh_logit / dc_carry / c_t
// (R, H) fp32, c_prev (R, H) or empty (= 0), gates (R, 4H) bf16 packed 4u + g,
// rng int32 (2); dh_scale (R); one-hot operands (DhOneHot) of the R rows;
// gvb16 (Bv, H, CP, 4) bf16 with vdiv and C: the non-fused attention epilogue
// (AttBwdEpi without flags).  dG (R, KD) is pre-filled with the 16-bit pattern
// `sentinel` (the kernel owes columns [0, 4H) only); the carry is updated on a
// clone.  Returns {dG, dc_carry, dal_part (H / 64, R, CP) or empty}.
std::vector<at::Tensor> lstm_step_bwd_test(
    at::Tensor dg_next, at::Tensor whhT, at::Tensor dh_logit, at::Tensor dc_carry,
    at::Tensor gates, at::Tensor c_t, at::Tensor c_prev, double drop_p, at::Tensor rng,
    int64_t step, int64_t cell, int64_t KD, int64_t sentinel,
    c10::optional<at::Tensor> dh_scale, c10::optional<at::Tensor> oh_W,
    c10::optional<at::Tensor> oh_a, c10::optional<at::Tensor> oh_ys,
    c10::optional<at::Tensor> oh_b, c10::optional<at::Tensor> oh_yx,
    c10::optional<at::Tensor> gvb16, int64_t vdiv, int64_t C) {
  check_cuda(whhT, "whhT");
  check_cuda(dh_logit, "dh_logit");
  check_cuda(dc_carry, "dc_carry");
  check_cuda(gates, "gates");
  check_cuda(c_t, "c_t");
  TORCH_CHECK(dh_logit.scalar_type() == at::kFloat && dh_logit.dim() == 2 &&
                  dh_logit.size(0) > 0 && dh_logit.size(1) > 0 && dh_logit.size(1) % 64 == 0,
              "lstm_step_bwd_test: dh_logit (R, H) fp32, H a multiple of 64");
  const int64_t R = dh_logit.size(0), H = dh_logit.size(1);
  TORCH_CHECK(KD % 64 == 0 && KD >= 4 * H && R * KD * 2 < (1LL << 31) && H * KD * 2 < (1LL << 31),
              "lstm_step_bwd_test: KD a multiple of 64, >= 4H, operands below 2 GB");
  TORCH_CHECK(whhT.scalar_type() == at::kBFloat16 && whhT.dim() == 2 && whhT.size(0) == H &&
                  whhT.size(1) == KD,
              "lstm_step_bwd_test: whhT (H, KD) bf16");
  TORCH_CHECK(f32_rows(dc_carry, R * H) && f32_rows(c_t, R * H) &&
                  gates.scalar_type() == at::kBFloat16 && gates.dim() == 2 && gates.size(0) == R &&
                  gates.size(1) == 4 * H,
              "lstm_step_bwd_test: dc_carry / c_t (R, H) fp32, gates (R, 4H) bf16");
  const bool has_next = dg_next.defined() && dg_next.numel() > 0;
  if (has_next)
    TORCH_CHECK(dg_next.is_cuda() && dg_next.is_contiguous() &&
                    dg_next.scalar_type() == at::kBFloat16 && dg_next.dim() == 2 &&
                    dg_next.size(0) == R && dg_next.size(1) == KD,
                "lstm_step_bwd_test: dg_next (R, KD) bf16");
  const bool has_cp = c_prev.defined() && c_prev.numel() > 0;
  if (has_cp) TORCH_CHECK(f32_rows(c_prev, R * H), "lstm_step_bwd_test: c_prev (R, H) fp32");
  TORCH_CHECK(drop_p >= 0.0 && drop_p < 1.0 && cell >= 0 && cell <= 2 &&
                  step >= 0 && step < (1LL << 31) && sentinel >= 0 && sentinel <= 0xffff,
              "lstm_step_bwd_test: drop_p in [0, 1), cell 0..2, step >= 0, 16-bit sentinel");
  TORCH_CHECK(rng.defined() && rng.numel() == 2, "lstm_step_bwd_test: rng int32 (2)");
  if (given(dh_scale)) TORCH_CHECK(f32_rows(*dh_scale, R), "lstm_step_bwd_test: dh_scale (R) fp32");
  const DhOneHot oh = onehot_operands("lstm_step_bwd_test", R, H, oh_W, oh_a, oh_ys, oh_b, oh_yx);
  at::Tensor dG = at::empty({R, KD}, gates.options());
  dG.view(at::kShort).fill_((int64_t)(int16_t)(uint16_t)sentinel);
  at::Tensor carry = dc_carry.clone();
  at::Tensor dal;
  AttBwdEpi att{};
  const bool has_att = given(gvb16);
  if (has_att) {
    const int64_t CP = C <= 8 ? 8 : 16;
    TORCH_CHECK(C >= 1 && vdiv >= 1 && (KD / 64) % 2 == 0 &&
                    att_bwd_epi_ok((int)vdiv, (int)C, (int)H),
                "lstm_step_bwd_test: attention epilogue shape not supported");
    TORCH_CHECK(gvb16->is_cuda() && gvb16->is_contiguous() &&
                    gvb16->scalar_type() == at::kBFloat16 && gvb16->dim() == 4 &&
                    gvb16->size(0) * vdiv >= R && gvb16->size(1) == H && gvb16->size(2) == CP &&
                    gvb16->size(3) == 4,
                "lstm_step_bwd_test: gvb16 (Bv >= R / vdiv, H, CP, 4) bf16");
    dal = at::full({H / 64, R, CP}, std::nanf(""), dh_logit.options());
    att.gvb16 = reinterpret_cast<const uint16_t*>(gvb16->data_ptr());
    att.vdiv = (int)vdiv;
    att.C = (int)C;
    att.CP = (int)CP;
    att.dal_part = dal.data_ptr<float>();
  } else {
    dal = at::empty({0}, dh_logit.options());
  }
  launch_lstm_step_bwd(has_next ? reinterpret_cast<const uint16_t*>(dg_next.data_ptr()) : nullptr,
                       reinterpret_cast<const uint16_t*>(whhT.data_ptr()),
                       dh_logit.data_ptr<float>(), carry.data_ptr<float>(),
                       reinterpret_cast<const uint16_t*>(gates.data_ptr()), c_t.data_ptr<float>(),
                       has_cp ? c_prev.data_ptr<float>() : nullptr, (int)R, (int)H, (float)drop_p,
                       rng_ptr(rng), (int)step, reinterpret_cast<uint16_t*>(dG.data_ptr()), (int)KD,
                       cur_stream(), (int)cell,
                       given(dh_scale) ? dh_scale->data_ptr<float>() : nullptr,
                       has_att ? &att : nullptr, oh.W != nullptr ? &oh : nullptr);
  return {dG, carry, dal};
}

// ONE launch_lstm_bwd_loop (the fold kernel ahead of it when scale / one-hot
// operands are given): whhT (H, 4H) bf16, dh (T, R, H) fp32 (cloned: the fold
// works in place), gates (T, R, 4H) bf16, c_all (T, R, H) fp32, scale (T, R),
// one-hot operands of all T R rows; form 1 = row-read, 0 = K-split.  Counters,
// exchange slabs, error word and poll bound as the executor takes them.
// Returns {dG (T, R, 4H) bf16, dc_out (R, H), dh as the loop read it}.
std::vector<at::Tensor> lstm_bwd_loop_test(
    at::Tensor whhT, at::Tensor dh, at::Tensor gates, at::Tensor c_all, double drop_p,
    at::Tensor rng, int64_t cell, int64_t form, c10::optional<at::Tensor> scale,
    c10::optional<at::Tensor> oh_W, c10::optional<at::Tensor> oh_a,
    c10::optional<at::Tensor> oh_ys, c10::optional<at::Tensor> oh_b,
    c10::optional<at::Tensor> oh_yx) {
  check_cuda(whhT, "whhT");
  check_cuda(dh, "dh");
  check_cuda(gates, "gates");
  check_cuda(c_all, "c_all");
  TORCH_CHECK(dh.scalar_type() == at::kFloat && dh.dim() == 3 && dh.numel() > 0,
              "lstm_bwd_loop_test: dh (T, R, H) fp32");
  const int64_t T = dh.size(0), R = dh.size(1), H = dh.size(2);
  TORCH_CHECK(T < (1 << 20) && R < (1 << 20) && H <= 512 &&
                  lstm_bwd_loop_ok((int)R, (int)H, (int)T),
              "lstm_bwd_loop_test: unsupported shape");
  TORCH_CHECK(whhT.scalar_type() == at::kBFloat16 && whhT.dim() == 2 && whhT.size(0) == H &&
                  whhT.size(1) == 4 * H,
              "lstm_bwd_loop_test: whhT (H, 4H) bf16");
  TORCH_CHECK(gates.scalar_type() == at::kBFloat16 && gates.dim() == 3 && gates.size(0) == T &&
                  gates.size(1) == R && gates.size(2) == 4 * H && f32_rows(c_all, T * R * H) &&
                  c_all.dim() == 3,
              "lstm_bwd_loop_test: gates (T, R, 4H) bf16, c_all (T, R, H) fp32");
  TORCH_CHECK(drop_p >= 0.0 && drop_p < 1.0 && cell >= 0 && cell <= 2 &&
                  (form == 0 || form == 1),
              "lstm_bwd_loop_test: drop_p in [0, 1), cell 0..2, form 0 / 1");
  TORCH_CHECK(rng.defined() && rng.numel() == 2, "lstm_bwd_loop_test: rng int32 (2)");
  if (given(scale)) TORCH_CHECK(f32_rows(*scale, T * R), "lstm_bwd_loop_test: scale (T, R) fp32");
  const DhOneHot oh = onehot_operands("lstm_bwd_loop_test", T * R, H, oh_W, oh_a, oh_ys, oh_b, oh_yx);
  // (the launcher folds when scale or oh_a is given: oh_b rides on oh_a)
  TORCH_CHECK(oh.b == nullptr || oh.a != nullptr, "lstm_bwd_loop_test: oh_b needs oh_a");
  const int dev = dh.device().index();
  at::Tensor dG = at::empty({T, R, 4 * H}, gates.options());
  dG.view(at::kShort).fill_(-1);  // (a NaN pattern: the loop owes every element)
  at::Tensor dc = at::full({R, H}, std::nanf(""), dh.options());
  at::Tensor dhf = dh.clone();
  BwdLoopArgs la{};
  la.dG = reinterpret_cast<uint16_t*>(dG.data_ptr());
  la.whhT = reinterpret_cast<const uint16_t*>(whhT.data_ptr());
  la.dh = dhf.data_ptr<float>();
  la.scale = given(scale) ? scale->data_ptr<float>() : nullptr;
  la.oh_W = oh.W;
  la.oh_a = oh.a;
  la.oh_ys = oh.ys;
  la.oh_b = oh.b;
  la.oh_yx = oh.yx;
  la.gates = reinterpret_cast<const uint16_t*>(gates.data_ptr());
  la.c_all = c_all.data_ptr<float>();
  la.dc_out = dc.data_ptr<float>();
  la.R = (int)R;
  la.H = (int)H;
  la.T = (int)T;
  la.cell = (int)cell;
  la.drop_p = (float)drop_p;
  la.rng = rng_ptr(rng);
  la.cnt = loop_counters(dev, lstm_bwd_loop_counter_ints((int)R, (int)H));
  la.err = device_err_word(dev);
  la.poll_bound = poll_bound();
  la.form = (int)form;
  if (la.form == 0) la.xb = loop_xb(dev, lstm_bwd_loop_xb_floats((int)R, (int)H));
  launch_lstm_bwd_loop(la, cur_stream());
  return {dG, dc, dhf};
}

// test entry: C (M x N) fp32 = A[:K]^T B[:K]
at::Tensor wgrad_tn(at::Tensor A, at::Tensor B, int64_t M, int64_t N, int64_t K) {
  check_cuda(A, "A");
  check_cuda(B, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.stride(1) == 1 && B.stride(1) == 1 &&
                  A.size(0) >= K && B.size(0) >= K && A.size(1) >= M && B.size(1) >= N,
              "wgrad_tn: operand shapes");
  at::Tensor C = at::empty({M, N}, A.options().dtype(at::kFloat));
  TORCH_CHECK(wgrad_tn_into(A, A.stride(0), B, B.stride(0), M, N, K, C.data_ptr<float>(), N, M,
                            nullptr, 0, cur_stream()),
              "wgrad_tn: shapes not supported (N a multiple of 128, 16-byte rows)");
  return C;
}

// test entry of the row-mapped store: row m of A[:K]^T B[:K] into row rmap[m]
// of out (fp32, >= N columns, any row stride; rmap int32 (M), < 0 = dropped)
void wgrad_tn_rows(at::Tensor A, at::Tensor B, int64_t M, int64_t N, int64_t K, at::Tensor out,
                   at::Tensor rmap) {
  check_cuda(A, "A");
  check_cuda(B, "B");
  check_cuda(out, "out");
  check_cuda(rmap, "rmap");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.stride(1) == 1 && B.stride(1) == 1 &&
                  A.size(0) >= K && B.size(0) >= K && A.size(1) >= M && B.size(1) >= N,
              "wgrad_tn_rows: operand shapes");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && out.stride(1) == 1 &&
                  out.size(1) >= N && rmap.scalar_type() == at::kInt && rmap.is_contiguous() &&
                  rmap.numel() == M,
              "wgrad_tn_rows: out fp32 (rows, >= N), rmap int32 (M)");
  TORCH_CHECK(rmap.max().item<int>() < out.size(0), "wgrad_tn_rows: rmap beyond the rows of out");
  TORCH_CHECK(wgrad_tn_into(A, A.stride(0), B, B.stride(0), M, N, K, out.data_ptr<float>(),
                            out.stride(0), M, nullptr, 0, cur_stream(), nullptr, nullptr,
                            rmap.data_ptr<int>()),
              "wgrad_tn_rows: shapes not supported (N a multiple of 128, 16-byte rows)");
}

// test entry of the fused form: {C (M x N), db (M)} with db[m] = sum_k al[k] A[k][m]
std::vector<at::Tensor> wgrad_tn_colsum(at::Tensor A, at::Tensor B, at::Tensor al, int64_t M,
                                        int64_t N, int64_t K) {
  check_cuda(A, "A");
  check_cuda(B, "B");
  check_cuda(al, "al");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.stride(1) == 1 && B.stride(1) == 1 &&
                  A.size(0) >= K && B.size(0) >= K && A.size(1) >= M && B.size(1) >= N &&
                  al.scalar_type() == at::kFloat && al.is_contiguous() && al.numel() >= K,
              "wgrad_tn_colsum: operand shapes");
  at::Tensor C = at::empty({M, N}, A.options().dtype(at::kFloat));
  at::Tensor db = at::empty({M}, A.options().dtype(at::kFloat));
  TORCH_CHECK(wgrad_tn_into(A, A.stride(0), B, B.stride(0), M, N, K, C.data_ptr<float>(), N, M,
                            nullptr, 0, cur_stream(), al.data_ptr<float>(), db.data_ptr<float>()),
              "wgrad_tn_colsum: shapes not supported (N = 512, 16-byte rows)");
  return {C, db};
}

// stand-in for a collective's kernel on `stream` (0: the current stream):
// `blocks` copying workgroups for `us` microseconds over `buf` (fp32 scratch)
void busy_copy(at::Tensor buf, int64_t blocks, double us, int64_t stream) {
  check_cuda(buf, "buf");
  TORCH_CHECK(buf.scalar_type() == at::kFloat && buf.is_contiguous(), "busy_copy: fp32 scratch");
  launch_busy_copy(buf.data_ptr<float>(), buf.numel(), (int)blocks, us,
                   stream != 0 ? reinterpret_cast<hipStream_t>(stream) : cur_stream());
}

// Microbenchmarks of single kernels (scripts/microbench_kernels.py): mean
// microseconds per launch over `iters` back-to-back launches, HIP events.
template <class F>
static double time_launches(F&& launch, int64_t iters, hipStream_t st) {
  launch(0);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) launch(i);
  (void)hipEventRecord(e1, st);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return 1000.0 * ms / (double)iters;
}

double vocab_fwd_bench(at::Tensor hd, at::Tensor wlog, at::Tensor blog, at::Tensor tgt,
                       int64_t flags, bool save, int64_t iters, int64_t variant) {
  const int64_t R = hd.size(0), H = hd.size(1), V = wlog.size(0);
  TORCH_CHECK(H % 64 == 0 && wlog.size(1) == H && blog.numel() == V, "shapes");
  auto dev = hd.device();
  const int64_t ldl = (V + 7) / 8 * 8;
  at::Tensor logits = save ? at::empty({R, ldl}, hd.options().dtype(at::kHalf)) : at::Tensor();
  const int n_vt = vocab_num_tiles((int)V);
  at::Tensor part = at::empty({(int64_t)n_vt * R * vocab_partial_bytes() / 4},
                              at::TensorOptions().dtype(at::kFloat).device(dev));
  at::Tensor rng = at::full({2}, 1234, at::TensorOptions().dtype(at::kInt).device(dev));
  const int64_t* tg = tgt.defined() && tgt.numel() ? tgt.data_ptr<int64_t>() : nullptr;
  hipStream_t st = cur_stream();
  return time_launches(
      [&](int i) {
        launch_vocab_fwd_variant((int)variant, reinterpret_cast<const uint16_t*>(hd.data_ptr()),
                                 (int)H, (int)R, (int)H,
                                 reinterpret_cast<const uint16_t*>(wlog.data_ptr()),
                                 blog.data_ptr<float>(), (int)V,
                                 save ? reinterpret_cast<uint16_t*>(logits.data_ptr()) : nullptr,
                                 ldl, part.data_ptr(), tg, 1, (int)flags, 1.f, rng_ptr(rng), i, st);
      },
      iters, st);
}

// bias-gradient column sums over the exp store: E (n, R, ldl) bf16, alpha (n*R)
double vgrad_colsum_bench(at::Tensor E, at::Tensor alpha, int64_t V, int64_t iters) {
  check_cuda(E, "E");
  const int64_t NR = E.size(0) * E.size(1), ldl = E.size(2);
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(E.device());
  at::Tensor part = at::empty({vgrad_colsum_blocks(NR), V}, f32), db = at::empty({V}, f32);
  hipStream_t st = cur_stream();
  return time_launches(
      [&](int) {
        launch_vgrad_colsum(reinterpret_cast<const uint16_t*>(E.data_ptr()), ldl, (int)V, NR,
                            alpha.data_ptr<float>(), part.data_ptr<float>(), db.data_ptr<float>(),
                            st);
      },
      iters, st);
}

// Phase stamps of one launch of the MFMA attention workgroups (microbenchmark,
// scripts/microbench_att.py): (Bv * A / 64, 8) int64 wall-clock ticks, phases
// 0 start, 1 operands in LDS, 2 query MFMA, 3 scores, 4 ticket, and for the
// video's last workgroup 5 slot sums, 7 softmax, 6 end (-1 where not reached).
at::Tensor att_mfma_phases(at::Tensor gv, at::Tensor P, at::Tensor wa, at::Tensor ba, int64_t R) {
  check_cuda(gv, "gv");
  const int64_t Bv = gv.size(0), C = gv.size(1), H4 = gv.size(2), A = P.size(2), H = H4 / 4;
  const int vdiv = (int)(R / Bv), CP = C <= 8 ? 8 : 16;
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(gv.device());
  auto bf = gv.options().dtype(at::kBFloat16);
  at::Tensor h = (at::rand({R, H}, f32) * 2 - 1).to(at::kBFloat16);
  at::Tensor wq = (at::randn({A, H}, f32) * 0.05).to(at::kBFloat16);
  at::Tensor gv16 = at::zeros({Bv, H4, CP}, bf), vg = at::empty({R, H4}, bf);
  gv16.narrow(2, 0, C).copy_(gv.transpose(1, 2));
  at::Tensor alpha = at::empty({R, C}, f32), qo = at::empty({R, A}, f32);
  at::Tensor ep = at::empty({Bv, A / 64, 32, CP}, f32);
  at::Tensor cnt = at::zeros({Bv}, f32.dtype(at::kInt));
  at::Tensor dbg = at::full({Bv * (A / 64), 8}, -1, f32.dtype(at::kLong));
  AttMfmaArgs am{reinterpret_cast<const uint16_t*>(h.data_ptr()),
                 reinterpret_cast<const uint16_t*>(wq.data_ptr()), P.data_ptr<float>(),
                 wa.data_ptr<float>(), ba.data_ptr<float>(),
                 reinterpret_cast<const uint16_t*>(gv16.data_ptr()), (int)H, (int)A, (int)C, CP,
                 (int)H4, vdiv, (int)Bv, reinterpret_cast<uint16_t*>(vg.data_ptr()),
                 alpha.data_ptr<float>(), qo.data_ptr<float>(), ep.data_ptr<float>(),
                 cnt.data_ptr<int>(), nullptr, nullptr};
  hipStream_t st = cur_stream();
  launch_att_mfma_fwd(am, st);  // warm-up
  (void)hipStreamSynchronize(st);
  am.dbg = dbg.data_ptr<int64_t>();
  launch_att_mfma_fwd(am, st);
  (void)hipStreamSynchronize(st);
  return dbg;
}

// temporal attention kernels alone (one decode / reverse step): Gv (Bv, C, 4H)
// fp32, P (Bv, C, A), q (R, A), w_a (A), b_a (1); which = 0: forward
// (accumulating into pre), 1: backward (dG rows (R, 4H + A) bf16, dq written)
double att_bench(at::Tensor gv, at::Tensor P, at::Tensor q, at::Tensor wa, at::Tensor ba,
                 int64_t R, int64_t which, int64_t iters) {
  check_cuda(gv, "gv");
  const int64_t Bv = gv.size(0), C = gv.size(1), H4 = gv.size(2), A = P.size(2);
  TORCH_CHECK(R % Bv == 0 && q.size(0) == R && q.size(1) == A, "att_bench shapes");
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(gv.device());
  const int vdiv = (int)(R / Bv);
  at::Tensor pre = at::zeros({R, H4}, f32), alpha = at::full({R, C}, 1.f / C, f32);
  at::Tensor dG = at::zeros({R, H4 + A}, gv.options().dtype(at::kBFloat16));
  const int rpw_b = which == 4 ? 2 : ATT_BWD_RPW;  // 1: backward, 4: backward at 2 rows
  const int64_t nwg = Bv * att_groups(vdiv, rpw_b);
  at::Tensor dpp = at::zeros({nwg, C, A}, f32), dwp = at::zeros({nwg, A}, f32),
             dbp = at::zeros({nwg, 1}, f32);
  hipStream_t st = cur_stream();
  const int64_t H = H4 / 4;
  if (which == 5 || which == 6) {  // MFMA path: att_mfma forward workgroups / att_bwd_mfma
    auto bf = gv.options().dtype(at::kBFloat16);
    const int CP = C <= 8 ? 8 : 16;
    at::Tensor h = (at::rand({R, H}, f32) * 2 - 1).to(at::kBFloat16);
    at::Tensor wq = (at::randn({A, H}, f32) * 0.05).to(at::kBFloat16);
    at::Tensor gv16 = at::zeros({Bv, H4, CP}, bf), vg = at::empty({R, H4}, bf);
    gv16.narrow(2, 0, C).copy_(gv.transpose(1, 2));
    at::Tensor qo = at::empty({R, A}, f32), dal = at::randn({H / 64, R, CP}, f32);
    at::Tensor dP = at::zeros({Bv, C, A}, f32), dwa = at::zeros({Bv, A}, f32),
               dba = at::zeros({Bv, 1}, f32);
    at::Tensor ep = at::empty({Bv, A / 64, 32, CP}, f32);
    at::Tensor cnt = at::zeros({Bv}, f32.dtype(at::kInt));
    AttMfmaArgs am{reinterpret_cast<const uint16_t*>(h.data_ptr()),
                   reinterpret_cast<const uint16_t*>(wq.data_ptr()), P.data_ptr<float>(),
                   wa.data_ptr<float>(), ba.data_ptr<float>(),
                   reinterpret_cast<const uint16_t*>(gv16.data_ptr()), (int)H, (int)A, (int)C, CP,
                   (int)H4, vdiv, (int)Bv, reinterpret_cast<uint16_t*>(vg.data_ptr()),
                   alpha.data_ptr<float>(), qo.data_ptr<float>(), ep.data_ptr<float>(),
                   cnt.data_ptr<int>()};
    return time_launches(
        [&](int) {
          if (which == 5)
            launch_att_mfma_fwd(am, st);
          else
            launch_att_bwd_mfma(dal.data_ptr<float>(), (int)(H / 64), (int)R,
                                alpha.data_ptr<float>(), q.data_ptr<float>(), P.data_ptr<float>(),
                                wa.data_ptr<float>(), (int)Bv, vdiv, (int)C, CP, (int)A, (int)H4,
                                reinterpret_cast<uint16_t*>(dG.data_ptr()), (int)(H4 + A), 1,
                                dP.data_ptr<float>(), dwa.data_ptr<float>(),
                                dba.data_ptr<float>(), st);
        },
        iters, st);
  }
  return time_launches(
      [&](int) {
        if (which != 1 && which != 4)  // forward at 4 (0), 2 (2) or 1 (3) rows per workgroup
          launch_att_fwd(gv.data_ptr<float>(), P.data_ptr<float>(), q.data_ptr<float>(), nullptr,
                         wa.data_ptr<float>(), ba.data_ptr<float>(), (int)Bv, vdiv, (int)C, (int)A,
                         (int)H4, pre.data_ptr<float>(), alpha.data_ptr<float>(), st, 1, 0,
                         which == 2 ? 2 : which == 3 ? 1 : 4);
        else
          launch_att_bwd(reinterpret_cast<uint16_t*>(dG.data_ptr()), (int)(H4 + A),
                         gv.data_ptr<float>(), P.data_ptr<float>(), q.data_ptr<float>(),
                         alpha.data_ptr<float>(), wa.data_ptr<float>(), (int)Bv, vdiv, (int)C,
                         (int)A, (int)H4, 1, dpp.data_ptr<float>(), dwp.data_ptr<float>(),
                         dbp.data_ptr<float>(), st, 0, rpw_b);
      },
      iters, st);
}

// counting sort of n token ids < V (the embedding-gradient grouping)
double token_sort_bench(at::Tensor toks, int64_t V, int64_t iters) {
  check_cuda(toks, "toks");
  const int64_t N = toks.numel();
  auto i32 = at::TensorOptions().dtype(at::kInt).device(toks.device());
  at::Tensor ws = at::empty({2 * V + 1}, i32), stok = at::empty({N}, i32), srow = at::empty({N}, i32);
  hipStream_t st = cur_stream();
  return time_launches(
      [&](int) {
        launch_token_sort(toks.data_ptr<int64_t>(), (int)N, (int)V, ws.data_ptr<int>(),
                          stok.data_ptr<int>(), srow.data_ptr<int>(), st);
      },
      iters, st);
}

// the vocab projection + sampler/argmax + combine alone (tests of the exact
// two-level sampler): rows hd (R, H) bf16 -> {token (R) int64, lse (R)}.
// mode: SEL_SAMPLE_H (1) or SEL_GREEDY_H (2).
// MFMA temporal-attention workgroups as a launch of their own (tests /
// microbenchmarks of kernels/att_mfma.h): h (R, H) bf16, wq (A, H) bf16,
// P (Bv, C, A), wa (A), ba (1) fp32, gv (Bv, C, 4H) fp32 ->
// {vg (R, 4H) bf16, alpha (R, C), q (R, A)}
std::vector<at::Tensor> att_mfma_fwd(at::Tensor h, at::Tensor wq, at::Tensor P, at::Tensor wa,
                                     at::Tensor ba, at::Tensor gv, int64_t whole) {
  for (auto* t : {&h, &wq, &P, &wa, &ba, &gv}) check_cuda(*t, "att_mfma operand");
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && wq.scalar_type() == at::kBFloat16 &&
                  P.scalar_type() == at::kFloat && wa.scalar_type() == at::kFloat &&
                  ba.scalar_type() == at::kFloat && gv.scalar_type() == at::kFloat,
              "att_mfma: h / wq bf16, P / wa / ba / gv fp32");
  const int64_t R = h.size(0), H = h.size(1), A = wq.size(0), Bv = P.size(0), C = P.size(1);
  TORCH_CHECK(wq.size(1) == H && P.size(2) == A && wa.numel() == A && ba.numel() == 1 &&
                  gv.size(0) == Bv && gv.size(1) == C && gv.size(2) == 4 * H && R % Bv == 0,
              "att_mfma: operand shapes");
  const int vdiv = (int)(R / Bv), CP = C <= 8 ? 8 : 16;
  TORCH_CHECK(att_mfma_fwd_ok(vdiv, (int)C, (int)A, (int)H, 0), "att_mfma: unsupported shape");
  at::Tensor gv16 = at::zeros({Bv, 4 * H, CP}, h.options());
  gv16.narrow(2, 0, C).copy_(gv.transpose(1, 2));
  at::Tensor vg = at::empty({R, 4 * H}, h.options());
  at::Tensor alpha = at::empty({R, C}, P.options()), q = at::empty({R, A}, P.options());
  at::Tensor ep = at::empty({Bv, A / 64, 32, CP}, P.options());
  at::Tensor cnt = at::zeros({Bv}, P.options().dtype(at::kInt));
  AttMfmaArgs a{reinterpret_cast<const uint16_t*>(h.data_ptr()),
                reinterpret_cast<const uint16_t*>(wq.data_ptr()), P.data_ptr<float>(),
                wa.data_ptr<float>(), ba.data_ptr<float>(),
                reinterpret_cast<const uint16_t*>(gv16.data_ptr()), (int)H, (int)A, (int)C, CP,
                (int)(4 * H), vdiv, (int)Bv, reinterpret_cast<uint16_t*>(vg.data_ptr()),
                alpha.data_ptr<float>(), q.data_ptr<float>(), ep.data_ptr<float>(),
                cnt.data_ptr<int>()};
  a.whole = whole < 0 ? att_mfma_whole_default((int)C, (int)H) : (whole != 0 ? 1 : 0);
  launch_att_mfma_fwd(a, cur_stream());
  return {vg, alpha, q};
}

std::vector<at::Tensor> vocab_select(at::Tensor hd, at::Tensor wlog, at::Tensor blog,
                                     at::Tensor rng, int64_t mode, double temperature,
                                     int64_t step, int64_t top_k, double top_p) {
  check_cuda(hd, "hd");
  check_cuda(wlog, "wlog");
  TORCH_CHECK(hd.scalar_type() == at::kBFloat16 && wlog.scalar_type() == at::kBFloat16 &&
                  blog.scalar_type() == at::kFloat, "bf16 hd / W, fp32 bias");
  TORCH_CHECK(mode == SEL_SAMPLE_H || mode == SEL_GREEDY_H, "mode: 1 sample, 2 greedy");
  const int64_t R = hd.size(0), H = hd.size(1), V = wlog.size(0);
  TORCH_CHECK(H % 64 == 0 && wlog.size(1) == H && blog.numel() == V, "shapes");
  auto dev = hd.device();
  const int n_vt = vocab_num_tiles((int)V);
  at::Tensor part = at::empty({(int64_t)n_vt * R * vocab_partial_bytes() / 4},
                              at::TensorOptions().dtype(at::kFloat).device(dev));
  at::Tensor tok = at::zeros({R, 1}, at::TensorOptions().dtype(at::kLong).device(dev));
  at::Tensor lse = at::empty({R}, at::TensorOptions().dtype(at::kFloat).device(dev));
  hipStream_t st = cur_stream();
  if (top_k > 0) {
    // truncated sampling (kernels/topk_sample.hip): the VF_TOPK vocab launch's
    // tile candidates + partials -> {token, lse, log-prob of the token}
    TORCH_CHECK(mode == SEL_SAMPLE_H, "top_k: sampling mode only");
    TORCH_CHECK(top_k <= 8 && top_k <= V, "top_k must be in [1, min(8, V)]");
    TORCH_CHECK(top_p > 0.0 && top_p <= 1.0 && temperature > 0.0, "top_p in (0, 1], temperature > 0");
    at::Tensor cand = at::empty({(int64_t)n_vt * R * top_k * 2}, lse.options());
    at::Tensor lp = at::empty({R}, lse.options());
    launch_vocab_fwd(reinterpret_cast<const uint16_t*>(hd.data_ptr()), (int)H, (int)R, (int)H,
                     reinterpret_cast<const uint16_t*>(wlog.data_ptr()), blog.data_ptr<float>(),
                     (int)V, reinterpret_cast<uint16_t*>(cand.data_ptr()), (V + 7) / 8 * 8,
                     part.data_ptr(), nullptr, 0, VF_TOPK_H | ((int)top_k << 8), 1.f, nullptr,
                     (int)step, st);
    TopkSampleArgs sa{reinterpret_cast<const VocabPartial*>(part.data_ptr()),
                      reinterpret_cast<const float2*>(cand.data_ptr()), n_vt, (int)R, (int)top_k,
                      (int)V, (float)top_p, (float)(1.0 / temperature), rng_ptr(rng), (int)step,
                      nullptr, tok.data_ptr<int64_t>(), 1, nullptr, lp.data_ptr<float>(), 1,
                      lse.data_ptr<float>()};
    launch_topk_sample(sa, st);
    return {tok.view({R}), lse, lp};
  }
  launch_vocab_fwd(reinterpret_cast<const uint16_t*>(hd.data_ptr()), (int)H, (int)R, (int)H,
                   reinterpret_cast<const uint16_t*>(wlog.data_ptr()), blog.data_ptr<float>(),
                   (int)V, nullptr, 0, part.data_ptr(), nullptr, 0, mode == SEL_SAMPLE_H ? 1 : 2,
                   (float)(1.0 / temperature), rng_ptr(rng), (int)step, st);
  launch_vocab_combine(part.data_ptr(), n_vt, (int)R, lse.data_ptr<float>(),
                       tok.data_ptr<int64_t>(), 1, nullptr, 0, nullptr, 0, nullptr, 0, (int)mode,
                       0.f, rng_ptr(rng), (int)step, nullptr, 0, nullptr, st);
  return {tok.view({R}), lse};
}

// ensemble_topk_kernel alone (tests): M hand-made (R, ldl) fp32 logits tensors,
// M (R) LSE vectors and the M log-weights -> {top_v (R, K), top_i (R, K)}.
// unfinished (R) uint8 given (K = 1): the greedy epilogue too, the mask updated
// in place -> {top_v, top_i, tok (R), lp (R), next_tok (R)}.  baseline (M = 1):
// beam_topk_kernel on the same input instead, the code this kernel is measured
// against (scripts/microbench_ensemble.py).
std::vector<at::Tensor> ensemble_topk_test(std::vector<at::Tensor> logits,
                                           std::vector<at::Tensor> lse, std::vector<double> logw,
                                           int64_t V, int64_t K,
                                           c10::optional<at::Tensor> unfinished, bool baseline) {
  const int64_t M = (int64_t)logits.size();
  TORCH_CHECK(M >= 1 && M <= ENS_MAXM, "ensemble: 1 to 8 members, got ", M);
  TORCH_CHECK((int64_t)lse.size() == M && (int64_t)logw.size() == M,
              "ensemble: one LSE vector and one log-weight per member");
  TORCH_CHECK(K >= 1 && K <= 16, "ensemble: K must be in [1, 16]");
  TORCH_CHECK(K <= V, "ensemble: K > vocab_size");
  for (double w : logw) TORCH_CHECK(std::isfinite(w), "ensemble: non-finite log-weight");
  const int64_t R = logits[0].size(0);
  EnsembleTopkArgs ea{};
  for (int64_t m = 0; m < M; ++m) {
    check_cuda(logits[m], "logits");
    check_cuda(lse[m], "lse");
    TORCH_CHECK(logits[m].scalar_type() == at::kFloat && logits[m].dim() == 2 &&
                    logits[m].is_contiguous() && logits[m].size(0) == R && logits[m].size(1) >= V,
                "ensemble: logits fp32 (R, ldl >= V), contiguous");
    TORCH_CHECK(lse[m].scalar_type() == at::kFloat && lse[m].is_contiguous() && lse[m].numel() == R,
                "ensemble: lse fp32 (R)");
    ea.logits[m] = logits[m].data_ptr<float>();
    ea.ldl[m] = logits[m].size(1);
    ea.lse[m] = lse[m].data_ptr<float>();
    ea.logw[m] = (float)logw[m];
  }
  ea.M = (int)M, ea.V = (int)V, ea.R = (int)R, ea.K = (int)K;
  at::Tensor top_v = at::empty({R, K}, logits[0].options());
  at::Tensor top_i = at::empty({R, K}, logits[0].options().dtype(at::kInt));
  ea.top_v = top_v.data_ptr<float>();
  ea.top_i = top_i.data_ptr<int>();
  std::vector<at::Tensor> out = {top_v, top_i};
  if (baseline) {
    TORCH_CHECK(M == 1 && !(unfinished.has_value() && unfinished->defined()),
                "ensemble: the beam_topk baseline is one member, no epilogue");
    launch_beam_topk(ea.logits[0], ea.ldl[0], (int)V, (int)R, (int)K, ea.lse[0], ea.top_v,
                     ea.top_i, cur_stream());
    return out;
  }
  if (unfinished.has_value() && unfinished->defined()) {
    TORCH_CHECK(K == 1, "ensemble: the greedy epilogue is K = 1");
    TORCH_CHECK(unfinished->is_cuda() && unfinished->scalar_type() == at::kByte &&
                    unfinished->is_contiguous() && unfinished->numel() == R,
                "ensemble: unfinished uint8 (R)");
    at::Tensor tok = at::empty({R}, logits[0].options().dtype(at::kLong));
    at::Tensor lp = at::empty({R}, logits[0].options());
    at::Tensor next = at::empty({R}, logits[0].options().dtype(at::kLong));
    ea.unfinished = unfinished->data_ptr<uint8_t>();
    ea.seq_out = tok.data_ptr<int64_t>();
    ea.lp_out = lp.data_ptr<float>();
    ea.out_stride = 1;
    ea.next_tok = next.data_ptr<int64_t>();
    out.insert(out.end(), {tok, lp, next});
  }
  launch_ensemble_topk(ea, cur_stream());
  return out;
}

// One decode step for tests: the decode launch + vocab_combine_kernel.  save: 0 none, 1 fp16 logits, 2 exp store
// (eoff given).  Cell (ptab defined): the next step's cell from c_prev and
// the chosen tokens (dropout drop_p, step key `step + 1`).  eos: 0 no
// end-of-sequence rules; 1 / 2 the all-rows-ended counter with a live / dead
// previous step; unfinished (R) uint8 nullable: the per-row mask, updated in
// place.  Returns {lse, tok, g_sel, g_xe, saved rows (R, ldl), pre (R, 4H),
// n_parts, h, c, h_drop, gates, counts, part}.  want_xe: g_xe is asked for
// (given tgt); the launch gets the target under the executor's rule
// (vocab_step_reads_target), the combine always.
std::vector<at::Tensor> decode_step_test(at::Tensor hd, at::Tensor h, at::Tensor wlog,
                                         at::Tensor blog, at::Tensor whh, at::Tensor vgate,
                                         int64_t vdiv, at::Tensor tgt, at::Tensor eoff,
                                         int64_t save, int64_t mode, int64_t step, at::Tensor rng,
                                         at::Tensor ptab, at::Tensor c_prev, double drop_p,
                                         int64_t cell, int64_t eos, at::Tensor unfinished,
                                         double ss_prob, bool want_xe) {
  check_cuda(hd, "hd");
  check_cuda(wlog, "wlog");
  const int64_t R = hd.size(0), H = hd.size(1), V = wlog.size(0);
  TORCH_CHECK(hd.scalar_type() == at::kBFloat16 && wlog.scalar_type() == at::kBFloat16 &&
                  hd.is_contiguous() && wlog.is_contiguous() && wlog.size(1) == H &&
                  blog.scalar_type() == at::kFloat && blog.numel() == V, "hd / wlog / blog");
  const bool lstm = whh.defined() && whh.numel() > 0;
  if (lstm)
    TORCH_CHECK(h.scalar_type() == at::kBFloat16 && h.is_contiguous() && h.sizes() == hd.sizes() &&
                    whh.scalar_type() == at::kBFloat16 && whh.is_contiguous() &&
                    whh.size(0) == 4 * H && whh.size(1) == H, "h / whh");
  const bool has_vg = vgate.defined() && vgate.numel() > 0;
  if (has_vg)
    TORCH_CHECK(vgate.scalar_type() == at::kFloat && vgate.is_contiguous() &&
                    vgate.size(0) * vdiv == R && vgate.size(1) == 4 * H, "vgate (R / vdiv, 4H)");
  const bool has_tgt = tgt.defined() && tgt.numel() > 0;
  if (has_tgt) TORCH_CHECK(tgt.scalar_type() == at::kLong && tgt.numel() == R, "tgt (R) int64");
  if (save == 2)
    TORCH_CHECK(eoff.defined() && eoff.scalar_type() == at::kFloat && eoff.numel() == R, "eoff (R)");
  const bool do_cell = ptab.defined() && ptab.numel() > 0;
  if (do_cell) {
    TORCH_CHECK(lstm, "the cell needs the recurrent part");
    check_cuda(ptab, "ptab");
    check_cuda(c_prev, "c_prev");
    TORCH_CHECK(ptab.scalar_type() == at::kHalf && ptab.size(0) == V && ptab.size(1) == 4 * H &&
                    c_prev.scalar_type() == at::kFloat && c_prev.numel() == R * H,
                "ptab (V, 4H) fp16 / c_prev (R, H) fp32");
  }
  const bool has_unf = unfinished.defined() && unfinished.numel() > 0;
  if (has_unf)
    TORCH_CHECK(unfinished.is_cuda() && unfinished.scalar_type() == at::kByte &&
                    unfinished.numel() == R, "unfinished (R) uint8");
  auto dev = hd.device();
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  auto bf = at::TensorOptions().dtype(at::kBFloat16).device(dev);
  const int64_t ldl = (V + 63) / 64 * 64;
  at::Tensor part = at::empty({(int64_t)vocab_part_slots((int)V) * R * vocab_partial_bytes() / 4}, f32);
  at::Tensor saved = save ? at::zeros({R, ldl}, at::TensorOptions()
                                                    .dtype(save == 2 ? at::kBFloat16 : at::kHalf)
                                                    .device(dev))
                          : at::Tensor();
  at::Tensor pre = lstm ? at::zeros({R, 4 * H}, f32) : at::Tensor();
  at::Tensor lse = at::empty({R}, f32), gsel = at::zeros({R}, f32), gxe = at::zeros({R}, f32);
  at::Tensor tok = at::zeros({R}, at::TensorOptions().dtype(at::kLong).device(dev));
  at::Tensor h_out, c_out, hdrop, gates;
  if (do_cell) {
    h_out = at::zeros({R, H}, bf);
    c_out = at::zeros({R, H}, f32);
    hdrop = at::zeros({R, H}, bf);
    gates = at::zeros({R, 4 * H}, bf);
  }
  // counts: steps 0..2 of the end-of-sequence flags; this step is count step 2
  const int cps = combine_count_ints_per_step();
  at::Tensor counts = at::zeros({3 * cps}, at::TensorOptions().dtype(at::kInt).device(dev));
  if (eos == 1) counts.narrow(0, cps, 1).fill_(1);  // a live row at the previous step
  int* CNT = eos ? counts.data_ptr<int>() : nullptr;
  hipStream_t st = cur_stream();
  const int flags = (mode == SEL_SAMPLE_H || mode == SEL_SS_H ? 1 : 0) |
                    (mode == SEL_GREEDY_H ? 2 : 0) | (save == 2 ? 16 : 0);
  const int64_t* TG = has_tgt ? tgt.data_ptr<int64_t>() : nullptr;
  const bool xe = has_tgt && want_xe;
  const int64_t* TGX = vocab_step_reads_target(xe, true, (int)mode) ? TG : nullptr;
  uint8_t* UNF = has_unf ? unfinished.data_ptr<uint8_t>() : nullptr;
  const int n = launch_vocab_lstm_fwd(
      reinterpret_cast<const uint16_t*>(hd.data_ptr()), (int)H, (int)R, (int)H,
      reinterpret_cast<const uint16_t*>(wlog.data_ptr()), blog.data_ptr<float>(), (int)V,
      save ? reinterpret_cast<uint16_t*>(saved.data_ptr()) : nullptr, ldl, part.data_ptr(), TGX, 1,
      flags, 1.f, rng_ptr(rng), (int)step,
      lstm ? reinterpret_cast<const uint16_t*>(h.data_ptr()) : nullptr,
      lstm ? reinterpret_cast<const uint16_t*>(whh.data_ptr()) : nullptr,
      has_vg ? vgate.data_ptr<float>() : nullptr, (int)vdiv, lstm ? pre.data_ptr<float>() : nullptr,
      st, 0, nullptr, save == 2 ? eoff.data_ptr<float>() : nullptr, nullptr);
  CellLaunch cl{};
  if (do_cell)
    cl = CellLaunch{pre.data_ptr<float>(), reinterpret_cast<const uint16_t*>(ptab.data_ptr()),
                    c_prev.data_ptr<float>(), c_out.data_ptr<float>(),
                    reinterpret_cast<uint16_t*>(h_out.data_ptr()),
                    reinterpret_cast<uint16_t*>(hdrop.data_ptr()), (int)H,
                    reinterpret_cast<uint16_t*>(gates.data_ptr()), (int)H, (float)drop_p,
                    (int)step + 1, (int)cell, nullptr, 0};
  launch_vocab_combine(part.data_ptr(), n, (int)R, lse.data_ptr<float>(), tok.data_ptr<int64_t>(),
                       1, gsel.data_ptr<float>(), 1, xe ? gxe.data_ptr<float>() : nullptr, 1,
                       TG, 1, (int)mode, (float)ss_prob, rng_ptr(rng), (int)step, CNT, 2, UNF, st,
                       do_cell ? &cl : nullptr);
  return {lse, tok, gsel, gxe, saved, pre, at::full({1}, n, at::TensorOptions().dtype(at::kLong)),
          h_out, c_out, hdrop, gates, counts, part};
}

// the counting sort itself, for tests: returns {stok, srow} (int32)
std::vector<at::Tensor> token_sort(at::Tensor toks, int64_t V) {
  check_cuda(toks, "toks");
  TORCH_CHECK(toks.scalar_type() == at::kLong, "int64 token ids");
  const int64_t N = toks.numel();
  auto i32 = at::TensorOptions().dtype(at::kInt).device(toks.device());
  at::Tensor ws = at::empty({2 * V + 1}, i32), stok = at::empty({N}, i32), srow = at::empty({N}, i32);
  launch_token_sort(toks.data_ptr<int64_t>(), (int)N, (int)V, ws.data_ptr<int>(),
                    stok.data_ptr<int>(), srow.data_ptr<int>(), cur_stream());
  return {stok, srow};
}

// per-token row sums for tests: x (N, C) bf16 (rows x.stride(0) apart: a
// column slice of a wider tensor will do), toks (N) int64 -> S (V, C) bf16
at::Tensor token_group_sum(at::Tensor x, at::Tensor toks, int64_t V) {
  check_cuda(toks, "toks");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 &&
                  x.stride(1) == 1 && x.stride(0) >= x.size(1) &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x: (N, C) bf16, unit column stride, 16-byte aligned");
  TORCH_CHECK(toks.scalar_type() == at::kLong && toks.numel() == x.size(0), "toks: (N) int64");
  const int64_t N = toks.numel(), C = x.size(1);
  auto i32 = at::TensorOptions().dtype(at::kInt).device(toks.device());
  at::Tensor ws = at::empty({2 * V + 1}, i32), stok = at::empty({N}, i32), srow = at::empty({N}, i32);
  at::Tensor S = at::empty({V, C}, x.options());
  at::Tensor S64 = at::empty({V, C}, x.options().dtype(at::kDouble));
  hipStream_t st = cur_stream();
  launch_token_sort(toks.data_ptr<int64_t>(), (int)N, (int)V, ws.data_ptr<int>(),
                    stok.data_ptr<int>(), srow.data_ptr<int>(), st);
  launch_token_long_zero(ws.data_ptr<int>(), (int)V, (int)C, S64.data_ptr<double>(), st);
  launch_token_group_sum(reinterpret_cast<const uint16_t*>(x.data_ptr()), (int)C, x.stride(0),
                         stok.data_ptr<int>(), srow.data_ptr<int>(), (int)N, ws.data_ptr<int>(),
                         (int)V, reinterpret_cast<uint16_t*>(S.data_ptr()), S64.data_ptr<double>(),
                         st);
  return S;
}

// vgrad_onehot (+ vgrad_fix when hd is given) alone, for tests: E (n, R, ldl)
// bf16 folded in place; lse (n, R); y_sel / dg_sel (R, T_sel) or both empty;
// labels (R, >= n + 1) int64 / dg_xe (R, >= n) with their own row strides, or
// both empty (y_xe = labels + 1 as in the backward's onehot_pass).  hd (n R, H)
// bf16 + wlog (V, H) bf16 + blog (V) + fix_total (int32 word) switch the range
// guard on.  forward_x: the one-hot weights / tokens are written out too, and
// with the guard the listed rows of X (n R, H) fp32 (empty: zeros) recomputed.
// Returns {alpha (n R), fix (1 + n R int32)[, oh_a, oh_ys, oh_b, oh_yx, X]}.
// ls_eps > 0 (label smoothing, kernels/label_smooth.hip): dg_xe is the gradient
// of the smoothed target log-prob -- the one-hot weight of the fold / oh_b is
// (1 - ls_eps) dg_xe, alpha keeps the total weight --, and X (n R, H) fp32,
// required then, gets the shift X_r += (ls_eps dg_r / alpha_r) ls_wbar[0 .. H)
// after the fold and the guard (ls_wbar: fp32, >= H + 1); X is returned last
// in every mode.
std::vector<at::Tensor> vgrad_fold(at::Tensor E, at::Tensor lse, at::Tensor y_sel,
                                   at::Tensor dg_sel, at::Tensor labels, at::Tensor dg_xe,
                                   int64_t V, int64_t zero_off, at::Tensor hd, at::Tensor wlog,
                                   at::Tensor blog, at::Tensor fix_total, bool forward_x,
                                   at::Tensor X, double ls_eps,
                                   c10::optional<at::Tensor> ls_wbar) {
  check_cuda(E, "E");
  check_cuda(lse, "lse");
  TORCH_CHECK(E.scalar_type() == at::kBFloat16 && E.dim() == 3, "vgrad_fold: E (n, R, ldl) bf16");
  const int64_t n = E.size(0), R = E.size(1), ldl = E.size(2), NR = n * R;
  TORCH_CHECK(NR > 0 && V > 0 && V <= ldl && lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == n && lse.size(1) == R,
              "vgrad_fold: V <= ldl, lse (n, R) fp32");
  auto in_vocab = [&](const at::Tensor& t) { return t.max().item<int64_t>() < V; };
  const bool has_sel = dg_sel.defined() && dg_sel.numel() > 0;
  const bool has_xe = dg_xe.defined() && dg_xe.numel() > 0;
  int64_t T_sel = 0;
  if (has_sel) {
    check_cuda(y_sel, "y_sel");
    check_cuda(dg_sel, "dg_sel");
    T_sel = y_sel.dim() == 2 ? y_sel.size(1) : 0;
    TORCH_CHECK(y_sel.scalar_type() == at::kLong && dg_sel.scalar_type() == at::kFloat &&
                    y_sel.dim() == 2 && y_sel.size(0) == R && T_sel > 0 &&
                    dg_sel.sizes() == y_sel.sizes() && in_vocab(y_sel),
                "vgrad_fold: y_sel int64 / dg_sel fp32 (R, T_sel), tokens < V");
  }
  if (has_xe) {
    TORCH_CHECK(labels.is_cuda() && dg_xe.is_cuda() && labels.scalar_type() == at::kLong &&
                    dg_xe.scalar_type() == at::kFloat && labels.dim() == 2 && dg_xe.dim() == 2 &&
                    labels.stride(1) == 1 && dg_xe.stride(1) == 1 && labels.size(0) == R &&
                    dg_xe.size(0) == R && labels.size(1) >= n + 1 && dg_xe.size(1) >= n &&
                    labels.stride(0) >= labels.size(1) && dg_xe.stride(0) >= dg_xe.size(1) &&
                    in_vocab(labels),
                "vgrad_fold: labels int64 (R, >= n + 1) / dg_xe fp32 (R, >= n), tokens < V");
  }
  const bool guard = hd.defined() && hd.numel() > 0;
  int64_t H = 0;
  if (guard) {
    check_cuda(hd, "hd");
    check_cuda(wlog, "wlog");
    check_cuda(blog, "blog");
    check_cuda(fix_total, "fix_total");
    H = hd.dim() == 2 ? hd.size(1) : 0;
    TORCH_CHECK(hd.scalar_type() == at::kBFloat16 && hd.dim() == 2 && hd.size(0) == NR &&
                    wlog.scalar_type() == at::kBFloat16 && wlog.dim() == 2 && wlog.size(0) == V &&
                    wlog.size(1) == H && blog.scalar_type() == at::kFloat && blog.numel() == V &&
                    fix_total.scalar_type() == at::kInt && fix_total.numel() >= 1,
                "vgrad_fold: hd (n R, H) / wlog (V, H) bf16, blog (V) fp32, fix_total int32");
  }
  auto dev = E.device();
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  auto i32 = at::TensorOptions().dtype(at::kInt).device(dev);
  at::Tensor alpha = at::empty({NR}, f32), fix = at::zeros({1 + NR}, i32);
  at::Tensor oh_a, oh_ys, oh_b, oh_yx;
  if (forward_x) {
    oh_a = at::empty({NR}, f32), oh_b = at::empty({NR}, f32);
    oh_ys = at::empty({NR}, i32), oh_yx = at::empty({NR}, i32);
    if (guard) {
      if (X.defined() && X.numel() > 0) {
        check_cuda(X, "X");
        TORCH_CHECK(X.scalar_type() == at::kFloat && X.dim() == 2 && X.size(0) == NR &&
                        X.size(1) == H, "vgrad_fold: X (n R, H) fp32");
      } else {
        X = at::zeros({NR, H}, f32);
      }
    }
  }
  const bool have_x = forward_x && guard;
  const bool ls = ls_eps > 0.0;
  if (ls) {
    TORCH_CHECK(ls_eps < 1.0 && has_xe && X.defined() && X.is_cuda() &&
                    X.scalar_type() == at::kFloat && X.dim() == 2 && X.size(0) == NR &&
                    X.is_contiguous() && X.size(1) % 4 == 0 && (!guard || X.size(1) == H) &&
                    ls_wbar.has_value() && ls_wbar->is_cuda() &&
                    ls_wbar->scalar_type() == at::kFloat && ls_wbar->is_contiguous() &&
                    ls_wbar->numel() >= X.size(1) + 1,
                "vgrad_fold: ls_eps in (0, 1) needs dg_xe, X (n R, H) fp32 and ls_wbar (>= H + 1) fp32");
  }
  VGradRows va{(int)R, (int)n, (int)T_sel, (int)H, (int)V, lse.data_ptr<float>(),
               has_sel ? y_sel.data_ptr<int64_t>() : nullptr,
               has_sel ? dg_sel.data_ptr<float>() : nullptr,
               has_xe ? labels.data_ptr<int64_t>() + 1 : nullptr, has_xe ? labels.stride(0) : 0,
               has_xe ? dg_xe.data_ptr<float>() : nullptr, has_xe ? dg_xe.stride(0) : 0,
               guard ? fix.data_ptr<int>() : nullptr, ptr_or_null<float>(oh_a),
               ptr_or_null<int>(oh_ys), ptr_or_null<float>(oh_b), ptr_or_null<int>(oh_yx),
               have_x ? X.data_ptr<float>() : nullptr, zero_off ? 1 : 0, (float)ls_eps};
  hipStream_t st = cur_stream();
  launch_vgrad_onehot(va, reinterpret_cast<uint16_t*>(E.data_ptr()), ldl, alpha.data_ptr<float>(),
                      st);
  if (guard)
    launch_vgrad_fix(va, reinterpret_cast<const uint16_t*>(hd.data_ptr()),
                     reinterpret_cast<const uint16_t*>(wlog.data_ptr()), blog.data_ptr<float>(),
                     reinterpret_cast<uint16_t*>(E.data_ptr()), ldl, alpha.data_ptr<float>(),
                     fix_total.data_ptr<int>(), st);
  if (ls)
    launch_ls_shift(X.data_ptr<float>(), alpha.data_ptr<float>(), ls_wbar->data_ptr<float>(),
                    LsRowW{dg_xe.data_ptr<float>(), dg_xe.stride(0), (int)R, (float)ls_eps, nullptr},
                    0, NR, (int)X.size(1), st);
  std::vector<at::Tensor> out{alpha, fix};
  if (forward_x) out.insert(out.end(), {oh_a, oh_ys, oh_b, oh_yx});
  if (have_x || ls) out.push_back(X);
  return out;
}

// scaled rows for tests: hs (NR, ldhs) bf16 = alpha . hd, the augmented
// columns as the kernel writes them; dhd (NR, H) fp32 or empty, scaled in place
at::Tensor vgrad_rows(at::Tensor alpha, at::Tensor hd, int64_t ldhs, at::Tensor dhd) {
  check_cuda(alpha, "alpha");
  check_cuda(hd, "hd");
  TORCH_CHECK(hd.scalar_type() == at::kBFloat16 && hd.dim() == 2 &&
                  alpha.scalar_type() == at::kFloat && alpha.numel() == hd.size(0),
              "vgrad_rows: hd (NR, H) bf16, alpha (NR) fp32");
  const int64_t NR = hd.size(0), H = hd.size(1);
  const bool has_dhd = dhd.defined() && dhd.numel() > 0;
  if (has_dhd) {
    check_cuda(dhd, "dhd");
    TORCH_CHECK(dhd.scalar_type() == at::kFloat && dhd.dim() == 2 && dhd.size(0) == NR &&
                    dhd.size(1) == H, "vgrad_rows: dhd (NR, H) fp32");
  }
  TORCH_CHECK(NR > 0 && ldhs >= H, "vgrad_rows: ldhs >= H");
  at::Tensor hs = at::empty({NR, ldhs}, hd.options());
  launch_vgrad_rows(alpha.data_ptr<float>(), NR, (int)H,
                    reinterpret_cast<const uint16_t*>(hd.data_ptr()),
                    has_dhd ? dhd.data_ptr<float>() : nullptr,
                    reinterpret_cast<uint16_t*>(hs.data_ptr()), cur_stream(), (int)ldhs);
  return hs;
}

// bias-gradient column sums for tests: E (NR, ldl) bf16, alpha (NR) -> db (V) fp32
// ls_mode (label smoothing's kernels, kernels/label_smooth.hip):
//   1  column mean: E = the bf16 logit weights (V, H), alpha = the bias (V) ->
//      (H + 8) fp32: the mean row, at [H] the mean bias (what the forward keeps)
//   2  rank-1 sums: E = hd (n R, H) bf16, ls_dg = dg_xe (R, >= n) fp32 (its own
//      row stride) -> (H + 8) fp32: (ls_eps / V) sum_r dg_r [hd_r | 1]; with
//      ls_dw (V, H) / ls_db (V) fp32 also added onto them in place
//   3  smoothed log-prob: E = hd (n R, H) bf16, alpha = lse (n R), ls_dw = the
//      mode-1 vector, ls_dg = the target log-probs (R, n), blended in place:
//      (1 - ls_eps) g + ls_eps (hd . wbar + bbar - lse); returns ls_dg
at::Tensor vgrad_colsum(at::Tensor E, at::Tensor alpha, int64_t V, int64_t ls_mode, double ls_eps,
                        c10::optional<at::Tensor> ls_dg, c10::optional<at::Tensor> ls_dw,
                        c10::optional<at::Tensor> ls_db) {
  check_cuda(E, "E");
  if (ls_mode != 0) {
    TORCH_CHECK(ls_mode >= 1 && ls_mode <= 3 && E.scalar_type() == at::kBFloat16 && E.dim() == 2 &&
                    E.is_contiguous() && E.size(0) > 0 && E.size(1) % 8 == 0 && E.size(1) <= 2048,
                "vgrad_colsum: ls_mode 1..3 over contiguous bf16 rows (n, H), H % 8 == 0, H <= 2048");
    const int64_t n = E.size(0), H = E.size(1);
    auto f32 = at::TensorOptions().dtype(at::kFloat).device(E.device());
    auto f32_cuda = [](const at::Tensor& t) {
      return t.defined() && t.is_cuda() && t.scalar_type() == at::kFloat;
    };
    const uint16_t* rows = reinterpret_cast<const uint16_t*>(E.data_ptr());
    hipStream_t st = cur_stream();
    if (ls_mode == 1) {
      TORCH_CHECK(f32_cuda(alpha) && alpha.is_contiguous() && alpha.numel() == n && V == n,
                  "vgrad_colsum: ls_mode 1 takes the bias (V) fp32");
      at::Tensor part = at::empty({ls_rowsum_blocks(n, LS_WBAR_ROWS), H + 8}, f32);
      at::Tensor out = at::zeros({H + 8}, f32);
      launch_ls_rowsum(rows, n, (int)H, LsRowW{nullptr, 0, 1, 0.f, alpha.data_ptr<float>()},
                       LS_WBAR_ROWS, (float)(1.0 / (double)V), part.data_ptr<float>(),
                       out.data_ptr<float>(), st);
      return out;
    }
    TORCH_CHECK(ls_eps > 0.0 && ls_eps < 1.0 && ls_dg.has_value() && f32_cuda(*ls_dg) &&
                    ls_dg->dim() == 2 && ls_dg->stride(1) == 1 && ls_dg->size(0) > 0 &&
                    n % ls_dg->size(0) == 0 && ls_dg->size(1) >= n / ls_dg->size(0) &&
                    ls_dg->stride(0) >= ls_dg->size(1),
                "vgrad_colsum: ls_mode 2 / 3 take ls_eps in (0, 1) and ls_dg (R, >= n) fp32");
    const int64_t R = ls_dg->size(0);
    if (ls_mode == 2) {
      TORCH_CHECK(V > 0, "vgrad_colsum: V");
      at::Tensor part = at::empty({ls_rowsum_blocks(n, LS_GSUM_ROWS), H + 8}, f32);
      at::Tensor out = at::zeros({H + 8}, f32);
      launch_ls_rowsum(rows, n, (int)H,
                       LsRowW{ls_dg->data_ptr<float>(), ls_dg->stride(0), (int)R, (float)ls_eps,
                              nullptr},
                       LS_GSUM_ROWS, (float)(1.0 / (double)V), part.data_ptr<float>(),
                       out.data_ptr<float>(), st);
      if (ls_dw.has_value() && ls_dw->defined() && ls_dw->numel() > 0) {
        TORCH_CHECK(f32_cuda(*ls_dw) && ls_dw->is_contiguous() && ls_dw->dim() == 2 &&
                        ls_dw->size(0) == V && ls_dw->size(1) == H && ls_db.has_value() &&
                        f32_cuda(*ls_db) && ls_db->is_contiguous() && ls_db->numel() == V,
                    "vgrad_colsum: ls_dw (V, H) / ls_db (V) fp32");
        launch_ls_add(ls_dw->data_ptr<float>(), ls_db->data_ptr<float>(), out.data_ptr<float>(),
                      (int)V, (int)H, st);
      }
      return out;
    }
    TORCH_CHECK(f32_cuda(alpha) && alpha.is_contiguous() && alpha.numel() == n &&
                    ls_dw.has_value() && f32_cuda(*ls_dw) && ls_dw->is_contiguous() &&
                    ls_dw->numel() >= H + 1,
                "vgrad_colsum: ls_mode 3 takes lse (n R) and the mean row (>= H + 1) fp32");
    launch_ls_blend(rows, ls_dw->data_ptr<float>(), alpha.data_ptr<float>(), n, (int)R, (int)H,
                    (float)ls_eps, ls_dg->data_ptr<float>(), ls_dg->stride(0), st);
    return *ls_dg;
  }
  check_cuda(alpha, "alpha");
  TORCH_CHECK(E.scalar_type() == at::kBFloat16 && E.dim() == 2 &&
                  alpha.scalar_type() == at::kFloat && alpha.numel() == E.size(0) &&
                  E.size(0) > 0 && V > 0 && V <= E.size(1),
              "vgrad_colsum: E (NR, ldl >= V) bf16, alpha (NR) fp32");
  const int64_t NR = E.size(0), ldl = E.size(1);
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(E.device());
  at::Tensor part = at::empty({vgrad_colsum_blocks(NR), V}, f32), db = at::empty({V}, f32);
  launch_vgrad_colsum(reinterpret_cast<const uint16_t*>(E.data_ptr()), ldl, (int)V, NR,
                      alpha.data_ptr<float>(), part.data_ptr<float>(), db.data_ptr<float>(),
                      cur_stream());
  return db;
}

// video-gate gradient for tests: dG (n, R, >= G4) bf16 (rows ld apart, steps
// R ld apart) -> (R / vdiv, G4) fp32 sums over the steps and each video's rows
at::Tensor video_gate_grad(at::Tensor dG, int64_t vdiv, int64_t G4) {
  TORCH_CHECK(dG.is_cuda() && dG.scalar_type() == at::kBFloat16 && dG.dim() == 3 &&
                  dG.numel() > 0 && dG.stride(2) == 1 && dG.size(2) >= G4 &&
                  dG.stride(1) >= dG.size(2) && dG.stride(0) == dG.size(1) * dG.stride(1) &&
                  reinterpret_cast<uintptr_t>(dG.data_ptr()) % 16 == 0,
              "video_gate_grad: dG (n, R, >= G4) bf16, unit column stride, 16-byte rows");
  const int64_t n = dG.size(0), R = dG.size(1);
  TORCH_CHECK(vdiv > 0 && R % vdiv == 0, "video_gate_grad: R a multiple of vdiv");
  at::Tensor out = at::empty({R / vdiv, G4}, dG.options().dtype(at::kFloat));
  launch_video_gate_grad(reinterpret_cast<const uint16_t*>(dG.data_ptr()), dG.stride(1), (int)n,
                         (int)R, (int)vdiv, (int)G4, out.data_ptr<float>(), cur_stream());
  return out;
}

}  // namespace cst
