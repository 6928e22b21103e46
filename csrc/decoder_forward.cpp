// decoder_forward (overview: engine.cpp).  `Rollout` checks the arguments
// (check_args), allocates the buffers (alloc) and runs one of the two loops:
// the XE all-rows chain (run_xe_rows) or the general step loop (run_steps).
#include "engine_internal.h"

namespace cst {
namespace {

struct Rollout {
  // decoder_forward's arguments, in its order (the aggregate's initialisers)
  const at::Tensor &wx, &emb, &ptab, &whh, &wlog, &blog, &vgate;
  const int64_t vgate_div;
  const at::Tensor &labels, &bos;
  const int64_t R, T;
  const std::vector<int64_t>& modes;
  const double ss_prob, drop_p, temperature;
  const at::Tensor& rng;
  const bool save, want_xe, use_counts, use_unfinished;
  const std::vector<at::Tensor>& att;
  const int64_t cell;
  const std::vector<at::Tensor>&state0, &up;
  const bool store_exp, xe_rows;
  const c10::optional<at::Tensor>& lab_idx;
  // label smoothing (kernels/label_smooth.hip): g_xe leaves as the smoothed
  // target log-prob, ls_wbar receives the mean logit row / bias (backward)
  const double ls_eps;
  const c10::optional<at::Tensor>& ls_wbar;
  // ---- sizes and operands (check_args) --------------------------------------
  bool has_att = false, have_labels = false, have_idx = false;
  int64_t H4 = 0, H = 0, E = 0, V = 0, L = 0, n_steps = 0, NL = 1;
  const uint16_t* PTAB = nullptr;
  AttOperands ao;
  UpperLayers upl;
  InitState s0;
  // ---- buffers and launch operands (alloc) ------------------------------------
  hipStream_t st = nullptr;
  at::TensorOptions f32, bf, i64;
  at::Tensor seq, g_sel, g_xe, lse, part, counts, unfinished;
  StepInit sinit{};
  int64_t ldl = 0;  // saved rows padded to 128 bytes (whole cache lines per row)
  // Per-layer buffers: h_t / c_t / gates_t saved per step in training (else
  // ping-pong), hd_t = dropout(h_t) (the next layer's input; the top layer's
  // is the vocab input)
  at::Tensor logits16;
  std::vector<at::Tensor> Hs, Cs, Gs, HDs;
  std::vector<std::array<at::Tensor, 2>> hpp, cpp;
  const uint32_t* RNG = nullptr;
  float inv_temp = 1.f;
  const uint16_t *W = nullptr, *WHH = nullptr;
  const int64_t* LAB = nullptr;
  TokRows LABR;  // the label rows as every kernel reads them (by index where given)
  at::Tensor h0, c0;
  bool att_mfma = false, pre16 = false;
  at::Tensor pre, xin;
  at::Tensor vg_rows, q_all, alpha_all, q_tmp;
  const float* VG = nullptr;
  int VDIV = 1;
  at::Tensor gv16, vg16, att_ep, att_cnt, u_all;

  int key(int64_t l, int64_t t) const { return drop_key(NL, l, t); }
  at::Tensor h_tensor(int64_t l, int64_t t) const { return save ? Hs[l][t] : hpp[l][t & 1]; }
  uint16_t* h_buf(int64_t l, int64_t t) const {
    return reinterpret_cast<uint16_t*>(h_tensor(l, t).data_ptr());
  }
  float* c_buf(int64_t l, int64_t t) const {
    return save ? Cs[l][t].data_ptr<float>() : cpp[l][t & 1].data_ptr<float>();
  }
  uint16_t* hd_buf(int64_t l, int64_t t) const {
    if (!HDs[l].defined()) return nullptr;
    return reinterpret_cast<uint16_t*>((save ? HDs[l][t] : HDs[l]).data_ptr());
  }
  at::Tensor out_tensor(int64_t l, int64_t t) const {  // layer l's output fed upward
    return HDs[l].defined() ? (save ? HDs[l][t] : HDs[l]) : h_tensor(l, t);
  }
  uint16_t* gates_buf(int64_t l, int64_t t) const {
    return save ? reinterpret_cast<uint16_t*>(Gs[l][t].data_ptr()) : nullptr;
  }

  void check_args() {
    check_cuda(wx, "wx");
    TORCH_CHECK(cell >= 0 && cell <= 2, "cell: 0 lstm, 1 gru, 2 rnn (tanh)");  // CellType (common.h)
    check_cuda(emb, "emb");
    check_cuda(wlog, "wlog");
    check_cuda(blog, "blog");
    has_att = !att.empty();  // (AttOperands, engine_internal.h)
    if (!has_att) check_cuda(vgate, "vgate");
    TORCH_CHECK(wx.scalar_type() == at::kBFloat16 && emb.scalar_type() == at::kBFloat16 &&
                    wlog.scalar_type() == at::kBFloat16,
                "decoder weights must be bf16");
    if (!has_att) TORCH_CHECK(vgate.scalar_type() == at::kFloat, "vgate must be fp32");
    check_cuda(ptab, "ptab");
    check_cuda(whh, "whh");
    TORCH_CHECK(ptab.scalar_type() == at::kHalf && ptab.size(0) == emb.size(0) &&
                    ptab.size(1) == wx.size(0), "ptab must be fp16 (V, 4H)");
    PTAB = reinterpret_cast<const uint16_t*>(ptab.data_ptr());
    TORCH_CHECK(whh.scalar_type() == at::kBFloat16 && whh.size(0) >= wx.size(0) &&
                    whh.size(1) * 4 == wx.size(0), "whh must be bf16 (4H[+A], H)");
    H4 = wx.size(0), H = H4 / 4, E = emb.size(1), V = wlog.size(0);
    TORCH_CHECK(wx.size(1) == E + H, "wx must be (4H, E+H)");
    TORCH_CHECK(E % 64 == 0 && H % 64 == 0, "E and H must be multiples of 64");
    TORCH_CHECK(wlog.size(1) == H && blog.numel() == V, "logit weight shape");
    if (!has_att)
      TORCH_CHECK(vgate.size(1) == H4 && vgate.size(0) * vgate_div >= R, "vgate shape");
    ao = AttOperands::parse(att, Site::Forward, H, R, vgate_div, 0);
    if (has_att)
      TORCH_CHECK(whh.size(0) == H4 + ao.A, "with attention whh must be [W_hh; W_q] (4H + A, H)");
    TORCH_CHECK(T >= 2 && (int64_t)modes.size() >= T - 1, "modes must cover T-1 steps");
    have_labels = labels.defined() && labels.numel() > 0;
    have_idx = have_labels && lab_idx.has_value() && lab_idx->defined() && lab_idx->numel() > 0;
    if (have_labels) {
      check_cuda(labels, "labels");
      // lab_idx: labels is the resident (captions, L) label table and row r of
      // this call is its row lab_idx[r] -- every reader below takes the index
      // (TokRows), no gathered copy is made
      TORCH_CHECK(labels.scalar_type() == at::kLong && labels.dim() == 2 && labels.is_contiguous() &&
                      (have_idx || labels.size(0) == R), "labels (R, L) int64");
      if (have_idx) {
        check_cuda(*lab_idx, "lab_idx");
        TORCH_CHECK(lab_idx->scalar_type() == at::kLong && lab_idx->is_contiguous() &&
                        lab_idx->numel() == R && labels.size(0) >= 1,
                    "lab_idx: (R) int64 rows of the label table");
        // (teacher forcing keeps the gathered copy: its loss reads it anyway)
        TORCH_CHECK(!xe_rows && !want_xe, "want_xe / xe_rows read a gathered (R, L) label copy");
      }
      L = labels.size(1);
      TORCH_CHECK(L >= T + (want_xe ? 1 : 0), "labels too short for T steps");
    } else {
      TORCH_CHECK(!want_xe, "want_xe needs labels");
      check_cuda(bos, "bos");
    }
    n_steps = want_xe ? T : T - 1;  // LSTM steps actually needed
    // Stacked layers (num_layers > 1): layer 0 is the fused pipeline below;
    // layer l >= 1 runs after it in every step: x_l = dropout(h_{l-1}) W_ih_l^T
    // (hipBLASLt, fp32) enters the step kernel as its per-row input term, the
    // kernel adds h_l W_hh_l^T and applies the cell.  (Dropout keys: drop_key.)
    upl = UpperLayers::parse(up, Site::Forward, has_att, !state0.empty(), H, 0);
    NL = upl.NL;
    // initial state (model_type 'standard': the state after the video step;
    // otherwise zero): state0 = {h0 bf16 (R, H), c0 fp32 (R, H)}
    s0 = InitState::parse(state0, Site::Forward, has_att, R, H);
    TORCH_CHECK(ls_eps >= 0.0 && ls_eps < 1.0, "ls_eps must be in [0, 1)");
    if (ls_eps > 0.0)
      TORCH_CHECK(want_xe && save && store_exp && H % 8 == 0 && H <= 2048 && ls_wbar.has_value() &&
                      ls_wbar->defined() && ls_wbar->is_cuda() &&
                      ls_wbar->scalar_type() == at::kFloat && ls_wbar->is_contiguous() &&
                      ls_wbar->numel() >= H + 1,
                  "label smoothing: a saved exp-store forward with XE targets, H <= 2048 and an "
                  "fp32 ls_wbar (>= H + 1)");
  }

  // label smoothing, after the last combine: the column mean of the bf16 logit
  // weights the vocabulary tiles read (and the mean bias) into ls_wbar, then
  // g_xe[r, t] = (1 - eps) lp[y] + eps (Hd . wbar + bbar - lse) from the saved
  // vocab input: no dense pass
  void smooth_xe() {
    if (!(ls_eps > 0.0)) return;
    at::Tensor lpart = at::empty({ls_rowsum_blocks(V, LS_WBAR_ROWS), H + 8}, f32);
    launch_ls_rowsum(W, V, (int)H, LsRowW{nullptr, 0, 1, 0.f, blog.data_ptr<float>()},
                     LS_WBAR_ROWS, (float)(1.0 / (double)V), lpart.data_ptr<float>(),
                     ls_wbar->data_ptr<float>(), st);
    launch_ls_blend(reinterpret_cast<const uint16_t*>(HDs[NL - 1].data_ptr()),
                    ls_wbar->data_ptr<float>(), lse.data_ptr<float>(), n_steps * R, (int)R, (int)H,
                    (float)ls_eps, g_xe.data_ptr<float>(), T, st);
  }

  void alloc() {
    auto dev = wx.device();
    f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    bf = at::TensorOptions().dtype(at::kBFloat16).device(dev);
    i64 = at::TensorOptions().dtype(at::kLong).device(dev);
    st = cur_stream();

    // (every entry is written by the combine of its step: no fill kernels)
    seq = at::empty({R, T - 1}, i64);
    g_sel = at::empty({R, T - 1}, f32);
    g_xe = want_xe ? at::empty({R, T}, f32) : at::Tensor();
    lse = at::empty({n_steps, R}, f32);
    part = at::empty({(int64_t)vocab_part_slots((int)V) * R * vocab_partial_bytes() / 4}, f32);
    // the end-of-sequence flags of every step and the row masks: no fill
    // launches -- the decode's first launch (lstm_step_fwd, step 0) zeroes the
    // flag words and sets the masks before any combine reads them (StepInit)
    const int64_t n_cnt = (T + 1) * combine_count_ints_per_step();
    counts = at::empty({n_cnt}, at::TensorOptions().dtype(at::kInt).device(dev));
    unfinished = use_unfinished ? at::empty({R}, at::TensorOptions().dtype(at::kByte).device(dev))
                                : at::Tensor();
    if (use_counts) {
      sinit.flags = counts.data_ptr<int>();
      sinit.n_flags = (int)(T + 1) * combine_count_slots();
      sinit.stride = combine_count_ints_per_step() / combine_count_slots();
    }
    if (use_unfinished) {
      sinit.ones = unfinished.data_ptr<uint8_t>();
      sinit.n_ones = (int)R;
    }
    ldl = (V + 63) / 64 * 64;
    Hs.resize(NL), Cs.resize(NL), Gs.resize(NL), HDs.resize(NL), hpp.resize(NL), cpp.resize(NL);
    // saved vocab rows: fp16 logits, or (store_exp) bf16 E = exp(x - lse of the
    // previous step) for the dS-free backward (kernels/vocab_grad.hip)
    if (save)
      logits16 = at::empty({n_steps, R, ldl}, at::TensorOptions()
                                                  .dtype(store_exp ? at::kBFloat16 : at::kHalf)
                                                  .device(dev));
    for (int64_t l = 0; l < NL; ++l) {
      if (save) {
        Hs[l] = at::empty({n_steps, R, H}, bf);
        Cs[l] = at::empty({n_steps, R, H}, f32);
        Gs[l] = at::empty({n_steps, R, H4}, bf);
        HDs[l] = at::empty({n_steps, R, H}, bf);
      } else {
        hpp[l] = {at::empty({R, H}, bf), at::empty({R, H}, bf)};
        cpp[l] = {at::empty({R, H}, f32), at::empty({R, H}, f32)};
        if (drop_p > 0) HDs[l] = at::empty({R, H}, bf);
      }
    }
    RNG = rng_ptr(rng);
    inv_temp = (float)(1.0 / temperature);
    W = reinterpret_cast<const uint16_t*>(wlog.data_ptr());
    WHH = reinterpret_cast<const uint16_t*>(whh.data_ptr());
    LAB = have_labels ? labels.data_ptr<int64_t>() : nullptr;
    LABR = TokRows(LAB, have_idx ? lab_idx->data_ptr<int64_t>() : nullptr,
                   have_idx ? labels.size(0) : 0);
    h0 = s0.h0, c0 = s0.c0;
    if (!s0.on) {
      h0 = zeros_view(dev, R * H, at::kBFloat16).view({R, H});
      c0 = zeros_view(dev, R * H, at::kFloat).view({R, H});
    }
    // pre-activations of the next step (the decode launch's recurrent tiles ->
    // the combine's cell epilogue) in fp16: half the bytes of the combine's
    // largest operand; fp32 where the VALU attention adds its video term into
    // them in place (attention without the MFMA path)
    static const bool pre16_env = [] {
      const char* e = getenv("CSTCAP_PRE16");
      return e == nullptr || atoi(e) != 0;
    }();
    // CSTCAP_GREEDY_ATT_MFMA=1: a forward that saves nothing (the SCST greedy
    // baseline, one row per video) takes the MFMA attention too.  Opt-in: its
    // A / 64 workgroups per video (512 per greedy step at the att8 shape, each
    // computing 32-row tiles for one row) slow the concurrent sampled rollout
    // more than the VALU scorer + query GEMM they replace (att8 4.730 / 4.771
    // vs 4.607 / 4.602 ms, interleaved on one box, profiles/r6/s2/).
    static const bool fwd1_env = [] {
      const char* e = getenv("CSTCAP_GREEDY_ATT_MFMA");
      return e != nullptr && atoi(e) != 0;
    }();
    const int64_t Bv = ao.Bv, C = ao.C, A = ao.A;
    att_mfma = has_att &&
               (save || !fwd1_env
                    ? att_mfma_ok((int)vgate_div, (int)C, (int)A, (int)H, ao.per_frame)
                    : att_mfma_fwd_ok((int)vgate_div, (int)C, (int)A, (int)H, ao.per_frame));
    pre16 = pre16_env && !(has_att && !att_mfma);
    pre = n_steps > 1 ? at::empty({R, H4}, f32.dtype(pre16 ? at::kHalf : at::kFloat))
                      : at::Tensor();
    xin = NL > 1 ? at::empty({R, H4}, f32) : at::Tensor();
    // Attention of step t: query q_t = W_q h_{t-1} (hipBLASLt, fp32 out; q_0 = 0),
    // then the attention kernel writes the per-row video gate term vg_rows.
    if (has_att) {
      vg_rows = at::empty({R, H4}, f32);
      if (save) {
        q_all = at::empty({n_steps, R, A}, f32);  // q_0 = 0 is never read
        alpha_all = at::empty({n_steps, R, C}, f32);
      } else {
        q_tmp = at::empty({R, A}, f32);
      }
    }
    VG = has_att ? vg_rows.data_ptr<float>() : vgate.data_ptr<float>();
    VDIV = has_att ? 1 : (int)vgate_div;
    // MFMA attention path (kernels/att_mfma.h): from step 1 on, the attention of
    // step t+1 runs as extra workgroups of step t's decode launch (it needs only
    // h_t) and writes bf16 per-row video gates that the combine's cell epilogue
    // adds; no attention launch between the decode launch and the combine.
    // Step 0 (q = 0) and other shapes use the attention kernels of attention.hip.
    if (att_mfma) {
      // training: the scorer values tanh(P + q) of steps >= 1 (fp16), read by
      // the fused attention backward (lstm.hip att_bwd_fused_wg)
      if (save) u_all = at::empty({n_steps, R, C, A}, f32.dtype(at::kHalf));
      gv16 = at::zeros({Bv, H4, ao.CPAD}, bf);  // frame-minor, frames zero-padded
      gv16.narrow(2, 0, C).copy_(ao.gv.transpose(1, 2));
      vg16 = at::empty({R, H4}, bf);
      att_ep = at::empty({Bv, A / 64, 32, ao.CPAD}, f32);
      att_cnt = at::zeros({Bv}, at::TensorOptions().dtype(at::kInt).device(dev));
    }
  }

  // layer l >= 1 at step t (its zero initial state is h0 / c0's zeros)
  void upper_step(int64_t l, int64_t t) {
    const at::Tensor& wu = upl(l, 0);
    at::mm_out(xin, out_tensor(l - 1, t), wu.narrow(1, 0, H).t(), at::kFloat);
    launch_lstm_step_fwd(nullptr, 0, nullptr,
                         t > 0 ? h_buf(l, t - 1) : reinterpret_cast<uint16_t*>(h0.data_ptr()),
                         t > 0 ? c_buf(l, t - 1) : c0.data_ptr<float>(), xin.data_ptr<float>(), 1,
                         (int)R, (int)H, reinterpret_cast<const uint16_t*>(upl(l, 1).data_ptr()),
                         h_buf(l, t), c_buf(l, t), hd_buf(l, t), (int)H, (float)drop_p, RNG,
                         key(l, t), gates_buf(l, t), st, nullptr, (int)cell);
  }

  // the attention of step t through the kernels of attention.hip
  void run_att(int64_t t) {
    const float* qp = nullptr;
    if (t > 0) {
      at::Tensor qo = save ? q_all[t] : q_tmp;
      at::mm_out(qo, h_tensor(0, t - 1), ao.wq.t(), at::kFloat);
      qp = qo.data_ptr<float>();
    }
    launch_att_fwd(ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(), qp, nullptr,
                   ao.wa.data_ptr<float>(), ao.ba.data_ptr<float>(), (int)ao.Bv, (int)vgate_div,
                   (int)ao.C, (int)ao.A, (int)H4, vg_rows.data_ptr<float>(),
                   save ? alpha_all[t].data_ptr<float>() : nullptr, st, 0, ao.per_frame);
  }

  // XE all rows (xe_rows: a teacher-forced training forward).  Every input
  // token is a label, known before the vocabulary projection of the previous
  // step, so the cell needs no combine: ONE launch per step runs the
  // vocabulary tiles of step t (E = exp(x), offset 0 -- the backward's
  // VGradRows::zero_off -- and the per-tile partials) together with the WHOLE
  // LSTM step t+1 (lstm_gemm.h lstm_cell_block: recurrent GEMM + table row +
  // cell); ONE combine over all rows after the chain gives every step's LSE
  // and target log-prob: the per-step combine (~12 us with its cell epilogue)
  // leaves the chain.  (Per-step combines on a side stream contended with the
  // chain: XE 3.279 / 3.308 vs 3.213 / 3.258 ms per step, profiles/r6/s2/.)  seq = labels[:, 1:T], exactly as the
  // per-step combine picks them (a step after which every row emitted EOS only
  // forces tokens the labels already hold as 0).
  std::vector<at::Tensor> run_xe_rows() {
    TORCH_CHECK(save && store_exp && want_xe && have_labels && NL == 1 && !has_att &&
                    state0.empty() && n_steps == T && n_steps <= XE_MAX_STEPS,
                "xe_rows: a saved, exp-store teacher-forced forward of a one-layer decoder "
                "without attention / initial state, <= 64 steps");
    for (int64_t t = 0; t + 1 < T; ++t)
      TORCH_CHECK(modes[t] == SEL_GT_H, "xe_rows: teacher forcing at every step");
    const int n_vt = vocab_num_tiles((int)V);
    const int64_t pstep = (int64_t)n_vt * R * vocab_partial_bytes();  // partial bytes per step
    at::Tensor part_all = at::empty({n_steps * pstep / 4}, f32);
    at::Tensor tgt_all = labels.narrow(1, 1, n_steps).t().contiguous();  // (n_steps, R)
    at::Tensor gx = at::empty({n_steps, R}, f32);
    stamp(STAMP_FWD_BEGIN, st);
    // (no StepInit: this path passes null counts to its one combine and never
    // returns the buffer, so the flag words stay unwritten and unread)
    launch_lstm_step_fwd(LAB, L, PTAB, nullptr, nullptr, VG, VDIV, (int)R, (int)H, WHH,
                         h_buf(0, 0), c_buf(0, 0), hd_buf(0, 0), (int)H, (float)drop_p, RNG,
                         key(0, 0), gates_buf(0, 0), st, nullptr, (int)cell);
    stamp(STAMP_FWD_STEP0, st);
    for (int64_t t = 0; t < n_steps; ++t) {
      const bool next = t + 1 < n_steps;
      XeCell xc{};
      if (next)
        xc = XeCell{LAB + (t + 1), L, PTAB, c_buf(0, t), h_buf(0, t + 1), c_buf(0, t + 1),
                    hd_buf(0, t + 1), gates_buf(0, t + 1), (float)drop_p, key(0, t + 1),
                    (int)cell};
      char* pt = reinterpret_cast<char*>(part_all.data_ptr()) + t * pstep;
      launch_vocab_lstm_xe(hd_buf(0, t), (int)R, (int)H, W, blog.data_ptr<float>(), (int)V,
                           reinterpret_cast<uint16_t*>(logits16[t].data_ptr()), ldl, pt,
                           tgt_all.data_ptr<int64_t>() + t * R, RNG, h_buf(0, t), WHH, VG, VDIV,
                           next ? &xc : nullptr, st);
    }
    // every step's LSE and target log-probs: one combine over all rows (the
    // per-step partial blocks), after the chain
    launch_vocab_combine(part_all.data_ptr(), n_vt, (int)(n_steps * R), lse.data_ptr<float>(),
                         nullptr, 0, nullptr, 0, gx.data_ptr<float>(), 1, nullptr, 0, SEL_GT_H,
                         0.f, RNG, 0, nullptr, 0, nullptr, st, nullptr, (int)R);
    at::Tensor gxt = gx.t();  // (R, T)
    g_xe.copy_(gxt);
    g_sel.copy_(gxt.narrow(1, 0, T - 1));
    seq.copy_(labels.narrow(1, 1, T - 1));
    smooth_xe();
    stamp(STAMP_FWD_END, st);
    return {seq, g_sel, g_xe, lse, logits16, HDs[0], Gs[0], Cs[0], Hs[0]};
  }

  // the general step loop
  std::vector<at::Tensor> run_steps() {
    const int64_t Bv = ao.Bv, C = ao.C, A = ao.A;
    // step 0: fused cell step from (h_{-1}, c_{-1}) = (h0, c0)
    stamp(STAMP_FWD_BEGIN, st);
    if (has_att) run_att(0);
    // (zero initial state: null h / c, the kernel skips the recurrent GEMM)
    launch_lstm_step_fwd(have_labels ? LABR : TokRows(bos.data_ptr<int64_t>()), have_labels ? L : 1,
                         PTAB,
                         state0.empty() ? nullptr : reinterpret_cast<uint16_t*>(h0.data_ptr()),
                         state0.empty() ? nullptr : c0.data_ptr<float>(), VG, VDIV, (int)R, (int)H, WHH, h_buf(0, 0),
                         c_buf(0, 0), hd_buf(0, 0), (int)H, (float)drop_p, RNG, key(0, 0),
                         gates_buf(0, 0), st, nullptr, (int)cell, &sinit);
    for (int64_t l = 1; l < NL; ++l) upper_step(l, 0);
    // Steps t >= 0: ONE launch runs the vocab projection of step t together with
    // the recurrent GEMM of step t+1 (pre = h_t W_hh^T + vgate, layer 0), then
    // the combine picks token t+1 and applies step t+1's cell epilogue (pre +
    // P[token]); the upper layers of step t+1 follow.
    bool conv_join = false;
    for (int64_t t = 0; t < n_steps; ++t) {
      const bool next = t + 1 < n_steps;
      uint16_t* hd = hd_buf(NL - 1, t);
      const uint16_t* vin = hd ? hd : h_buf(NL - 1, t);
      const bool choose = t < T - 1;
      const int mode = choose ? (int)modes[t] : SEL_GT_H;
      const int do_sample = choose && (mode == SEL_SAMPLE_H || mode == SEL_SS_H);
      const bool exp_t = save && store_exp && t > 0;  // step 0: fp16, converted below
      const int vflags = do_sample | ((choose && mode == SEL_GREEDY_H) ? 2 : 0) | (exp_t ? 16 : 0);
      const TokRows tgt = (have_labels && t + 1 < L) ? LABR.col(t + 1) : TokRows();
      // the launch looks the target token's logit up only where this step's
      // combine reads it (the combine keeps the token itself)
      const TokRows tgt_x = vocab_step_reads_target(want_xe, choose, mode) ? tgt : TokRows();
      // attention: the same launch also projects q_{t+1} = h_t W_q^T (extra
      // W_q tiles of the recurrent GEMM, no vgate add); the attention kernel then
      // adds each row's video term into pre before the combine's cell epilogue
      at::Tensor q_next;
      if (has_att && next) q_next = save ? q_all[t + 1] : q_tmp;
      AttMfmaArgs am{};
      if (att_mfma && next)
        am = AttMfmaArgs{h_buf(0, t), WHH + H4 * H, ao.pre.data_ptr<float>(), ao.wa.data_ptr<float>(),
                         ao.ba.data_ptr<float>(), reinterpret_cast<const uint16_t*>(gv16.data_ptr()),
                         (int)H, (int)A, (int)C, ao.CPAD, (int)H4, (int)vgate_div, (int)Bv,
                         reinterpret_cast<uint16_t*>(vg16.data_ptr()),
                         save ? alpha_all[t + 1].data_ptr<float>() : nullptr,
                         save ? q_next.data_ptr<float>() : nullptr, att_ep.data_ptr<float>(),
                         att_cnt.data_ptr<int>(),
                         save ? reinterpret_cast<uint16_t*>(u_all[t + 1].data_ptr()) : nullptr};
      if (att_mfma && next) am.whole = att_mfma_whole_default((int)C, (int)H);
      const bool q_tiles = has_att && !att_mfma;  // W_q tiles in the recurrent GEMM
      const int n_vt = launch_vocab_lstm_fwd(
          vin, (int)H, (int)R, (int)H, W, blog.data_ptr<float>(), (int)V,
          save ? reinterpret_cast<uint16_t*>(logits16[t].data_ptr()) : nullptr, ldl, part.data_ptr(),
          tgt_x, L, vflags, inv_temp, RNG, (int)t, h_buf(0, t), WHH, has_att ? nullptr : VG, VDIV,
          next ? reinterpret_cast<float*>(pre.data_ptr()) : nullptr, st, q_tiles ? (int)A : 0,
          q_tiles && next ? q_next.data_ptr<float>() : nullptr,
          exp_t ? lse[t - 1].data_ptr<float>() : nullptr, att_mfma && next ? &am : nullptr,
          pre16 ? 1 : 0);
      if (q_tiles && next)
        launch_att_fwd(ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(), q_next.data_ptr<float>(),
                       nullptr, ao.wa.data_ptr<float>(), ao.ba.data_ptr<float>(), (int)Bv,
                       (int)vgate_div, (int)C, (int)A, (int)H4, pre.data_ptr<float>(),
                       save ? alpha_all[t + 1].data_ptr<float>() : nullptr, st, /*accumulate=*/1,
                       ao.per_frame);
      CellLaunch cl{};
      if (next) {
        TORCH_CHECK(choose, "internal: a next step needs a chosen token");
        cl = CellLaunch{pre.data_ptr(), PTAB, c_buf(0, t), c_buf(0, t + 1),
                        h_buf(0, t + 1), hd_buf(0, t + 1), (int)H, gates_buf(0, t + 1), (int)H,
                        (float)drop_p, key(0, t + 1), (int)cell,
                        att_mfma ? reinterpret_cast<const uint16_t*>(vg16.data_ptr()) : nullptr,
                        pre16 ? 1 : 0};
      }
      launch_vocab_combine(part.data_ptr(), n_vt, (int)R, lse[t].data_ptr<float>(),
                             choose ? seq.data_ptr<int64_t>() + t : nullptr, T - 1,
                             choose ? g_sel.data_ptr<float>() + t : nullptr, T - 1,
                             want_xe ? g_xe.data_ptr<float>() + t : nullptr, T, tgt, L, mode,
                             (float)ss_prob, RNG, (int)t,
                             use_counts ? counts.data_ptr<int>() : nullptr, (int)(t + 1),
                             use_unfinished ? unfinished.data_ptr<uint8_t>() : nullptr, st,
                             next ? &cl : nullptr);
      if (save && store_exp && t == 0) {
        // only the backward reads step 0's exp store: the conversion runs on a
        // side stream, off the decode chain, joined after the loop
        DeviceAux& aux = device_aux((int)wx.device().index());
        const hipStream_t cs = aux.side[1].stream();
        fork(aux.fwd_ev[0], st, cs);
        launch_vocab_exp_convert(reinterpret_cast<uint16_t*>(logits16[0].data_ptr()), ldl, (int)V,
                                 (int)R, lse[0].data_ptr<float>(), cs);
        (void)hipEventRecord(aux.fwd_ev[1], cs);
        conv_join = true;
      }
      if (next)
        for (int64_t l = 1; l < NL; ++l) upper_step(l, t + 1);
      if (t == 0) stamp(STAMP_FWD_STEP0, st);
    }
    if (conv_join)
      (void)hipStreamWaitEvent(st, device_aux((int)wx.device().index()).fwd_ev[1], 0);
    smooth_xe();
    stamp(STAMP_FWD_END, st);
    // saved: {logits16, hd of the top layer (vocab input), layer 0's gates, c, h}
    // (+ {alpha_all, q_all, u_all}) (+ {h, c, gates of layer l, hd of layer l-1} per l >= 1)
    std::vector<at::Tensor> out = {seq, g_sel, want_xe ? g_xe : at::Tensor(), lse};
    if (save) {
      out.push_back(logits16);
      out.push_back(HDs[NL - 1]);
      out.push_back(Gs[0]);
      out.push_back(Cs[0]);
      out.push_back(Hs[0]);
      if (has_att) {
        out.push_back(alpha_all);
        out.push_back(q_all);
        out.push_back(u_all.defined() ? u_all : at::empty({0}, f32.dtype(at::kHalf)));
      }
      for (int64_t l = 1; l < NL; ++l) {
        out.push_back(Hs[l]);
        out.push_back(Cs[l]);
        out.push_back(Gs[l]);
        out.push_back(HDs[l - 1]);
      }
    }
    return out;
  }
};

}  // namespace

// modes[t] = token-selection mode for token t+1 (see SelModeHost)
std::vector<at::Tensor> decoder_forward(at::Tensor wx, at::Tensor emb, at::Tensor ptab,
                                        at::Tensor whh, at::Tensor wlog,
                                        at::Tensor blog, at::Tensor vgate, int64_t vgate_div,
                                        at::Tensor labels, at::Tensor bos, int64_t R, int64_t T,
                                        std::vector<int64_t> modes, double ss_prob,
                                        double drop_p, double temperature, at::Tensor rng,
                                        bool save, bool want_xe, bool use_counts,
                                        bool use_unfinished, std::vector<at::Tensor> att,
                                        int64_t cell, std::vector<at::Tensor> state0,
                                        std::vector<at::Tensor> up, bool store_exp,
                                        bool xe_rows, c10::optional<at::Tensor> lab_idx,
                                        double ls_eps, c10::optional<at::Tensor> ls_wbar) {
  Rollout r{wx, emb, ptab, whh, wlog, blog, vgate, vgate_div, labels, bos, R, T, modes, ss_prob,
            drop_p, temperature, rng, save, want_xe, use_counts, use_unfinished, att, cell, state0,
            up, store_exp, xe_rows, lab_idx, ls_eps, ls_wbar};
  r.check_args();
  r.alloc();
  return xe_rows ? r.run_xe_rows() : r.run_steps();
}

}  // namespace cst
