// decoder_backward (overview: engine.cpp).  `Backward` validates the arguments, makes
// every mode decision once, owns the tensors that several streams touch and has one method
// per phase; decoder_backward, at the end, is the schedule: streams, forks and joins.
#include "engine_internal.h"

namespace cst {
namespace {

// The environment knobs of the backward, read once.
struct BwdKnobs {
  // dW_logit after the persistent loop starts once the main stream's token
  // sums are enqueued (1; 0: right after the loop, 2: after the d_emb GEMM):
  // its long-running GEMM workgroups no longer hold every CU while the
  // latency-bound post-loop chain waits for slots.  Interleaved on one box:
  // 3.210-3.218 (1) / 3.232-3.237 (2) vs 3.292-3.295 ms (0) per headline
  // step, XE 3.32-3.34 vs 3.39-3.40 (profiles/r6/README_r6.md)
  int dw_late;  // CSTCAP_DW_LATE
  // the dW batch with the measured hipBLASLt choice (gemm_bf16_tuned_batched)
  bool dw_tuned;  // CSTCAP_DW_TUNED
  // CSTCAP_DW_AUG unset (-1): the augmented rows with the persistent loop only
  // (dW after the loop); with the per-step loop the dW GEMM runs UNDER the
  // loop, where its 16 extra columns contend with the latency-bound step
  // kernels and the column sums' 210 long workgroups leave them CU slots
  int dw_aug;
  // CSTCAP_DW_WGRAD=1: dW_logit AND the bias column sums in one hand-written
  // split-K MFMA kernel instead (kernels/wgrad.hip: M = V with a ragged last
  // tile, the sums from the E' tiles already in LDS): one pass over the exp
  // store too, but 737 us at the headline shape against 392 + 209 us for the
  // vendor batch + the column sums (profiles/r6/README_r6.md)
  bool dw_wgrad;
  // (the augmented rows padded to H + 64 columns: hipBLASLt's pick for the
  // split-K batch runs 443 us at N = 576 against 479 at N = 528 and 537 at
  // N = 512, isolated timings, profiles/r6/README_r6.md; CSTCAP_DW_PAD)
  int64_t dw_pad;
  // d_emb = S W_ie (M = V, N = E, K = 4H): the measured hipBLASLt choice
  // (host/blaslt_tuned.cpp) -- PyTorch's heuristic pick ran it at 0.17 PF/s
  // (130 us, profiles/r5/final5/steps_final5.txt).  CSTCAP_DEMB_TUNED=0: at::mm.
  bool demb_tuned;
};
const BwdKnobs& knobs() {
  static const BwdKnobs k = [] {
    BwdKnobs k{};
    const char* e = getenv("CSTCAP_DW_LATE");
    k.dw_late = e != nullptr ? atoi(e) : 1;
    e = getenv("CSTCAP_DW_TUNED");
    k.dw_tuned = e != nullptr && e[0] == '1';
    e = getenv("CSTCAP_DW_AUG");
    k.dw_aug = e == nullptr || e[0] == 0 ? -1 : atoi(e);
    e = getenv("CSTCAP_DW_WGRAD");
    k.dw_wgrad = e != nullptr && atoi(e) != 0;
    e = getenv("CSTCAP_DW_PAD");
    const int64_t v = e != nullptr ? atoll(e) : 64;
    k.dw_pad = v >= 16 && v <= 512 && v % 8 == 0 ? v : 64;
    e = getenv("CSTCAP_DEMB_TUNED");
    k.demb_tuned = e == nullptr || atoi(e) != 0;
    return k;
  }();
  return k;
}

// Where the vocab head's weight gradients (side stream; they need no loop result) start.
enum DwStart {
  DW_UNDER_LOOP,    // per-step loop: right after the X chunks, under the loop
  DW_AFTER_LOOP,    // persistent loop, data parallelism / grad events: right after it
  DW_AFTER_TOKSUM,  // persistent loop (default): after the main stream's token sums
  DW_AFTER_DEMB,    // persistent loop, CSTCAP_DW_LATE=2: after the d_emb GEMM
  DW_NOT_STARTED    // (persistent loop and CSTCAP_DW_LATE outside 0..2)
};

// decoder_backward's arguments, in its order
struct BwdArgs {
  const at::Tensor &wx, &wlog, &emb, &lse, &logits16, &hdrop_all, &gates_all, &c_all, &h_all, &seq,
      &labels, &toks, &dg_sel, &dg_xe;
  const double drop_p;
  const at::Tensor &rng, &out_wlog, &out_blog;
  const int64_t comm_stream;
  const std::vector<at::Tensor>& att;
  const at::Tensor &out_emb, &ds_bias;
  const int64_t cell;
  const std::vector<at::Tensor>&state0, &up;
  const at::Tensor &blog, &fix_total;
  const int64_t vgate_div;
  const at::Tensor& xw;
  const std::vector<at::Tensor>& vg_bwd;
  const int64_t vg_nf;
  const double vg_p;
  const int64_t x_wait;
  const bool exp_zero_off;
  const std::vector<at::Tensor>& dw_slots;
  const c10::optional<at::Tensor>& vg_idx;
  const int64_t vg_C;
  // label smoothing (kernels/label_smooth.hip): dg_xe is the gradient of the
  // smoothed target log-prob; ls_wbar = the forward's (H + 1) column mean of
  // the logit weights and mean bias.  0: none of it runs
  const double ls_eps;
  const c10::optional<at::Tensor>& ls_wbar;
};

bool nonempty(const at::Tensor& t) { return t.defined() && t.numel() > 0; }

struct Backward : BwdArgs {
  // ---- sizes and operands -------------------------------------------------
  const int64_t n_steps, R, ldl, H4, H, E, V, T_sel, NR;
  const hipStream_t st;  // the main stream (current at the call)
  const at::Device dev;
  const at::TensorOptions f32, i32;
  const bool has_sel, has_xe;
  const uint32_t* const RNG;
  const AttOperands ao;
  const bool has_att;
  const int64_t Bv, C, A, vdiv;
  const int per_frame;
  const int64_t NWA;  // scorer-weight rows
  const int64_t KD;   // dG rows: 4H gate gradients (+ A columns of dq with attention)
  const UpperLayers upw;
  const int64_t NL;
  const InitState s0;
  const bool has_s0;
  DeviceAux& aux;
  const c10::hip::HIPStream side, side2;

  // ---- mode decisions (all made here, none changes afterwards) -------------
  // X = E W computed right after the rollout (engine.launch_x, vocab_x): no
  // GEMM here, the loop waits only for the row weights
  const bool have_x;
  // 1-2. vocab head on the side stream.  Exp store (training): alpha and the
  // one-hot terms folded into E, X = E' W (dHd = alpha X, scaled by the
  // loop), the alpha-scaled Hd rows for dW; kernels/vocab_grad.hip.  Dense
  // dS given by the caller (full log-prob API, fp16-logits buffer rewritten
  // as bf16 dS): dHd = dS W.
  const bool ds_ready;
  // The whole reverse recurrence as ONE persistent launch (lstm_loop.hip):
  // one-layer decoders without attention / initial state whose shape fits
  // (headline: 256 workgroups, one per CU, all resident: the side stream's
  // vocab-head weight gradients start after it).  CSTCAP_BWD_LOOP=0 keeps the
  // launch per step.
  const bool persistent;
  const bool early;  // dW_logit / db_logit go into the caller's slots
  // 3. dW_logit and the bias gradient: exp store: dW = E'^T (alpha Hd), db =
  // sum_r alpha_r E'_r; dense dS: dW = dS^T Hd, db = ds_bias.  Neither needs
  // the reverse loop.  One GPU: after the loop, concurrent with the input-token
  // gradients (3.864-3.872 ms per step vs 3.961 before the loop, 3.889
  // concurrent with it, 3.946 GEMM before / column sums during it;
  // profiles/r2/ab_vh_sched.txt).  Data parallelism runs them concurrently
  // with the loop, so the vocab head's all-reduce hides under it.
  const bool early_comm;
  // DP overlap (set_grad_events): vocab head / embedding gradients final events
  const bool grad_ev;
  // (data parallelism: dW_logit right after the persistent loop, so the vocab
  // head's all-reduce starts ~270 us before the backward ends and hides under
  // the post-loop chain -- test_gpu_dist.py; late, it would start at the end)
  const int dw_late_at;
  const DwStart dw_start;
  // (the bias gradient as two extra bf16 columns (alpha hi / lo) of the dW
  // GEMM instead of the column sums measured slower: the N = 528 GEMM took
  // ~100 us longer, profiles/r3/ab_dbdw.txt)
  // dW GEMM over augmented rows [alpha Hd | alpha_hi | alpha_lo | 0 ...]
  // (bf16, H + dw_pad columns): the same pass over E' also yields the bias
  // gradient (columns H, H + 1 of the product), instead of a separate
  // column-sum pass over the 753 MB exp store.  CSTCAP_DW_AUG=0: the separate
  // column sums (vgrad_colsum).
  const bool dw_aug;
  // dW_logit and the bias column sums run on the side stream under the
  // latency-bound reverse loop (data parallelism: the vocab head's all-reduce
  // starts there too).  Round 4: with the bias column sums in fewer
  // workgroups (vocab_grad.hip) this beats the sums-under-the-loop /
  // dW-after-it schedule on one GPU too: interleaved A/B 3.591-3.604 vs
  // 3.628-3.682 ms per step (profiles/r4/README_r4.md).
  // dW = E'^T (alpha Hd): M = V, N = H, K = NR.  As one GEMM the 256 x 256
  // tiles put only (V / 256) x (H / 256) = 82 workgroups on the 256 CUs; a
  // split-K batch over groups of decode steps multiplies the tiles in flight,
  // the partial products summed afterwards (4 groups: 3.745-3.774 vs
  // 3.792-3.831 ms per step for one GEMM, 7 groups 3.862-3.873,
  // profiles/r3/ab_sched.txt).  The groups split the rows, not the steps:
  // tied to the step count, the 29 steps of an XE step ran one K = 37k GEMM
  // (712 vs 461 us, profiles/r6/steps_xe3.txt)
  const int64_t dw_split;
  const int64_t ldhs;  // columns of the scaled Hd rows
  // Forward X: the loop's first operands are the row weights of this pass and
  // X itself, so the pass runs on the main stream -- no hop to the side stream
  // and back before the loop; the side stream's dW work waits for it.
  // (3.416-3.427 vs 3.429-3.431 ms per step with the pass on the side stream,
  // interleaved on one box, profiles/r5/tail/ab_ohm_*.json)
  const bool oh_main;
  // exp-store range guard: rows whose LSE jumped by > 60 since the previous
  // step are listed and recomputed exactly (vocab_grad.hip vgrad_fix)
  const bool guard_rows;
  // label smoothing: the uniform part of dS as three rank-1 terms -- the X
  // shift before the loop, the broadcast add onto dW_logit / db_logit after
  // dw_gemm (kernels/label_smooth.hip)
  const bool ls;
  // MFMA attention path backward: dalpha partials from the step kernel's
  // epilogue (lstm.hip) + att_bwd_mfma (attention.hip); else att_bwd
  const int CPAD;
  const bool att_mfma;
  // the attention backward of step t + 1 runs as extra workgroups of step t's
  // launch (lstm.hip att_bwd_fused_wg) instead of a launch of its own between
  // the two reverse steps; the dalpha partials alternate between two buffers
  // (att8: 4.717 / 4.728 vs 4.884 / 4.939 ms per step unfused, interleaved on
  // one box, profiles/r5/README_r5.md)
  const bool att_fuse;
  const bool emb_direct;   // d_emb goes into the caller's slot
  const bool vg_direct;    // video-gate / FeatPool backward here (vg_bwd)
  const bool slot_direct;  // layer 0's weight gradients go into dw_slots
  // (an initial state adds its own term onto dW_hh afterwards: through dWx)
  const bool slot_map;
  // dHd = alpha X, X = E' W, is computed in chunks of steps in reverse time
  // order on the side stream, one event per chunk: reverse step t waits only
  // for the chunk that holds its rows, so the loop starts after the first
  // (smallest) chunk instead of after the whole 35,840-row GEMM, and the rest
  // of the GEMM runs under the loop
  const std::vector<std::array<int64_t, 2>> dhd_chunks;  // [t0, t1)

  // ---- tensors allocated on the main stream, touched by a side stream: alive to the final join
  at::Tensor buf, Ev, hd2, dHd;          // E (or dense dS) as bf16 / its K = V columns / Hd rows
  at::Tensor oh_a, oh_ys, oh_b, oh_yx;   // the row's one-hot weights / tokens for the loop (forward X)
  at::Tensor dWlog, dblog, alpha, hs, cs_part, fix;
  at::Tensor ls_part, ls_gs;  // label smoothing: the rank-1 sums' partials / (H + 1) result
  at::Tensor dG_all, dc, whhT;
  at::Tensor d_emb, sort_ws, stok, srow, S_tok, S64;
  at::Tensor dpre_part, dwa_part, dba_part, gvb16, dal_part, att_flags;
  AttBwdEpi abe{};
  std::vector<at::Tensor> whhT_up, dG_up, dc_up;
  at::Tensor dX_up;
  at::Tensor dgv_part, dGv_side, dvg;
  std::vector<at::Tensor> vg_keep;  // the video-gate / FeatPool backward's side-stream temporaries
  at::Tensor dGx, dG2, dWx, dWq;

  // ---- set by exactly one phase each --------------------------------------
  bool rows_early = false;  // scaled_rows(): the scaled Hd rows are formed
  bool dw_fused = false;    // dw_gemm(): the bias gradient came out of the dW pass
  bool hh_in_slot = false;  // recurrent_dw(): dW_hh stored straight into its slot
  bool ie_in_slot = false;  // input_dw(): dW_ie stored straight into its slot

  explicit Backward(const BwdArgs& a)
      : BwdArgs(a),
        n_steps(logits16.size(0)), R(logits16.size(1)), ldl(logits16.size(2)), H4(wx.size(0)),
        H(H4 / 4), E(wx.size(1) - H), V(wlog.size(0)), T_sel(seq.size(1)), NR(n_steps * R),
        st(cur_stream()), dev(wx.device()), f32(at::TensorOptions().dtype(at::kFloat).device(dev)),
        i32(at::TensorOptions().dtype(at::kInt).device(dev)), has_sel(nonempty(dg_sel)),
        has_xe(nonempty(dg_xe)), RNG(rng_ptr(rng)),
        ao(AttOperands::parse(att, Site::Backward, H, R, 0, n_steps)), has_att(ao.on), Bv(ao.Bv),
        C(ao.C), A(ao.A), vdiv(ao.vdiv), per_frame(ao.per_frame), NWA(per_frame ? C : 1), KD(H4 + A),
        upw(UpperLayers::parse(up, Site::Backward, has_att, !state0.empty(), H, n_steps)),
        NL(upw.NL), s0(InitState::parse(state0, Site::Backward, has_att, R, H)), has_s0(s0.on),
        aux(device_aux((int)dev.index())), side(aux.side[0]), side2(aux.side[1]),
        have_x(nonempty(xw)), ds_ready(nonempty(ds_bias)),
        persistent(bwd_loop_mode() != 0 && NL == 1 && !has_att && !has_s0 &&
                   lstm_bwd_loop_ok((int)R, (int)H, (int)n_steps)),
        early(nonempty(out_wlog)), early_comm(early && comm_stream != 0),
        grad_ev(grad_events_on() && early),
        dw_late_at(early_comm || (grad_events_on() && early) ? 0 : knobs().dw_late),
        dw_start(!persistent        ? DW_UNDER_LOOP
                 : dw_late_at == 0 ? DW_AFTER_LOOP
                 : dw_late_at == 1 ? DW_AFTER_TOKSUM
                 : dw_late_at == 2 ? DW_AFTER_DEMB
                                   : DW_NOT_STARTED),
        dw_aug(!ds_ready && !knobs().dw_wgrad &&
               (knobs().dw_aug < 0 ? persistent : knobs().dw_aug != 0)),
        dw_split(NR % 4 == 0 ? 4 : (NR % 2 == 0 ? 2 : 1)),
        ldhs(dw_aug ? H + knobs().dw_pad : H), oh_main(have_x && !ds_ready),
        guard_rows(!ds_ready && blog.defined() && blog.numel() == V),
        ls(ls_eps > 0.0 && has_xe), CPAD(ao.CPAD),
        att_mfma(has_att && att_mfma_ok((int)vdiv, (int)C, (int)A, (int)H, per_frame) &&
                 att_bwd_epi_ok((int)vdiv, (int)C, (int)H) && (KD / 64) % 2 == 0),
        att_fuse(att_fuse_on() && att_mfma && n_steps > 1 && ao.u_all.defined() &&
                 ao.u_all.scalar_type() == at::kHalf && ao.u_all.size(0) == n_steps &&
                 ao.u_all.size(1) == R && ao.u_all.size(2) == C && ao.u_all.size(3) == A &&
                 att_bwd_fuse_ok((int)vdiv, (int)C, (int)A, (int)H, (int)Bv, (int)R)),
        emb_direct(nonempty(out_emb)), vg_direct(!has_att && !vg_bwd.empty()),
        slot_direct(!dw_slots.empty()), slot_map(slot_direct && !has_s0), dhd_chunks(make_chunks()) {
    validate();
  }

  std::vector<std::array<int64_t, 2>> make_chunks() const {
    std::vector<std::array<int64_t, 2>> chunks;
    if (oh_main) return chunks;  // (X is final: the loop waits for no chunk)
    if (have_x) return {{0, n_steps}};
    int64_t t1 = n_steps;
    const int64_t k_first = 2, k_rest = 4;  // steps per chunk
    while (t1 > 0) {
      const int64_t k = chunks.empty() ? k_first : k_rest;
      const int64_t t0 = std::max<int64_t>(0, t1 - k);
      chunks.push_back({t0, t1});
      t1 = t0;
    }
    TORCH_CHECK((int)chunks.size() <= MAX_DHD_CHUNKS, "too many decode steps for the dHd chunks");
    return chunks;
  }

  void validate() const {
    if (has_sel) TORCH_CHECK(dg_sel.is_contiguous() && dg_sel.size(1) == T_sel, "dg_sel shape");
    if (has_xe) TORCH_CHECK(dg_xe.is_contiguous() && labels.defined(), "dg_xe needs labels");
    TORCH_CHECK(toks.numel() == n_steps * R, "toks must hold one token per (step, row)");
    TORCH_CHECK(V < 65536, "vocab: token sort supports V < 65536");
    if (have_x)
      TORCH_CHECK(xw.is_cuda() && xw.scalar_type() == at::kFloat && xw.is_contiguous() &&
                      xw.numel() == NR * H && !ds_ready,
                  "xw must be the forward's fp32 (n_steps, R, H) X = E W (exp store only)");
    if (ds_ready) {
      TORCH_CHECK(ds_bias.is_cuda() && ds_bias.scalar_type() == at::kFloat && ds_bias.numel() == V,
                  "ds_bias must be fp32 (V)");
    } else {
      TORCH_CHECK(logits16.scalar_type() == at::kBFloat16,
                  "decoder_backward: the saved rows must be the exp store (forward store_exp) "
                  "unless a dense dS is given");
    }
    TORCH_CHECK(ls_eps >= 0.0 && ls_eps < 1.0, "ls_eps must be in [0, 1)");
    if (ls) {
      TORCH_CHECK(!ds_ready, "label smoothing runs on the exp store, not with a dense dS");
      TORCH_CHECK(ls_wbar.has_value() && ls_wbar->defined() && ls_wbar->is_cuda() &&
                      ls_wbar->scalar_type() == at::kFloat && ls_wbar->is_contiguous() &&
                      ls_wbar->numel() >= H + 1 && H % 8 == 0 && H <= 2048,
                  "ls_wbar must be the forward's fp32 (>= H + 1) mean logit row and bias");
    }
    if (early) {
      TORCH_CHECK(out_wlog.scalar_type() == at::kFloat && out_wlog.is_contiguous() &&
                      out_wlog.size(0) == V && out_wlog.size(1) == H,
                  "out_wlog must be a contiguous fp32 (V, H) tensor");
      TORCH_CHECK(out_blog.scalar_type() == at::kFloat && out_blog.numel() == V, "out_blog shape");
    }
    if (guard_rows) {
      TORCH_CHECK(blog.is_cuda() && blog.scalar_type() == at::kFloat && blog.is_contiguous(),
                  "blog must be a contiguous fp32 GPU tensor");
      TORCH_CHECK(!fix_total.defined() || fix_total.numel() == 0 ||
                      (fix_total.is_cuda() && fix_total.scalar_type() == at::kInt),
                  "fix_total must be an int32 GPU tensor");
    }
    if (emb_direct)
      TORCH_CHECK(out_emb.is_contiguous() && out_emb.scalar_type() == at::kFloat &&
                      out_emb.size(0) == V && out_emb.size(1) == E,
                  "out_emb must be a contiguous fp32 (V, E) tensor");
    if (vg_direct) {
      TORCH_CHECK(vg_nf >= 1 &&
                      ((int64_t)vg_bwd.size() == 6 + 4 * vg_nf ||
                       (int64_t)vg_bwd.size() == 7 + 4 * vg_nf) &&
                      NL == 1 && !has_s0,
                  "vg_bwd = {dst_ie, dst_hh, W_ih slot, W_hh slot, packed W_iv shadow, fc, FeatPool slots, "
                  "inputs, weights(, fc as bf16)}");
      TORCH_CHECK(vg_bwd[4].scalar_type() == at::kBFloat16 && vg_bwd[4].size(0) == H4,
                  "vg_bwd[4]: the packed bf16 (4H, Fv) W_iv shadow");
    }
    if (!has_att)
      TORCH_CHECK(vgate_div >= 1 && R % vgate_div == 0, "vgate_div must divide the rows");
    // dw_slots (direct gradient slots): {W_ih slot (G*H, >= E columns), W_hh slot
    // (G*H, H), dst_ie, dst_hh (int64, G*H: packed row of each PyTorch row),
    // inv_ie, inv_hh (int32, 4H: PyTorch row of each packed row, -1 = unused
    // gate slot)}.  The split-K reduce (kernels/wgrad.hip) stores layer 0's dW_ie
    // and dW_hh rows straight into the slots through the inverse maps; a shape
    // the kernel does not take goes through dWx and a gather + copy instead.
    if (slot_direct) {
      TORCH_CHECK(dw_slots.size() == 6, "dw_slots = {W_ih slot, W_hh slot, dst_ie, dst_hh, inv_ie, inv_hh}");
      const at::Tensor &s_ih = dw_slots[0], &s_hh = dw_slots[1];
      for (const at::Tensor& t : dw_slots) check_cuda(t, "dw_slots");
      TORCH_CHECK(s_ih.scalar_type() == at::kFloat && s_ih.dim() == 2 && s_ih.stride(1) == 1 &&
                      s_ih.size(1) >= E && s_hh.scalar_type() == at::kFloat && s_hh.dim() == 2 &&
                      s_hh.stride(1) == 1 && s_hh.size(1) == H && s_ih.size(0) == s_hh.size(0) &&
                      s_ih.size(0) <= H4,
                  "dw_slots: fp32 W_ih (rows, >= E) / W_hh (rows, H) slots with unit column stride");
      TORCH_CHECK(dw_slots[2].scalar_type() == at::kLong && dw_slots[3].scalar_type() == at::kLong &&
                      dw_slots[2].numel() == s_ih.size(0) && dw_slots[3].numel() == s_hh.size(0),
                  "dw_slots: dst_ie / dst_hh int64, one entry per slot row");
      TORCH_CHECK(dw_slots[4].scalar_type() == at::kInt && dw_slots[5].scalar_type() == at::kInt &&
                      dw_slots[4].is_contiguous() && dw_slots[5].is_contiguous() &&
                      dw_slots[4].numel() == H4 && dw_slots[5].numel() == H4,
                  "dw_slots: inv_ie / inv_hh int32 (4H)");
    }
    TORCH_CHECK(!vg_direct || slot_direct, "vg_bwd needs dw_slots (W_ih / W_hh slots and row maps)");
  }

  hipEvent_t ev(int k) const { return aux.ev[k]; }
  int key(int64_t l, int64_t t) const { return drop_key(NL, l, t); }
  // ---- phases, in schedule order -------------------------------------------
  // main: the vocab head's and the loop's operands.  X-independent preparation
  // of the loop first, then (in the schedule) the wait for X (x_wait: the event
  // engine.launch_x recorded after X = E W): the counter resets, the dc zeros,
  // the W_hh^T copy and the token sort run under the X GEMM instead of between
  // it and the loop (they sat on the critical path after X,
  // profiles/r6/steps_scst*.txt)
  void prepare_operands() {
    buf = logits16.scalar_type() == at::kBFloat16 ? logits16 : logits16.view(at::kBFloat16);
    Ev = buf.view({NR, ldl}).narrow(1, 0, V);  // E (or dense dS), K = V columns
    hd2 = hdrop_all.view({NR, H});
    dHd = have_x ? xw.view({NR, H}) : at::empty({NR, H}, f32);
    if (have_x) {
      oh_a = at::empty({NR}, f32);
      oh_ys = at::empty({NR}, i32);
      if (has_xe) {
        oh_b = at::empty({NR}, f32);
        oh_yx = at::empty({NR}, i32);
      }
    }
    dWlog = early ? out_wlog : at::empty({V, H}, f32);
    dblog = early ? out_blog.view({V}) : at::empty({V}, f32);
    if (!ds_ready) {
      alpha = at::empty({NR}, f32);
      hs = at::empty({NR, ldhs}, wx.options());
      if (!dw_aug) cs_part = at::empty({vgrad_colsum_blocks(NR), V}, f32);
    }
    // (only the row counter fix[0] needs zeroing: the list entries are written
    // by vgrad_onehot before vgrad_fix reads them)
    if (guard_rows) fix = at::empty({1 + NR}, i32);
    if (ls) {
      ls_part = at::empty({ls_rowsum_blocks(NR, LS_GSUM_ROWS), H + 8}, f32);
      ls_gs = at::empty({H + 8}, f32);
    }
    if (fix.defined()) (void)hipMemsetAsync(fix.data_ptr(), 0, sizeof(int), st);
    dG_all = at::empty({n_steps, R, KD}, wx.options());
    dc = at::zeros({R, H}, f32);
    // W_hh^T (H, 4H): K-contiguous B operand of the fused step kernel; with
    // attention [W_hh^T | W_q^T] (H, 4H + A), so the step GEMM over
    // [dG_{t+1} | dq_{t+1}] also adds dq_{t+1} W_q (q_{t+1} = W_q h_t) into dh_t
    whhT = has_att ? at::cat({wx.narrow(1, E, H).t(), ao.wq.t()}, 1).contiguous()
                   : wx.narrow(1, E, H).t().contiguous();
    // token-only operands of the embedding / input-weight gradients: rows
    // grouped by input token (counting sort), per-token sum scratch
    d_emb = emb_direct ? out_emb : at::empty({V, E}, f32);
    sort_ws = at::empty({2 * V + 1}, i32);
    stok = at::empty({NR}, i32), srow = at::empty({NR}, i32);
    S_tok = at::empty({V, H4}, wx.options());  // per-token gate-gradient sums
    // rows of long groups only (token_long_zero); fp64: exact fixed-point sums
    S64 = at::empty({V, H4}, f32.dtype(at::kDouble));
  }

  // side2: the input-token counting sort, off the critical path (needed after
  // the loop); records EV_TOK_SORTED
  void token_sort() {
    launch_token_sort(toks.data_ptr<int64_t>(), (int)NR, (int)V, sort_ws.data_ptr<int>(),
                      stok.data_ptr<int>(), srow.data_ptr<int>(), side2.stream());
    launch_token_long_zero(sort_ws.data_ptr<int>(), (int)V, (int)H4, S64.data_ptr<double>(),
                           side2.stream());
    (void)hipEventRecord(ev(EV_TOK_SORTED), side2.stream());
  }

  // s: alpha, one-hot terms folded into E (dS = diag(alpha) E'), then the
  // exp-store range guard's exact rows
  void onehot_pass(hipStream_t s) {
    VGradRows va{(int)R, (int)n_steps, (int)T_sel, (int)H, (int)V, lse.data_ptr<float>(),
                 has_sel ? seq.data_ptr<int64_t>() : nullptr,
                 has_sel ? dg_sel.data_ptr<float>() : nullptr,
                 has_xe ? labels.data_ptr<int64_t>() + 1 : nullptr,
                 has_xe ? labels.size(1) : 0, has_xe ? dg_xe.data_ptr<float>() : nullptr,
                 has_xe ? dg_xe.size(1) : 0, guard_rows ? fix.data_ptr<int>() : nullptr,
                 ptr_or_null<float>(oh_a), ptr_or_null<int>(oh_ys), ptr_or_null<float>(oh_b),
                 ptr_or_null<int>(oh_yx), have_x ? dHd.data_ptr<float>() : nullptr,
                 exp_zero_off ? 1 : 0, ls ? (float)ls_eps : 0.f};
    launch_vgrad_onehot(va, reinterpret_cast<uint16_t*>(buf.data_ptr()), ldl,
                        alpha.data_ptr<float>(), s);
    if (guard_rows)
      launch_vgrad_fix(va, reinterpret_cast<const uint16_t*>(hd2.data_ptr()),
                       reinterpret_cast<const uint16_t*>(wlog.data_ptr()), blog.data_ptr<float>(),
                       reinterpret_cast<uint16_t*>(buf.data_ptr()), ldl, alpha.data_ptr<float>(),
                       ptr_or_null<int>(fix_total), s);
    // forward X: final here (the guard's rows recomputed), read next by the loop
    if (ls && have_x) ls_shift(0, NR, s);
    stamp(STAMP_BWD_ONEHOT, s);
  }

  // label smoothing: the rows' weights eps dg_xe, and X_r += (eps dg_r / alpha_r) wbar
  LsRowW ls_rows() const {
    return LsRowW{dg_xe.data_ptr<float>(), dg_xe.size(1), (int)R, (float)ls_eps, nullptr};
  }
  void ls_shift(int64_t r0, int64_t nr, hipStream_t s) {
    launch_ls_shift(dHd.data_ptr<float>(), alpha.data_ptr<float>(), ls_wbar->data_ptr<float>(),
                    ls_rows(), r0, nr, (int)H, s);
  }

  // side (current): X = E' W, chunk by chunk; the reverse loop reads alpha X
  // (row scales at load), and the scaled Hd rows of the dW GEMM are formed
  // under it.  Records EV_DHD_CHUNK0 + ci after chunk ci.
  void x_chunks() {
    for (size_t ci = 0; ci < dhd_chunks.size(); ++ci) {
      const int64_t r0 = dhd_chunks[ci][0] * R, nr = (dhd_chunks[ci][1] - dhd_chunks[ci][0]) * R;
      at::Tensor dst = dHd.narrow(0, r0, nr);
      if (!have_x) at::mm_out(dst, Ev.narrow(0, r0, nr), wlog, at::kFloat);
      if (ls && !have_x) ls_shift(r0, nr, side.stream());
      (void)hipEventRecord(ev(EV_DHD_CHUNK0 + (int)ci), side.stream());
      if (ci == 0) stamp(STAMP_BWD_DHD0, side.stream());
    }
  }

  // side: the dW GEMM's scaled Hd rows alpha Hd.  With the persistent loop
  // they are formed early: they need only alpha, so next to the fold on the
  // main stream instead of between the loop and the GEMM
  void scaled_rows() {
    launch_vgrad_rows(alpha.data_ptr<float>(), NR, (int)H,
                      reinterpret_cast<const uint16_t*>(hd2.data_ptr()), nullptr,
                      reinterpret_cast<uint16_t*>(hs.data_ptr()), side.stream(), (int)ldhs);
    rows_early = true;
  }

  // side (current): dW_logit
  void dw_gemm() {
    const at::Tensor& rhs = ds_ready ? hd2 : hs;
    if (dw_aug) {
      // split-K batch over the augmented rows; the partial products summed
      // into the dW slot and the bias gradient (hi + lo columns).  (One GEMM
      // over all rows with the measured hipBLASLt choice: 3.439-3.451 vs
      // 3.330-3.343 ms per step, profiles/r6/README_r6.md)
      const int64_t kr = NR / dw_split;
      at::Tensor p;  // (split, V, ldhs)
      if (knobs().dw_tuned) {
        p = at::empty({dw_split, V, ldhs}, f32);
        gemm_bf16_tuned_batched(
            p, buf.view({NR, ldl}).as_strided({dw_split, kr, V}, {kr * ldl, ldl, 1}), true,
            hs.view({dw_split, kr, ldhs}), false, 24);
      } else {
        at::Tensor a = buf.view({NR, ldl}).as_strided({dw_split, V, kr}, {kr * ldl, 1, ldl});
        p = at::bmm(a, hs.view({dw_split, kr, ldhs}), at::kFloat);
      }
      at::sum_out(dWlog, p.narrow(2, 0, H), 0);
      at::sum_out(dblog, p.narrow(2, H, 2), at::IntArrayRef({0, 2}));
      dw_fused = true;
      return;
    }
    if (!ds_ready && knobs().dw_wgrad &&
        wgrad_tn_into(buf.view({NR, ldl}), ldl, hs, H, V, H, NR, dWlog.data_ptr<float>(), H, V,
                      nullptr, 0, side.stream(), alpha.data_ptr<float>(), dblog.data_ptr<float>())) {
      dw_fused = true;
      return;
    }
    // (hipBLASLt's measured choice as one GEMM: 3.683-3.731 vs 3.628-3.682 ms
    // per step, the round-4 hand-written GEMM 3.746-3.795: the split-K batch)
    if (dw_split == 1) {
      at::mm_out(dWlog, Ev.t(), rhs, at::kFloat);
      return;
    }
    const int64_t kr = NR / dw_split;
    at::Tensor a = buf.view({NR, ldl}).as_strided({dw_split, V, kr}, {kr * ldl, 1, ldl});
    at::sum_out(dWlog, at::bmm(a, rhs.view({dw_split, kr, H}), at::kFloat), 0);
  }

  // side (current): the vocab head's weight gradients: scaled rows (unless
  // formed early), dW_logit, the bias gradient; records EV_SIDE_DONE (and grad
  // event 0; the comm stream waits on it under data parallelism)
  void vocab_head_dw() {
    if (!ds_ready && !rows_early) scaled_rows();
    stamp(STAMP_BWD_DHD, side.stream());
    dw_gemm();
    stamp(STAMP_BWD_DW, side.stream());
    if (ds_ready)
      dblog.copy_(ds_bias);
    else if (!dw_fused)
      launch_vgrad_colsum(reinterpret_cast<const uint16_t*>(buf.data_ptr()), ldl, (int)V, NR,
                          alpha.data_ptr<float>(), cs_part.data_ptr<float>(),
                          dblog.data_ptr<float>(), side.stream());
    if (ls) {
      // the uniform part: (1 / V) sum_r eps dg_r [Hd_r | 1] onto every row of
      // dW_logit / entry of db_logit, once both are written
      launch_ls_rowsum(reinterpret_cast<const uint16_t*>(hd2.data_ptr()), NR, (int)H, ls_rows(),
                       LS_GSUM_ROWS, (float)(1.0 / (double)V), ls_part.data_ptr<float>(),
                       ls_gs.data_ptr<float>(), side.stream());
      launch_ls_add(dWlog.data_ptr<float>(), dblog.data_ptr<float>(), ls_gs.data_ptr<float>(),
                    (int)V, (int)H, side.stream());
    }
    (void)hipEventRecord(ev(EV_SIDE_DONE), side.stream());
    if (grad_ev) record_grad_event(aux.grad_ev[0], side.stream(), 0);
    if (early_comm)
      (void)hipStreamWaitEvent(reinterpret_cast<hipStream_t>(comm_stream), ev(EV_SIDE_DONE), 0);
  }
  // main -> side: the same after a persistent loop: fork, then the gradients
  // on the side stream (the vocab head's weight gradients after the loop --
  // every CU is the loop's until it ends --, concurrently with the post-loop
  // chain; CSTCAP_DW_LATE=1 / 2: started after the token sums / the d_emb GEMM
  // of that chain instead)
  void fork_vocab_head_dw() {
    fork(ev(EV_DW_START), st, side.stream());
    c10::hip::HIPStreamGuard guard(side);
    vocab_head_dw();
  }

  // main: the reverse loop's scratch: attention partials, the upper layers'
  // W_hh_l^T (K-contiguous B operands), gate gradients, carries
  // (the loop operands filled on the second side stream concurrently with
  // the one-hot pass measured slower: att8 4.487-4.516 vs 4.379-4.417 ms,
  // headline 3.424-3.514 vs 3.337-3.339, profiles/r5/tail/ab_prep*.json)
  void prepare_loop() {
    if (att_mfma) {
      // gate tables with the 4 packed gates of a unit innermost: (Bv, H, CP, 4)
      gvb16 = at::zeros({Bv, H, CPAD, 4}, wx.options());
      gvb16.narrow(2, 0, C).copy_(ao.gv.view({Bv, C, H, 4}).permute({0, 2, 1, 3}));
      dal_part = at::empty({2, H / 64, R, CPAD}, f32);
      if (att_fuse) att_flags = at::zeros({n_steps, Bv}, i32);
      abe = AttBwdEpi{reinterpret_cast<const uint16_t*>(gvb16.data_ptr()), (int)vdiv, (int)C, CPAD,
                      dal_part.data_ptr<float>()};
      dpre_part = at::zeros({Bv, C, A}, f32);
      dwa_part = at::zeros({Bv, A}, f32);
      dba_part = at::zeros({Bv, 1}, f32);
    } else if (has_att) {
      const int64_t nwg = Bv * att_groups((int)vdiv);
      dpre_part = at::zeros({nwg, C, A}, f32);
      dwa_part = at::zeros({nwg, NWA * A}, f32);
      dba_part = at::zeros({nwg, NWA}, f32);
    }
    whhT_up.resize(NL), dG_up.resize(NL), dc_up.resize(NL);
    dX_up = NL > 1 ? at::empty({R, H}, f32) : at::Tensor();
    for (int64_t l = 1; l < NL; ++l) {
      whhT_up[l] = upw(l, 0).narrow(1, H, H).t().contiguous();
      dG_up[l] = at::empty({n_steps, R, H4}, wx.options());
      dc_up[l] = at::zeros({R, H}, f32);
    }
  }

  // main: the whole reverse recurrence as one launch, after every dHd chunk
  // (forward X: none)
  void loop_persistent() {
    for (size_t ci = 0; ci < dhd_chunks.size(); ++ci)
      (void)hipStreamWaitEvent(st, ev(EV_DHD_CHUNK0 + (int)ci), 0);
    BwdLoopArgs la{};
    la.dG = reinterpret_cast<uint16_t*>(dG_all.data_ptr());
    la.whhT = reinterpret_cast<const uint16_t*>(whhT.data_ptr());
    la.dh = dHd.data_ptr<float>();
    la.scale = ds_ready ? nullptr : alpha.data_ptr<float>();
    if (have_x) {
      la.oh_W = reinterpret_cast<const uint16_t*>(wlog.data_ptr());
      la.oh_a = oh_a.data_ptr<float>();
      la.oh_ys = oh_ys.data_ptr<int>();
      if (has_xe) {
        la.oh_b = oh_b.data_ptr<float>();
        la.oh_yx = oh_yx.data_ptr<int>();
      }
    }
    la.gates = reinterpret_cast<const uint16_t*>(gates_all.data_ptr());
    la.c_all = c_all.data_ptr<float>();
    la.dc_out = dc.data_ptr<float>();
    la.R = (int)R;
    la.H = (int)H;
    la.T = (int)n_steps;
    la.cell = (int)cell;
    la.drop_p = (float)drop_p;
    la.rng = RNG;
    la.cnt = loop_counters((int)dev.index(), lstm_bwd_loop_counter_ints((int)R, (int)H));
    la.err = device_err_word((int)dev.index());
    la.poll_bound = poll_bound();
    la.form = bwd_loop_mode() == 2 ? 0 : 1;
    if (la.form == 0) la.xb = loop_xb((int)dev.index(), lstm_bwd_loop_xb_floats((int)R, (int)H));
    TORCH_CHECK(gates_all.is_contiguous() && c_all.is_contiguous() && dG_all.is_contiguous() &&
                    dHd.is_contiguous() && gates_all.size(0) >= n_steps && c_all.size(0) >= n_steps,
                "persistent reverse loop: operand layout");
    launch_lstm_bwd_loop(la, st);
    stamp(STAMP_BWD_LOOP0, st);
  }

  // the vocab head's gradient rows enter the loop as X = E' W with the row
  // scales alpha applied at load (exp store); a dense dS gives dHd directly
  const float* dh_scale_t(int64_t t) const {
    return ds_ready ? nullptr : alpha.data_ptr<float>() + t * R;
  }
  // forward X: the one-hot rows of the top layer's h gradient (see DhOneHot)
  DhOneHot dh_onehot_t(int64_t t) const {
    if (!have_x) return DhOneHot{};
    return DhOneHot{reinterpret_cast<const uint16_t*>(wlog.data_ptr()),
                    oh_a.data_ptr<float>() + t * R, oh_ys.data_ptr<int>() + t * R,
                    has_xe ? oh_b.data_ptr<float>() + t * R : nullptr,
                    has_xe ? oh_yx.data_ptr<int>() + t * R : nullptr};
  }

  // main: the reverse recurrence, one fused launch per (step, layer); step t
  // waits for the dHd chunk that holds its rows
  void loop_per_step() {
    size_t next_chunk = 0;
    for (int64_t t = n_steps - 1; t >= 0; --t) {
      if (next_chunk < dhd_chunks.size() && t == dhd_chunks[next_chunk][1] - 1)
        (void)hipStreamWaitEvent(st, ev(EV_DHD_CHUNK0 + (int)next_chunk++), 0);  // this chunk's dHd rows
      const DhOneHot oh_t = dh_onehot_t(t);
      // top layer first: its h gradient comes from the vocab head (dHd, with the
      // vocab dropout mask); layer l < top gets dG_{l+1, t} W_ih_{l+1} through
      // the inter-layer dropout mask of layer l's output
      for (int64_t l = NL - 1; l >= 1; --l) {
        const float* dh_in = dHd.data_ptr<float>() + t * R * H;
        const float* dh_sc = dh_scale_t(t);
        const DhOneHot* ohp = &oh_t;
        if (l < NL - 1) {
          at::mm_out(dX_up, dG_up[l + 1][t], upw(l + 1, 0).narrow(1, 0, H), at::kFloat);
          dh_in = dX_up.data_ptr<float>();
          dh_sc = nullptr;
          ohp = nullptr;
        }
        launch_lstm_step_bwd(
            t + 1 < n_steps ? reinterpret_cast<const uint16_t*>(dG_up[l][t + 1].data_ptr()) : nullptr,
            reinterpret_cast<const uint16_t*>(whhT_up[l].data_ptr()), dh_in,
            dc_up[l].data_ptr<float>(), reinterpret_cast<const uint16_t*>(upw(l, 3)[t].data_ptr()),
            upw(l, 2)[t].data_ptr<float>(), t > 0 ? upw(l, 2)[t - 1].data_ptr<float>() : nullptr,
            (int)R, (int)H, (float)drop_p, RNG, key(l, t),
            reinterpret_cast<uint16_t*>(dG_up[l][t].data_ptr()), (int)H4, st, (int)cell, dh_sc,
            nullptr, ohp);
      }
      const float* dh0_in = dHd.data_ptr<float>() + t * R * H;
      const float* dh0_sc = dh_scale_t(t);
      if (NL > 1) {
        at::mm_out(dX_up, dG_up[1][t], upw(1, 0).narrow(1, 0, H), at::kFloat);
        dh0_in = dX_up.data_ptr<float>();
        dh0_sc = nullptr;
      }
      if (att_mfma) {
        abe.dal_part = dal_part[t & 1].data_ptr<float>();
        abe.flags = nullptr;
        if (att_fuse && t + 1 < n_steps) {  // + step t + 1's attention backward
          abe.flags = att_flags[t + 1].data_ptr<int>();
          abe.dal_next = dal_part[(t + 1) & 1].data_ptr<float>();
          abe.alpha = ao.alpha_all[t + 1].data_ptr<float>();
          abe.u = reinterpret_cast<const uint16_t*>(ao.u_all[t + 1].data_ptr());
          abe.wa = ao.wa.data_ptr<float>();
          abe.Bv = (int)Bv;
          abe.A = (int)A;
          abe.G4 = (int)H4;
          abe.dP_acc = dpre_part.data_ptr<float>();
          abe.dwa_part = dwa_part.data_ptr<float>();
          abe.dba_part = dba_part.data_ptr<float>();
          abe.poll_bound = poll_bound();
          abe.poll_err = device_err_word((int)dev.index());
        }
      }
      launch_lstm_step_bwd(
          t + 1 < n_steps ? reinterpret_cast<const uint16_t*>(dG_all[t + 1].data_ptr()) : nullptr,
          reinterpret_cast<const uint16_t*>(whhT.data_ptr()), dh0_in, dc.data_ptr<float>(),
          reinterpret_cast<const uint16_t*>(gates_all[t].data_ptr()), c_all[t].data_ptr<float>(),
          t > 0 ? c_all[t - 1].data_ptr<float>() : (has_s0 ? s0.c0.data_ptr<float>() : nullptr),
          (int)R, (int)H, (float)drop_p, RNG, key(0, t),
          reinterpret_cast<uint16_t*>(dG_all[t].data_ptr()), (int)KD, st, (int)cell, dh0_sc,
          att_mfma ? &abe : nullptr, NL == 1 ? &oh_t : nullptr);
      if (att_fuse) {
        // (step t's attention backward: in step t - 1's launch, or after the loop)
      } else if (att_mfma)
        att_bwd_mfma_step(t);
      else if (has_att)  // dq_t (bf16, columns [4H, 4H+A) of dG_t) + dP / dw_a / db_a partials
        launch_att_bwd(reinterpret_cast<uint16_t*>(dG_all[t].data_ptr()), (int)KD,
                       ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(),
                       t > 0 ? ao.q_all[t].data_ptr<float>() : nullptr,
                       ao.alpha_all[t].data_ptr<float>(), ao.wa.data_ptr<float>(), (int)Bv,
                       (int)vdiv, (int)C, (int)A, (int)H4, t > 0 ? 1 : 0,
                       dpre_part.data_ptr<float>(), dwa_part.data_ptr<float>(),
                       dba_part.data_ptr<float>(), st, per_frame);
      if (t == n_steps - 1) stamp(STAMP_BWD_LOOP0, st);
    }
  }

  // main: step t's attention backward on the MFMA path as a launch of its own
  void att_bwd_mfma_step(int64_t t) {
    launch_att_bwd_mfma(dal_part[t & 1].data_ptr<float>(), (int)(H / 64), (int)R,
                        ao.alpha_all[t].data_ptr<float>(),
                        t > 0 ? ao.q_all[t].data_ptr<float>() : nullptr, ao.pre.data_ptr<float>(),
                        ao.wa.data_ptr<float>(), (int)Bv, (int)vdiv, (int)C, CPAD, (int)A, (int)H4,
                        reinterpret_cast<uint16_t*>(dG_all[t].data_ptr()), (int)KD, t > 0 ? 1 : 0,
                        dpre_part.data_ptr<float>(), dwa_part.data_ptr<float>(),
                        dba_part.data_ptr<float>(), st);
  }

  // main -> side2: attention: the per-frame gate-table gradient dGv needs only
  // the finished dG rows; it runs on the second side stream under the post-loop
  // chain (joined in collect()); records EV_DGV_DONE
  void att_dgv() {
    dgv_part = at::empty({att_dgv_chunks((int)n_steps), Bv, C, H4}, f32);
    dGv_side = at::empty({Bv, C, H4}, f32);
    fork(ev(EV_LOOP_DONE), st, side2.stream());
    launch_att_dgv(reinterpret_cast<const uint16_t*>(dG_all.data_ptr()), (int)KD,
                   ao.alpha_all.data_ptr<float>(), (int)n_steps, (int)R, (int)Bv, (int)vdiv, (int)C,
                   (int)H4, dgv_part.data_ptr<float>(), side2.stream());
    {
      c10::hip::HIPStreamGuard guard(side2);
      at::sum_out(dGv_side, dgv_part, 0);
    }
    (void)hipEventRecord(ev(EV_DGV_DONE), side2.stream());
  }

  // main -> side2: the video-gate gradient (Bv, 4H): sum over time and over
  // the rows of each video in one pass (kernels/embed_grad.hip), streaming the
  // finished dG rows on the second side stream under the post-loop GEMM chain
  // (joined in collect()); with vg_bwd the FeatPool backward after it; records
  // EV_DVG_DONE
  void video_gate_grads() {
    dvg = at::empty({R / vgate_div, H4}, f32);
    fork(ev(EV_LOOP_DONE), st, side2.stream());
    launch_video_gate_grad(reinterpret_cast<const uint16_t*>(dG_all.data_ptr()), KD, (int)n_steps,
                           (int)R, (int)vgate_div, (int)H4, dvg.data_ptr<float>(), side2.stream());
    if (vg_direct) {
      // video-gate and FeatPool backward on the same stream (ops/featpool.py
      // _FeatPoolVgateFn does this after the call otherwise): dfc = dvg W_iv,
      // dW_iv = dvg^T fc into W_ih's slot, FeatPool gradients into theirs
      c10::hip::HIPStreamGuard guard(side2);
      // dfc = dvg W_iv (packed gate order on both sides: vg_bwd[4] is the
      // engine's packed bf16 W_iv shadow, zero rows in unused slots) and
      // dW_iv = dvg^T fc (PyTorch gate order, into the slot's column range):
      // bf16 operands, fp32 accumulation and output, the measured hipBLASLt
      // choices.  As fp32 at::mm, dfc ran as an MT32x16 fp32 kernel: 79 us
      // alone and 380-575 us next to the dW_logit GEMM after the persistent
      // loop (profiles/r6/steps_xe*.txt)
      const int64_t Fv = vg_bwd[4].size(1);
      at::Tensor dvg_p16 = dvg.to(at::kBFloat16);
      at::Tensor dvg16 = dvg_p16.index_select(1, vg_bwd[0]);  // PyTorch gate order
      at::Tensor dfc = at::empty({dvg.size(0), Fv}, f32);
      at::Tensor wiv16 = vg_bwd[4];
      // (fc as bf16: the forward's FeatPool epilogue wrote it next to fc)
      at::Tensor fc16 = (int64_t)vg_bwd.size() == 7 + 4 * vg_nf ? vg_bwd.back()
                                                               : vg_bwd[5].to(at::kBFloat16);
      TORCH_CHECK(fc16.scalar_type() == at::kBFloat16 && fc16.sizes() == vg_bwd[5].sizes() &&
                      fc16.is_contiguous(),
                  "vg_bwd: fc as bf16 must match fc");
      gemm_bf16_tuned(dfc, dvg_p16, false, wiv16, false, 24);
      at::Tensor wiv_slot = vg_bwd[2].narrow(1, E, Fv);
      gemm_bf16_tuned(wiv_slot, dvg16, true, fc16, false, 24);
      std::vector<at::Tensor> outs(vg_bwd.begin() + 6, vg_bwd.begin() + 6 + 2 * vg_nf);
      std::vector<at::Tensor> xs(vg_bwd.begin() + 6 + 2 * vg_nf, vg_bwd.begin() + 6 + 3 * vg_nf);
      std::vector<at::Tensor> wsv(vg_bwd.begin() + 6 + 3 * vg_nf, vg_bwd.begin() + 6 + 4 * vg_nf);
      // (vg_idx: the forward read its rows out of the resident tables by index)
      (void)featpool_backward(dfc, vg_bwd[5], xs, wsv, vg_p, outs, vg_idx, vg_C);
      vg_keep = {dfc, dvg16, dvg_p16, fc16};
    }
    (void)hipEventRecord(ev(EV_DVG_DONE), side2.stream());
  }

  // 6. weight gradients dWx = dG^T [x ; h_prev].  The K = steps*rows
  //    reductions run as batched GEMMs over groups of steps (many more output
  //    tiles in flight than one K = 35k GEMM), summed afterwards.
  at::Tensor grouped_wgrad(const at::Tensor& a_rows, const at::Tensor& b_rows, int64_t nsteps) const {
    int64_t G = 1;  // steps per group: largest divisor <= 7
    for (int64_t g = 7; g >= 1; --g)
      if (nsteps % g == 0) { G = g; break; }
    const int64_t nc = nsteps / G;
    at::Tensor a = a_rows.view({nc, G * R, a_rows.size(1)}).transpose(1, 2);
    at::Tensor b = b_rows.reshape({nc, G * R, b_rows.size(1)});
    return at::bmm(a, b, at::kFloat).sum(0);
  }

  // main: the outputs of the weight-gradient phases
  void alloc_weight_grads() {
    dGx = dG_all.view({NR, KD});  // [dG | dq] rows
    dG2 = dGx.narrow(1, 0, H4);
    dWx = at::empty({H4, E + H}, f32);
    dWq = has_att ? at::empty({A, H}, f32) : at::Tensor();
  }

  // side (current): recurrent columns dW_hh = sum_t dG_t^T h_{t-1} (+ dG_0^T h0
  // with an initial state); with attention the extra rows of [dG | dq]^T h_prev
  // are dW_q; records EV_SIDE_DONE.
  // The recurrent-weight gradient (hand-written split-K GEMM, kernels/wgrad.hip)
  // on the first side stream, idle after dW_logit + the bias sums, concurrent
  // with the input-token chain: interleaved on one box 3.351-3.386 vs
  // 3.362-3.402 ms per step after that chain on the main stream
  // (profiles/r5/tail/ab_ws_*.json; with the round-4 vendor GEMMs the same
  // move measured slower)
  void recurrent_dw() {
    const hipStream_t ws = side.stream();
    if (n_steps > 1 && h_all.is_contiguous() &&
        wgrad_tn_into(dGx.narrow(0, R, (n_steps - 1) * R), KD, h_all, H, KD, H,
                      (n_steps - 1) * R,
                      slot_map ? dw_slots[1].data_ptr<float>() : dWx.data_ptr<float>() + E,
                      slot_map ? dw_slots[1].stride(0) : E + H, H4,
                      has_att ? dWq.data_ptr<float>() : nullptr, H, ws, nullptr, nullptr,
                      slot_map ? dw_slots[5].data_ptr<int>() : nullptr)) {
      // (hand-written split-K MFMA kernel, kernels/wgrad.hip: rows [0, 4H) of
      // [dG | dq]^T h_prev into dW_hh's columns of dWx -- or, through the row
      // map, into W_hh's gradient slot --, the dq rows into dW_q)
      hh_in_slot = slot_map;
    } else if (n_steps > 1) {
      at::Tensor wh;
      wh = grouped_wgrad(dGx.narrow(0, R, (n_steps - 1) * R),
                         h_all.narrow(0, 0, n_steps - 1).reshape({(n_steps - 1) * R, H}),
                         n_steps - 1);
      dWx.narrow(1, E, H).copy_(wh.narrow(0, 0, H4));
      if (has_att) dWq.copy_(wh.narrow(0, H4, A));
    } else {
      dWx.narrow(1, E, H).zero_();
      if (has_att) dWq.zero_();
    }
    if (has_s0) dWx.narrow(1, E, H).add_(at::mm(dG2.narrow(0, 0, R).t(), s0.h0, at::kFloat));
    if (slot_direct && !hh_in_slot)  // (a shape outside the kernel: gather + copy)
      dw_slots[1].copy_(dWx.narrow(1, E, H).index_select(0, dw_slots[3]));
    (void)hipEventRecord(ev(EV_SIDE_DONE), side.stream());  // (joined in collect())
  }

  // 5. input-token gradients through the per-token sums S[v] = sum of the dG
  //    rows whose input token is v (bf16, V x 4H): embedding gradient S W_ie,
  //    input-weight gradient S^T emb -- GEMMs over V rows instead of n*R
  // main: the sums, after the token sort (second side stream)
  void token_sums() {
    (void)hipStreamWaitEvent(st, ev(EV_TOK_SORTED), 0);
    launch_token_group_sum(reinterpret_cast<const uint16_t*>(dG_all.data_ptr()), (int)H4, KD,
                           stok.data_ptr<int>(), srow.data_ptr<int>(), (int)NR,
                           sort_ws.data_ptr<int>(), (int)V,
                           reinterpret_cast<uint16_t*>(S_tok.data_ptr()), S64.data_ptr<double>(), st);
    stamp(STAMP_BWD_TOKSUM, st);
  }

  // main: d_emb = S W_ie (+ grad event 1)
  void emb_grad() {
    if (knobs().demb_tuned && d_emb.is_contiguous() && d_emb.scalar_type() == at::kFloat &&
        S_tok.is_contiguous() && wx.stride(1) == 1)
      gemm_bf16_tuned(d_emb, S_tok, false, wx.narrow(1, 0, E), false, 24);
    else
      at::mm_out(d_emb, S_tok, wx.narrow(1, 0, E), at::kFloat);
    if (grad_ev && emb_direct) record_grad_event(aux.grad_ev[1], st, 1);
  }

  // main: input columns dW_ie = S^T emb: M = 4H, N = E, K = V.  One GEMM puts only
  // (4H / 64) x (E / 64) tiles on the chip with a 10.5k-long K (164 us, ~134
  // TFLOP/s at V = 10,509); a split-K batch over the largest divisor of V up to
  // 8 multiplies the tiles in flight, the partial products summed afterwards
  // (49 us + a ~20 us sum, profiles/r2/kernel_summary_r2_v19.txt).
  // (dW_ie on the second side stream, concurrent with the embedding GEMM:
  // 3.355-3.361 vs 3.342-3.356 ms per step, profiles/r5/tail/ab_wie_*.json)
  void input_dw() {
    int64_t nk = 1;
    for (int64_t g = 8; g >= 2; --g)
      if (V % g == 0 && V / g >= 512) { nk = g; break; }
    at::Tensor dWie = dWx.narrow(1, 0, E);
    if (emb.dim() == 2 && emb.stride(1) == 1 && S_tok.is_contiguous() &&
        wgrad_tn_into(S_tok, H4, emb, emb.stride(0), H4, E, V,
                      slot_map ? dw_slots[0].data_ptr<float>() : dWie.data_ptr<float>(),
                      slot_map ? dw_slots[0].stride(0) : E + H, H4, nullptr, 0, st, nullptr, nullptr,
                      slot_map ? dw_slots[4].data_ptr<int>() : nullptr)) {
      // (hand-written split-K MFMA kernel, kernels/wgrad.hip; with direct slots
      // the rows land in W_ih's token columns in PyTorch gate order)
      ie_in_slot = slot_map;
    } else if (nk > 1 && emb.is_contiguous())
      at::sum_out(dWie,
                  at::bmm(S_tok.view({nk, V / nk, H4}).transpose(1, 2), emb.view({nk, V / nk, E}),
                          at::kFloat),
                  0);
    else
      dWie.copy_(at::mm(S_tok.t(), emb, at::kFloat));
    stamp(STAMP_BWD_TOKGEMM, st);
    if (slot_direct && !ie_in_slot)  // (a shape outside the kernel: gather + copy)
      dw_slots[0].narrow(1, 0, E).copy_(dWx.narrow(1, 0, E).index_select(0, dw_slots[2]));
    if (vg_direct) {
      // W_ih's token columns are in the slot (above) and, from the second side
      // stream, its video columns and the FeatPool gradients: slice 2 is final
      (void)hipStreamWaitEvent(st, ev(EV_DVG_DONE), 0);
      if (grad_ev) record_grad_event(aux.grad_ev[2], st, 2);
    }
  }

  // main: joins the second side stream (dvg / dGv), reduces the attention partials
  // and lists the results (the schedule then joins side; upper_dw appends its own)
  std::vector<at::Tensor> collect() {
    at::Tensor dh0;
    if (has_s0)  // step 0's recurrent input h0: dh0 = dG_0 W_hh
      dh0 = at::mm(dG2.narrow(0, 0, R), wx.narrow(1, E, H), at::kFloat);
    std::vector<at::Tensor> res;
    if (!has_att) {
      (void)hipStreamWaitEvent(st, ev(EV_DVG_DONE), 0);  // dvg (second side stream)
    } else {
      // dGv[b, c] = sum_{t, rows of b} alpha[t, r, c] dG_t[r] (kernels/attention.hip:
      // one pass over the bf16 dG rows, partials per step chunk)
      at::Tensor dGv;
      if (C <= 8) {  // (computed on the side stream after the loop)
        (void)hipStreamWaitEvent(st, ev(EV_DGV_DONE), 0);
        dGv = dGv_side;
      } else {  // one batched GEMM per (step, video), K = rows per video
        at::Tensor al =
            ao.alpha_all.to(at::kBFloat16).view({n_steps * Bv, vdiv, C}).transpose(1, 2);
        at::Tensor dgv = dG_all.view({n_steps * Bv, vdiv, KD}).narrow(2, 0, H4);
        dGv = at::bmm(al, dgv, at::kFloat).view({n_steps, Bv, C, H4}).sum(0);
      }
      if (att_mfma) {
        res = {dGv, dpre_part, dwa_part.sum(0).view_as(ao.wa), dba_part.sum(0).view({1}), dWq};
      } else {
        const int64_t ng = att_groups((int)vdiv);
        res = {dGv, dpre_part.view({Bv, ng, C, A}).sum(1), dwa_part.sum(0).view_as(ao.wa),
               dba_part.sum(0).view({NWA}), dWq};
      }
    }
    stamp(STAMP_BWD_END, st);
    std::vector<at::Tensor> out = {dWx, dWlog, dblog, d_emb, dvg};
    out.insert(out.end(), res.begin(), res.end());
    if (has_s0) {
      out.push_back(dh0);
      out.push_back(dc);  // carry into step -1 (LSTM: dc0; GRU / RNN: direct dh0 term)
    }
    return out;
  }

  // main: the upper layers' dW_l = dG_l^T [hd_{l-1, t} | h_{l, t-1}], appended to out
  void upper_dw(std::vector<at::Tensor>& out) {
    for (int64_t l = 1; l < NL; ++l) {
      at::Tensor dWu = at::empty({H4, 2 * H}, f32);
      at::Tensor dGl = dG_up[l].view({NR, H4});
      dWu.narrow(1, 0, H).copy_(grouped_wgrad(dGl, upw(l, 4).reshape({NR, H}), n_steps));
      if (n_steps > 1)
        dWu.narrow(1, H, H).copy_(grouped_wgrad(
            dGl.narrow(0, R, (n_steps - 1) * R),
            upw(l, 1).narrow(0, 0, n_steps - 1).reshape({(n_steps - 1) * R, H}), n_steps - 1));
      else
        dWu.narrow(1, H, H).zero_();
      out.push_back(dWu);
    }
  }
};

}  // namespace

// Returns {dWx_packed (4H, E+H), dWlog (V, H), dblog (V), d_emb (V, E), d_vgate (R / vgate_div, 4H)}
// (+ {dGv (Bv, C, 4H), dP (Bv, C, A), dw_a (A), db_a (1), dW_q (A, H)} with attention,
// att = {Gv, P, W_q bf16, w_a, alpha_all (n, R, C), q_all (n, R, A)}; dvg_rows empty)
// (+ {dh0 (R, H) through W_hh, dc0 (R, H) the state carry} with an initial
// state, state0 = {h0, c0} of the forward)
// (+ {dW_up_l (4H, 2H) packed [W_ih | W_hh]} per upper layer; up = {[W_ih |
// W_hh] bf16, h_all, c_all, gates_all of layer l, hd_all of layer l-1} each).
// toks: (n_steps*R) input token of every (step, row), step-major.
//
// Schedule (streams):
//   side 0 : row weights alpha and the one-hot terms folded into E (dS =
//            diag(alpha) E'), X = E' W_logit (one BLAS GEMM over all T*R
//            rows), then (under the loop) the scaled rows alpha Hd;
//   main   : the input-token counting sort (under the side stream's GEMM),
//            then waits for X and runs the reverse LSTM loop (one fused
//            kernel per step: recurrent GEMM + cell backward; dHd = alpha X
//            row-scaled as the step loads it), then the per-token
//            gate-gradient sums, the embedding / input-weight gradient GEMMs
//            over them and the batched recurrent-weight GEMMs;
//   side 0 : dW_logit = E'^T (alpha Hd) and the bias column sums -- after
//            the loop on one GPU, concurrently with the loop under data
//            parallelism so the vocab head's all-reduce (comm_stream waits
//            on it) hides under the loop.
// vg_bwd (concat model with direct gradient slots): the video-gate / FeatPool
// backward done HERE instead of after the call, so W_ih's and the FeatPool
// parameters' gradients are final shortly after the reverse loop (a third
// early all-reduce slice, grad event 2):
//   {dst_ie, dst_hh (int64 row maps), W_ih slot (4H x (E + Fv)), W_hh slot
//    (4H x H), packed W_iv shadow (bf16), fc (FeatPool output, B x Fv),
//    FeatPool weight slots x vg_nf, bias slots x vg_nf, inputs x vg_nf,
//    weights x vg_nf(, fc as bf16: the forward's side output)}; vg_p the
//    FeatPool dropout.  The packed -> PyTorch row order of layer 0's weight
//    gradients: dw_slots (the weight-gradient reduce's row map).
std::vector<at::Tensor> decoder_backward(at::Tensor wx, at::Tensor wlog, at::Tensor emb,
                                         at::Tensor lse, at::Tensor logits16,
                                         at::Tensor hdrop_all, at::Tensor gates_all,
                                         at::Tensor c_all, at::Tensor h_all, at::Tensor seq,
                                         at::Tensor labels, at::Tensor toks, at::Tensor dg_sel,
                                         at::Tensor dg_xe, double drop_p, at::Tensor rng,
                                         at::Tensor out_wlog, at::Tensor out_blog,
                                         int64_t comm_stream, std::vector<at::Tensor> att,
                                         at::Tensor out_emb, at::Tensor ds_bias, int64_t cell,
                                         std::vector<at::Tensor> state0,
                                         std::vector<at::Tensor> up, at::Tensor blog,
                                         at::Tensor fix_total, int64_t vgate_div,
                                         at::Tensor xw, std::vector<at::Tensor> vg_bwd,
                                         int64_t vg_nf, double vg_p, int64_t x_wait,
                                         bool exp_zero_off, std::vector<at::Tensor> dw_slots,
                                         c10::optional<at::Tensor> vg_idx, int64_t vg_C,
                                         double ls_eps, c10::optional<at::Tensor> ls_wbar) {
  Backward b(BwdArgs{wx, wlog, emb, lse, logits16, hdrop_all, gates_all, c_all, h_all, seq, labels,
                     toks, dg_sel, dg_xe, drop_p, rng, out_wlog, out_blog, comm_stream, att, out_emb,
                     ds_bias, cell, state0, up, blog, fix_total, vgate_div, xw, vg_bwd, vg_nf, vg_p,
                     x_wait, exp_zero_off, dw_slots, vg_idx, vg_C, ls_eps, ls_wbar});
  const hipStream_t st = b.st, side = b.side.stream(), side2 = b.side2.stream();

  // main: operands; side2: the token sort, under X and the loop
  b.prepare_operands();
  fork(b.ev(EV_PRE_X), st, side2);
  b.token_sort();
  if (x_wait != 0) (void)hipStreamWaitEvent(st, reinterpret_cast<hipEvent_t>(x_wait), 0);
  stamp(STAMP_BWD_BEGIN, st);
  if (b.oh_main) {
    b.onehot_pass(st);
    stamp(STAMP_BWD_DHD0, st);
  }
  // side: the vocab head  (the side stream's dW work held back until the first 1 / 2 reverse steps
  // are enqueued, so they do not share the CUs with the GEMM's first wave,
  // measured slower: 3.462-3.489 ms per step, profiles/r5/tail/ab_ohm_d*.json)
  fork(b.ev(EV_ROWS_READY), st, side);
  {
    c10::hip::HIPStreamGuard guard(b.side);
    if (!b.ds_ready && !b.oh_main) b.onehot_pass(side);
    b.x_chunks();
    if (b.dw_start == DW_UNDER_LOOP)
      b.vocab_head_dw();
    else if (!b.ds_ready)
      b.scaled_rows();
  }
  // 4. main: the reverse LSTM loop
  b.prepare_loop();
  if (b.persistent) {
    b.loop_persistent();
    if (b.dw_start == DW_AFTER_LOOP) b.fork_vocab_head_dw();
  } else {
    b.loop_per_step();
  }
  if (b.att_fuse) b.att_bwd_mfma_step(0);  // (step 0's has no launch to ride in)
  stamp(STAMP_BWD_LOOP, st);
  // side2: what needs only the finished dG rows, under the post-loop chain
  if (b.has_att && b.C <= 8) b.att_dgv();
  if (!b.has_att) b.video_gate_grads();
  // side: the recurrent-weight gradients, concurrent with the input-token chain
  b.alloc_weight_grads();
  fork(b.ev(EV_DG_ROWS), st, side);  // the loop's dG rows
  {
    c10::hip::HIPStreamGuard guard(b.side);
    b.recurrent_dw();
  }
  // main: the input-token chain
  b.token_sums();
  if (b.dw_start == DW_AFTER_TOKSUM) b.fork_vocab_head_dw();
  b.emb_grad();
  if (b.dw_start == DW_AFTER_DEMB) b.fork_vocab_head_dw();
  b.input_dw();
  std::vector<at::Tensor> out = b.collect();  // (joins side2)
  // (The bias column sums at the end of the main chain, which ends ~0.3 ms
  // before the side stream's in step_timeline_r2_v20.txt, measured slower:
  // 3.86-3.88 vs 3.76-3.86 ms, they contend with the dW_logit GEMM;
  // profiles/r2/ab_colsum_main.txt.)
  // join the side stream (dW_logit, dW_hh): every tensor a side stream touched
  // is a member of `b`, released after this point
  (void)hipStreamWaitEvent(st, b.ev(EV_SIDE_DONE), 0);
  b.upper_dw(out);
  return out;
}

}  // namespace cst
