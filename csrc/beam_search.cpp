// beam_search: batched beam search of the decoder executor.
#include "engine_internal.h"

namespace cst {

// Batched beam search (reference sample_beam, model.py:369-512) for B videos
// x K beams, entirely on the GPU: per step one LSTM launch (h/c of each row's
// parent beam via row_map), one vocab launch (fp32 logits + LSE partials),
// the LSE combine, a top-K launch and one beam-step launch.  Returns
// {best_seq (B, T) int64, best_logprobs (B, T) fp32}, T = seq_length,
// padded with zeros like the reference.
std::vector<at::Tensor> beam_search(at::Tensor wx, at::Tensor ptab, at::Tensor whh,
                                    at::Tensor wlog, at::Tensor blog, at::Tensor vgate,
                                    int64_t K, int64_t T, int64_t bos_index,
                                    std::vector<at::Tensor> att, int64_t cell,
                                    std::vector<at::Tensor> state0, std::vector<at::Tensor> up) {
  check_cuda(wx, "wx");
  check_cuda(vgate, "vgate");
  TORCH_CHECK(K >= 1 && K <= 16, "beam_size must be in [1, 16]");
  const int64_t H4 = wx.size(0), H = H4 / 4, V = wlog.size(0), B = vgate.size(0), R = B * K;
  TORCH_CHECK(K <= V, "beam_size > vocab_size");
  // temporal attention: att = {Gv, P, W_q, w_a, b_a} as in decoder_forward; the
  // query of a beam row comes from its parent's h (q rows gathered by parent)
  const AttOperands ao = AttOperands::parse(att, Site::Beam, H, R, K, 0);
  const bool has_att = ao.on;
  const int64_t C = ao.C, A = ao.A;
  const int per_frame = ao.per_frame, CPAD = ao.CPAD;
  at::Tensor vg_rows, qb;
  auto dev = wx.device();
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  auto i64 = at::TensorOptions().dtype(at::kLong).device(dev);
  auto i32 = at::TensorOptions().dtype(at::kInt).device(dev);
  hipStream_t st = cur_stream();
  const int64_t ldl = (V + 7) / 8 * 8;
  const int n_vt = vocab_num_tiles((int)V);
  // K <= 8: the vocab launch keeps each tile's K best logits per row (VF_TOPK)
  // and the top-K merges n_vt * K candidates -- no R x V fp32 logits
  const bool tile_topk = K <= 8;
  at::Tensor logits = tile_topk ? at::empty({(int64_t)n_vt * R * K * 2}, f32) : at::empty({R, ldl}, f32);
  at::Tensor lse = at::empty({R}, f32);
  at::Tensor part = at::empty({(int64_t)n_vt * R * vocab_partial_bytes() / 4}, f32);
  at::Tensor top_v = at::empty({R, K}, f32);
  at::Tensor top_i = at::empty({R, K}, i32);
  at::Tensor beam_sum = at::zeros({R}, f32);
  at::Tensor seq_hist = at::zeros({2, R, T}, i64);
  at::Tensor lp_hist = at::zeros({2, R, T}, f32);
  at::Tensor best_ppl = at::full({B}, INFINITY, f32);
  at::Tensor best_seq = at::zeros({B, T}, i64);
  at::Tensor best_lp = at::zeros({B, T}, f32);
  at::Tensor tok = at::full({R}, bos_index, i64);
  at::Tensor parent = at::empty({R}, i32);
  // stacked layers: up = {[W_ih | W_hh] (4H, 2H), W_hh (4H, H)} per upper layer
  const UpperLayers upl = UpperLayers::parse(up, Site::Beam, has_att, !state0.empty(), H, 0);
  const int64_t NL = upl.NL;
  std::vector<std::array<at::Tensor, 2>> hl(NL), cl(NL);
  for (int64_t l = 0; l < NL; ++l) {
    hl[l] = {at::zeros({R, H}, wx.options()), at::empty({R, H}, wx.options())};
    cl[l] = {at::zeros({R, H}, f32), at::empty({R, H}, f32)};
  }
  at::Tensor xin = NL > 1 ? at::empty({R, H4}, f32) : at::Tensor();
  at::Tensor* h = hl[0].data();
  at::Tensor* c = cl[0].data();
  const InitState s0 = InitState::parse(state0, Site::Beam, has_att, B, H);
  if (s0.on) {  // per-video initial state {h0 (B, H), c0 (B, H)}, one copy per beam
    h[0].copy_(s0.h0.repeat_interleave(K, 0));
    c[0].copy_(s0.c0.repeat_interleave(K, 0));
  }
  const uint16_t* W = reinterpret_cast<const uint16_t*>(wlog.data_ptr());
  const uint16_t* WHH = reinterpret_cast<const uint16_t*>(whh.data_ptr());
  // (MFMA attention for the beam rows -- parent-gathered query input, the
  // decode launch's attention workgroups on their own -- measured slower,
  // 26.0k vs 29.6k videos/s at att8 beam 5, profiles/r4/README_r4.md)
  if (has_att) {
    vg_rows = at::empty({R, H4}, f32);
    qb = at::empty({R, A}, f32);
  }
  // Fused form (one layer, no attention, K <= 8): per decode step TWO launches
  // -- the vocab launch (tile top-K candidates + partials) carrying the NEXT
  // step's recurrent GEMM pre = h W_hh^T + video gates for every current row,
  // then beam_fused_step_kernel (LSE, candidate top-K, selection / fork /
  // harvest, and the cell of the new beams from their parents' pre and c) --
  // instead of five (vocab, combine, top-K merge, beam step, LSTM step).
  // With temporal attention (MFMA shape) the vocab launch also carries the
  // attention workgroups: every current row's next video gates (bf16) from
  // its own h_t, which the fused step adds for the parent like pre.
  const bool att_fused = has_att && !per_frame && att_mfma_ok((int)K, (int)C, (int)A, (int)H, 0);
  if (tile_topk && NL == 1 && (!has_att || att_fused)) {
    at::Tensor pre = at::empty({R, H4}, f32);
    const float* VG = has_att ? nullptr : vgate.data_ptr<float>();
    at::Tensor gv16, vg16, att_ep, att_cnt;
    if (has_att) {
      gv16 = at::zeros({B, H4, CPAD}, wx.options());  // frame-minor, frames zero-padded
      gv16.narrow(2, 0, C).copy_(ao.gv.transpose(1, 2));
      vg16 = at::empty({R, H4}, wx.options());
      att_ep = at::empty({B, A / 64, 32, CPAD}, f32);
      att_cnt = at::zeros({B}, at::TensorOptions().dtype(at::kInt).device(wx.device()));
      // step 0 (q = 0): the VALU scorer's fp32 video gates of every row
      launch_att_fwd(ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(), nullptr, nullptr,
                     ao.wa.data_ptr<float>(), ao.ba.data_ptr<float>(), (int)B, (int)K, (int)C,
                     (int)A, (int)H4, vg_rows.data_ptr<float>(), nullptr, st, 0, per_frame);
    }
    // step 0: every row's cell from the initial state and BOS
    launch_lstm_step_fwd(tok.data_ptr<int64_t>(), 1, reinterpret_cast<const uint16_t*>(ptab.data_ptr()),
                         reinterpret_cast<const uint16_t*>(h[0].data_ptr()), c[0].data_ptr<float>(),
                         has_att ? vg_rows.data_ptr<float>() : VG, has_att ? 1 : (int)K, (int)R,
                         (int)H, WHH,
                         reinterpret_cast<uint16_t*>(h[1].data_ptr()), c[1].data_ptr<float>(),
                         nullptr, (int)H, 0.f, nullptr, 0, nullptr, st, nullptr, (int)cell);
    for (int64_t t = 1; t < T - 1; ++t) {
      // vocab projection of h_t (rows = beams of step t) + pre_{t+1} of every row
      const at::Tensor& ht = h[t & 1];
      const bool next = t < T - 2;
      AttMfmaArgs am{};
      if (has_att && next)
        am = AttMfmaArgs{reinterpret_cast<const uint16_t*>(ht.data_ptr()),
                         reinterpret_cast<const uint16_t*>(ao.wq.data_ptr()),
                         ao.pre.data_ptr<float>(), ao.wa.data_ptr<float>(),
                         ao.ba.data_ptr<float>(), reinterpret_cast<const uint16_t*>(gv16.data_ptr()),
                         (int)H, (int)A, (int)C, CPAD, (int)H4, (int)K, (int)B,
                         reinterpret_cast<uint16_t*>(vg16.data_ptr()), nullptr, nullptr,
                         att_ep.data_ptr<float>(), att_cnt.data_ptr<int>()};
      if (has_att && next) am.whole = att_mfma_whole_default((int)C, (int)H);
      (void)launch_vocab_lstm_fwd(reinterpret_cast<const uint16_t*>(ht.data_ptr()), (int)H, (int)R,
                                  (int)H, W, blog.data_ptr<float>(), (int)V,
                                  reinterpret_cast<uint16_t*>(logits.data_ptr()), ldl,
                                  part.data_ptr(), nullptr, 0, VF_TOPK_H | ((int)K << 8), 1.f,
                                  nullptr, (int)t, reinterpret_cast<const uint16_t*>(ht.data_ptr()),
                                  WHH, VG, (int)K, next ? pre.data_ptr<float>() : nullptr, st, 0,
                                  nullptr, nullptr, has_att && next ? &am : nullptr);
      BeamFusedArgs ba{reinterpret_cast<const VocabPartial*>(part.data_ptr()),
                       reinterpret_cast<const float2*>(logits.data_ptr()), n_vt, (int)R, (int)K,
                       (int)B, (int)T, beam_sum.data_ptr<float>(), seq_hist.data_ptr<int64_t>(),
                       lp_hist.data_ptr<float>(), best_ppl.data_ptr<float>(),
                       best_seq.data_ptr<int64_t>(), best_lp.data_ptr<float>(),
                       tok.data_ptr<int64_t>(), next ? pre.data_ptr<float>() : nullptr,
                       reinterpret_cast<const uint16_t*>(ptab.data_ptr()), c[t & 1].data_ptr<float>(),
                       c[(t + 1) & 1].data_ptr<float>(),
                       reinterpret_cast<uint16_t*>(h[(t + 1) & 1].data_ptr()), (int)H, (int)cell,
                       has_att && next ? reinterpret_cast<const uint16_t*>(vg16.data_ptr())
                                       : nullptr};
      launch_beam_fused_step(ba, (int)t, st);
    }
    return {best_seq, best_lp};
  }
  for (int64_t t = 0; t < T - 1; ++t) {
    if (t >= 1) {
      if (tile_topk)
        launch_beam_topk_cand(logits.data_ptr(), n_vt, (int)R, (int)K, lse.data_ptr<float>(),
                              top_v.data_ptr<float>(), top_i.data_ptr<int>(), st);
      else
        launch_beam_topk(logits.data_ptr<float>(), ldl, (int)V, (int)R, (int)K,
                         lse.data_ptr<float>(), top_v.data_ptr<float>(), top_i.data_ptr<int>(),
                         st);
      launch_beam_step(top_v.data_ptr<float>(), top_i.data_ptr<int>(), (int)B, (int)K, (int)T,
                       (int)t, beam_sum.data_ptr<float>(), seq_hist.data_ptr<int64_t>(),
                       lp_hist.data_ptr<float>(), best_ppl.data_ptr<float>(),
                       best_seq.data_ptr<int64_t>(), best_lp.data_ptr<float>(),
                       tok.data_ptr<int64_t>(), parent.data_ptr<int>(), st);
      if (t == T - 2) break;  // the reference's last LSTM step feeds nothing
    }
    const at::Tensor& hp = h[t & 1];
    const at::Tensor& cp = c[t & 1];
    at::Tensor& ho = h[(t + 1) & 1];
    at::Tensor& co = c[(t + 1) & 1];
    if (has_att) {
      if (t >= 1) at::mm_out(qb, hp, ao.wq.t(), at::kFloat);
      launch_att_fwd(ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(),
                     t >= 1 ? qb.data_ptr<float>() : nullptr, t >= 1 ? parent.data_ptr<int>() : nullptr,
                     ao.wa.data_ptr<float>(), ao.ba.data_ptr<float>(), (int)B, (int)K, (int)C,
                     (int)A, (int)H4, vg_rows.data_ptr<float>(), nullptr, st, 0, per_frame);
    }
    launch_lstm_step_fwd(tok.data_ptr<int64_t>(), 1, reinterpret_cast<const uint16_t*>(ptab.data_ptr()),
                         reinterpret_cast<const uint16_t*>(hp.data_ptr()), cp.data_ptr<float>(),
                         has_att ? vg_rows.data_ptr<float>() : vgate.data_ptr<float>(),
                         has_att ? 1 : (int)K, (int)R, (int)H, WHH,
                         reinterpret_cast<uint16_t*>(ho.data_ptr()), co.data_ptr<float>(), nullptr,
                         (int)H, 0.f, nullptr, (int)t, nullptr, st,
                         t >= 1 ? parent.data_ptr<int>() : nullptr, (int)cell);
    for (int64_t l = 1; l < NL; ++l) {  // upper layers: their state follows the parent beam too
      at::mm_out(xin, hl[l - 1][(t + 1) & 1], upl(l, 0).narrow(1, 0, H).t(), at::kFloat);
      launch_lstm_step_fwd(nullptr, 0, nullptr,
                           reinterpret_cast<const uint16_t*>(hl[l][t & 1].data_ptr()),
                           cl[l][t & 1].data_ptr<float>(), xin.data_ptr<float>(), 1, (int)R,
                           (int)H, reinterpret_cast<const uint16_t*>(upl(l, 1).data_ptr()),
                           reinterpret_cast<uint16_t*>(hl[l][(t + 1) & 1].data_ptr()),
                           cl[l][(t + 1) & 1].data_ptr<float>(), nullptr, (int)H, 0.f, nullptr,
                           (int)t, nullptr, st, t >= 1 ? parent.data_ptr<int>() : nullptr,
                           (int)cell);
    }
    const at::Tensor& htop = hl[NL - 1][(t + 1) & 1];
    launch_vocab_fwd(reinterpret_cast<const uint16_t*>(htop.data_ptr()), (int)H, (int)R, (int)H, W,
                     blog.data_ptr<float>(), (int)V,
                     reinterpret_cast<uint16_t*>(logits.data_ptr()), ldl, part.data_ptr(),
                     nullptr, 0, tile_topk ? (VF_TOPK_H | ((int)K << 8)) : /*fp32 logits*/ 8, 1.f,
                     nullptr, (int)t, st);
    launch_vocab_combine(part.data_ptr(), n_vt, (int)R, lse.data_ptr<float>(), nullptr, 0,
                         nullptr, 0, nullptr, 0, nullptr, 0, SEL_GT_H, 0.f, nullptr, (int)t, nullptr,
                         0, nullptr, st);
  }
  return {best_seq, best_lp};
}

}  // namespace cst
