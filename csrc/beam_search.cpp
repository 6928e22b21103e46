// beam_search: batched beam search of the decoder executor, and the truncated
// (top-k / nucleus) sampling decode that shares its general step.
#include "engine_internal.h"

namespace cst {

namespace {

// The rows of one decode chain -- B videos x `rows` rows per video -- and the
// part of a decode step that beam search and truncated sampling share: the
// cell step(s) from the current input tokens (each row's state taken from row
// parent[r] when a parent map is given), attention where present, and the
// vocab launch that leaves each 128-column tile's `ktop` best (logit, index)
// pairs per row (VF_TOPK, ktop <= 8) or the fp32 logits.
struct DecodeRows {
  const at::Tensor &wx, &ptab, &whh, &wlog, &blog, &vgate;
  const int64_t rows, ktop, cell;
  const int64_t H4, H, V, B, R, ldl;
  const int n_vt;
  const bool tile_topk;
  const AttOperands ao;
  const bool has_att;
  const UpperLayers upl;
  const int64_t NL;
  at::TensorOptions f32, i64, i32;
  hipStream_t st;
  at::Tensor logits, lse, part, tok, vg_rows, qb, xin;
  std::vector<std::array<at::Tensor, 2>> hl, cl;

  DecodeRows(const at::Tensor& wx_, const at::Tensor& ptab_, const at::Tensor& whh_,
             const at::Tensor& wlog_, const at::Tensor& blog_, const at::Tensor& vgate_,
             int64_t rows_, int64_t ktop_, int64_t bos_index, const std::vector<at::Tensor>& att,
             int64_t cell_, const std::vector<at::Tensor>& state0,
             const std::vector<at::Tensor>& up, int dense = -1,
             const at::Tensor* shared_tok = nullptr)
      : wx(wx_), ptab(ptab_), whh(whh_), wlog(wlog_), blog(blog_), vgate(vgate_), rows(rows_),
        ktop(ktop_), cell(cell_), H4(wx_.size(0)), H(H4 / 4), V(wlog_.size(0)), B(vgate_.size(0)),
        R(B * rows_), ldl((V + 7) / 8 * 8), n_vt(vocab_num_tiles((int)V)),
        // ktop <= 8: the vocab launch keeps each tile's best logits per row
        // (VF_TOPK) and the selection merges n_vt * ktop candidates -- no R x V
        // fp32 logits; `dense` 0 / 1 says so explicitly (-1: by ktop, as always)
        tile_topk(dense < 0 ? ktop_ <= 8 : dense == 0),
        // temporal attention: att = {Gv, P, W_q, w_a, b_a} as in decoder_forward
        ao(AttOperands::parse(att, Site::Beam, H, R, rows_, 0)), has_att(ao.on),
        // stacked layers: up = {[W_ih | W_hh] (4H, 2H), W_hh (4H, H)} per upper layer
        upl(UpperLayers::parse(up, Site::Beam, has_att, !state0.empty(), H, 0)), NL(upl.NL) {
    auto dev = wx.device();
    f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
    i64 = at::TensorOptions().dtype(at::kLong).device(dev);
    i32 = at::TensorOptions().dtype(at::kInt).device(dev);
    st = cur_stream();
    logits = tile_topk ? at::empty({(int64_t)n_vt * R * ktop * 2}, f32) : at::empty({R, ldl}, f32);
    lse = at::empty({R}, f32);
    part = at::empty({(int64_t)n_vt * R * vocab_partial_bytes() / 4}, f32);
    // the rows' input tokens; shared_tok: another chain's buffer instead (the
    // members of an ensemble all read member 0's)
    tok = shared_tok != nullptr ? *shared_tok : at::full({R}, bos_index, i64);
    hl.resize(NL), cl.resize(NL);
    for (int64_t l = 0; l < NL; ++l) {
      hl[l] = {at::zeros({R, H}, wx.options()), at::empty({R, H}, wx.options())};
      cl[l] = {at::zeros({R, H}, f32), at::empty({R, H}, f32)};
    }
    xin = NL > 1 ? at::empty({R, H4}, f32) : at::Tensor();
    const InitState s0 = InitState::parse(state0, Site::Beam, has_att, B, H);
    if (s0.on) {  // per-video initial state {h0 (B, H), c0 (B, H)}, one copy per row
      hl[0][0].copy_(s0.h0.repeat_interleave(rows, 0));
      cl[0][0].copy_(s0.c0.repeat_interleave(rows, 0));
    }
    if (has_att) {
      vg_rows = at::empty({R, H4}, f32);
      qb = at::empty({R, ao.A}, f32);
    }
  }

  // step t of the chain: state parity t -> t + 1, then the vocab launch on the
  // top layer's new h; `combine`: the row LSE into `lse` as a launch of its own
  void step(int64_t t, const int* parent, bool combine) {
    const uint16_t* W = reinterpret_cast<const uint16_t*>(wlog.data_ptr());
    const uint16_t* WHH = reinterpret_cast<const uint16_t*>(whh.data_ptr());
    const at::Tensor& hp = hl[0][t & 1];
    const at::Tensor& cp = cl[0][t & 1];
    at::Tensor& ho = hl[0][(t + 1) & 1];
    at::Tensor& co = cl[0][(t + 1) & 1];
    if (has_att) {
      if (t >= 1) at::mm_out(qb, hp, ao.wq.t(), at::kFloat);
      launch_att_fwd(ao.gv.data_ptr<float>(), ao.pre.data_ptr<float>(),
                     t >= 1 ? qb.data_ptr<float>() : nullptr, parent,
                     ao.wa.data_ptr<float>(), ao.ba.data_ptr<float>(), (int)B, (int)rows, (int)ao.C,
                     (int)ao.A, (int)H4, vg_rows.data_ptr<float>(), nullptr, st, 0, ao.per_frame);
    }
    launch_lstm_step_fwd(tok.data_ptr<int64_t>(), 1, reinterpret_cast<const uint16_t*>(ptab.data_ptr()),
                         reinterpret_cast<const uint16_t*>(hp.data_ptr()), cp.data_ptr<float>(),
                         has_att ? vg_rows.data_ptr<float>() : vgate.data_ptr<float>(),
                         has_att ? 1 : (int)rows, (int)R, (int)H, WHH,
                         reinterpret_cast<uint16_t*>(ho.data_ptr()), co.data_ptr<float>(), nullptr,
                         (int)H, 0.f, nullptr, (int)t, nullptr, st, parent, (int)cell);
    for (int64_t l = 1; l < NL; ++l) {  // upper layers: their state follows the parent row too
      at::mm_out(xin, hl[l - 1][(t + 1) & 1], upl(l, 0).narrow(1, 0, H).t(), at::kFloat);
      launch_lstm_step_fwd(nullptr, 0, nullptr,
                           reinterpret_cast<const uint16_t*>(hl[l][t & 1].data_ptr()),
                           cl[l][t & 1].data_ptr<float>(), xin.data_ptr<float>(), 1, (int)R,
                           (int)H, reinterpret_cast<const uint16_t*>(upl(l, 1).data_ptr()),
                           reinterpret_cast<uint16_t*>(hl[l][(t + 1) & 1].data_ptr()),
                           cl[l][(t + 1) & 1].data_ptr<float>(), nullptr, (int)H, 0.f, nullptr,
                           (int)t, nullptr, st, parent, (int)cell);
    }
    const at::Tensor& htop = hl[NL - 1][(t + 1) & 1];
    launch_vocab_fwd(reinterpret_cast<const uint16_t*>(htop.data_ptr()), (int)H, (int)R, (int)H, W,
                     blog.data_ptr<float>(), (int)V,
                     reinterpret_cast<uint16_t*>(logits.data_ptr()), ldl, part.data_ptr(),
                     nullptr, 0, tile_topk ? (VF_TOPK_H | ((int)ktop << 8)) : /*fp32 logits*/ 8, 1.f,
                     nullptr, (int)t, st);
    if (combine)
      launch_vocab_combine(part.data_ptr(), n_vt, (int)R, lse.data_ptr<float>(), nullptr, 0,
                           nullptr, 0, nullptr, 0, nullptr, 0, SEL_GT_H, 0.f, nullptr, (int)t,
                           nullptr, 0, nullptr, st);
  }
};

// Truncated sampling decode (CaptionModel.sample with top_k in [1, 8]) for B
// videos x S rows per video with the operands of beam_search: per step the
// cell step(s) -- every row continues its own state, no parent map --,
// attention where present, the VF_TOPK vocab launch with K = top_k and the
// selection launch (kernels/topk_sample.hip: LSE, global top-K, temperature,
// nucleus, draw, end-of-sequence rule).  Three launches per step for a
// one-layer decoder without attention; no host synchronisation and a fixed
// launch count.  rng: int32[2] device seeds, slot 1 keys the draws.  Returns
// {seq (R, T - 2) int64, logprobs (R, T - 2) fp32}, T = seq_length: the
// width of the sampler of decoder_forward, zeros after a row's end.
std::vector<at::Tensor> sample_topk(const at::Tensor& wx, const at::Tensor& ptab,
                                    const at::Tensor& whh, const at::Tensor& wlog,
                                    const at::Tensor& blog, const at::Tensor& vgate,
                                    int64_t top_k, int64_t T, int64_t bos_index,
                                    const std::vector<at::Tensor>& att, int64_t cell,
                                    const std::vector<at::Tensor>& state0,
                                    const std::vector<at::Tensor>& up, int64_t S, double top_p,
                                    double temperature, const at::Tensor& rng) {
  TORCH_CHECK(top_k >= 1 && top_k <= 8, "top_k must be in [1, 8] on the engine");
  TORCH_CHECK(top_k <= wlog.size(0), "top_k > vocab_size");
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "top_p must be in (0, 1]");
  TORCH_CHECK(temperature > 0.0 && std::isfinite(temperature), "temperature must be positive");
  TORCH_CHECK(T >= 3, "seq_length must be at least 3");
  DecodeRows d(wx, ptab, whh, wlog, blog, vgate, S, top_k, bos_index, att, cell, state0, up);
  const int64_t R = d.R, Ts = T - 2;
  at::Tensor seq = at::zeros({R, Ts}, d.i64);
  at::Tensor lp = at::zeros({R, Ts}, d.f32);
  at::Tensor unfinished = at::ones({R}, d.f32.dtype(at::kByte));
  for (int64_t t = 0; t < T - 1; ++t) {
    if (t >= 1) {
      TopkSampleArgs sa{reinterpret_cast<const VocabPartial*>(d.part.data_ptr()),
                        reinterpret_cast<const float2*>(d.logits.data_ptr()), d.n_vt, (int)R,
                        (int)top_k, (int)d.V, (float)top_p, (float)(1.0 / temperature),
                        rng_ptr(rng), (int)t, unfinished.data_ptr<uint8_t>(),
                        seq.data_ptr<int64_t>() + (t - 1), Ts, d.tok.data_ptr<int64_t>(),
                        lp.data_ptr<float>() + (t - 1), Ts, nullptr};
      launch_topk_sample(sa, d.st);
      if (t == T - 2) break;  // the last cell step would feed nothing
    }
    d.step(t, nullptr, /*combine=*/false);
  }
  return {seq, lp};
}

// One member's operands of the ensemble decode, as Python packs them: {wx,
// ptab, whh, wlog, blog, vgate, meta, att.., state0.., up..} with meta a CPU
// int64 tensor {cell, n_att, n_state0, n_up}.
struct MemberPack {
  at::Tensor wx, ptab, whh, wlog, blog, vgate;
  int64_t cell = 0;
  std::vector<at::Tensor> att, state0, up;
  static MemberPack parse(const std::vector<at::Tensor>& p) {
    TORCH_CHECK(p.size() >= 7, "ensemble member: {wx, ptab, whh, wlog, blog, vgate, meta, ...}");
    const at::Tensor& meta = p[6];
    TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.numel() == 4,
                "ensemble member: meta = CPU int64 {cell, n_att, n_state0, n_up}");
    const int64_t* q = meta.data_ptr<int64_t>();
    TORCH_CHECK(q[1] >= 0 && q[2] >= 0 && q[3] >= 0 && (int64_t)p.size() == 7 + q[1] + q[2] + q[3],
                "ensemble member: list length does not match meta");
    MemberPack m{p[0], p[1], p[2], p[3], p[4], p[5], q[0], {}, {}, {}};
    auto it = p.begin() + 7;
    m.att.assign(it, it + q[1]);
    m.state0.assign(it + q[1], it + q[1] + q[2]);
    m.up.assign(it + q[1] + q[2], p.end());
    return m;
  }
};

// Ensemble decoding (models/ensemble.py): M members, each with its own weights
// and state, decode the same B videos in lock-step under the mixture
// lp_ens[v] = logsumexp_m(logw_m + lp_m[v]).  One DecodeRows per member in the
// dense-logits form; per step every member runs its cell(s), attention and
// vocab launch + LSE combine on the shared input tokens and parent map (`tok`
// of member 0 drives them all), one launch_ensemble_topk takes the mixture's
// top-K, and for beam search the unchanged launch_beam_step selects, forks and
// harvests.  Greedy (rows = 1): the top-K launch's epilogue writes the token,
// so no further launch.  Everything runs on the current stream: no host
// synchronisation and no allocation inside the loop, a fixed launch count.
// (Forking the members onto side streams and capturing the decode into a graph
// are out of scope here: the members run back to back.)
// Returns beam: {best_seq (B, T), best_lp (B, T)}; greedy: {seq (B, T - 2), lp}.
std::vector<at::Tensor> ensemble_decode(const std::vector<MemberPack>& mp,
                                        const std::vector<double>& logw, int64_t K, int64_t T,
                                        int64_t bos_index, bool greedy) {
  const int64_t M = (int64_t)mp.size();
  // refused before any launch
  TORCH_CHECK(M >= 1 && M <= ENS_MAXM, "ensemble: 1 to 8 members, got ", M);
  TORCH_CHECK((int64_t)logw.size() == M, "ensemble: ", logw.size(), " log-weights for ", M,
              " members");
  for (double w : logw) TORCH_CHECK(std::isfinite(w), "ensemble: non-finite log-weight");
  if (greedy) K = 1;
  TORCH_CHECK(K >= 1 && K <= 16, "beam_size must be in [1, 16]");
  TORCH_CHECK(T >= 3, "seq_length must be at least 3");
  const int64_t V = mp[0].wlog.size(0), B = mp[0].vgate.size(0);
  TORCH_CHECK(K <= V, "beam_size > vocab_size");
  // frames of a temporal-attention member (w_a (A): one scorer for all frames;
  // MANet's modality blocks are not frames of the input)
  auto frames = [](const MemberPack& m) -> int64_t {
    return m.att.size() == 5 && m.att[3].numel() == m.att[1].size(2) ? m.att[0].size(1) : 0;
  };
  int64_t C = 0;
  for (int64_t m = 0; m < M; ++m) {
    check_cuda(mp[m].wx, "wx");
    check_cuda(mp[m].vgate, "vgate");
    TORCH_CHECK(mp[m].wlog.size(0) == V, "ensemble: member ", m, " has vocab_size ",
                mp[m].wlog.size(0), ", member 0 has ", V);
    TORCH_CHECK(mp[m].vgate.size(0) == B, "ensemble: member ", m, " decodes ", mp[m].vgate.size(0),
                " videos, member 0 decodes ", B);
    const int64_t c = frames(mp[m]);
    TORCH_CHECK(c == 0 || C == 0 || c == C, "ensemble: member ", m, " attends over ", c,
                " frames, an earlier member over ", C);
    if (c) C = c;
  }
  std::vector<std::unique_ptr<DecodeRows>> d;
  for (int64_t m = 0; m < M; ++m) {
    const MemberPack& p = mp[m];
    d.emplace_back(new DecodeRows(p.wx, p.ptab, p.whh, p.wlog, p.blog, p.vgate, K, K, bos_index,
                                  p.att, p.cell, p.state0, p.up, /*dense=*/1,
                                  /*shared_tok=*/m > 0 ? &d[0]->tok : nullptr));
  }
  DecodeRows& d0 = *d[0];
  const int64_t R = d0.R;
  hipStream_t st = d0.st;
  EnsembleTopkArgs ea{};
  for (int64_t m = 0; m < M; ++m) {
    ea.logits[m] = d[m]->logits.data_ptr<float>();
    ea.ldl[m] = d[m]->ldl;
    ea.lse[m] = d[m]->lse.data_ptr<float>();
    ea.logw[m] = (float)logw[m];
  }
  ea.M = (int)M, ea.V = (int)V, ea.R = (int)R, ea.K = (int)K;
  if (greedy) {
    const int64_t Ts = T - 2;
    at::Tensor seq = at::zeros({R, Ts}, d0.i64);
    at::Tensor lp = at::zeros({R, Ts}, d0.f32);
    at::Tensor unfinished = at::ones({R}, d0.f32.dtype(at::kByte));
    ea.unfinished = unfinished.data_ptr<uint8_t>();
    ea.out_stride = Ts;
    ea.next_tok = d0.tok.data_ptr<int64_t>();
    for (int64_t t = 0; t < T - 1; ++t) {
      if (t >= 1) {
        ea.seq_out = seq.data_ptr<int64_t>() + (t - 1);
        ea.lp_out = lp.data_ptr<float>() + (t - 1);
        launch_ensemble_topk(ea, st);
        if (t == T - 2) break;  // the last cell step would feed nothing
      }
      for (auto& dm : d) dm->step(t, nullptr, /*combine=*/true);
    }
    return {seq, lp};
  }
  at::Tensor top_v = at::empty({R, K}, d0.f32);
  at::Tensor top_i = at::empty({R, K}, d0.i32);
  at::Tensor beam_sum = at::zeros({R}, d0.f32);
  at::Tensor seq_hist = at::zeros({2, R, T}, d0.i64);
  at::Tensor lp_hist = at::zeros({2, R, T}, d0.f32);
  at::Tensor best_ppl = at::full({B}, INFINITY, d0.f32);
  at::Tensor best_seq = at::zeros({B, T}, d0.i64);
  at::Tensor best_lp = at::zeros({B, T}, d0.f32);
  at::Tensor parent = at::empty({R}, d0.i32);
  ea.top_v = top_v.data_ptr<float>();
  ea.top_i = top_i.data_ptr<int>();
  for (int64_t t = 0; t < T - 1; ++t) {
    if (t >= 1) {
      launch_ensemble_topk(ea, st);
      launch_beam_step(top_v.data_ptr<float>(), top_i.data_ptr<int>(), (int)B, (int)K, (int)T,
                       (int)t, beam_sum.data_ptr<float>(), seq_hist.data_ptr<int64_t>(),
                       lp_hist.data_ptr<float>(), best_ppl.data_ptr<float>(),
                       best_seq.data_ptr<int64_t>(), best_lp.data_ptr<float>(),
                       d0.tok.data_ptr<int64_t>(), parent.data_ptr<int>(), st);
      if (t == T - 2) break;  // the reference's last LSTM step feeds nothing
    }
    for (auto& dm : d) dm->step(t, t >= 1 ? parent.data_ptr<int>() : nullptr, /*combine=*/true);
  }
  return {best_seq, best_lp};
}

}  // namespace

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
                                    std::vector<at::Tensor> state0, std::vector<at::Tensor> up,
                                    int64_t rows_per_video, double top_p, double temperature,
                                    c10::optional<at::Tensor> rng,
                                    std::vector<std::vector<at::Tensor>> ensemble,
                                    std::vector<double> ens_weights, bool ens_greedy) {
  if (!ens_weights.empty()) {
    // ensemble decoding: this call's operands are member 0, `ensemble` holds the
    // packs of members 1..M-1, ens_weights the M log-weights (host)
    TORCH_CHECK(rows_per_video == 0, "ensemble: no truncated sampling");
    TORCH_CHECK(ensemble.size() + 1 <= (size_t)ENS_MAXM, "ensemble: 1 to 8 members, got ",
                ensemble.size() + 1);
    std::vector<MemberPack> mp;
    mp.push_back(MemberPack{wx, ptab, whh, wlog, blog, vgate, cell, att, state0, up});
    for (const auto& p : ensemble) mp.push_back(MemberPack::parse(p));
    return ensemble_decode(mp, ens_weights, K, T, bos_index, ens_greedy);
  }
  TORCH_CHECK(ensemble.empty() && !ens_greedy, "ensemble operands need ens_weights");
  check_cuda(wx, "wx");
  check_cuda(vgate, "vgate");
  if (rows_per_video > 0)  // the truncated sampling decode: K is top_k
    return sample_topk(wx, ptab, whh, wlog, blog, vgate, K, T, bos_index, att, cell, state0, up,
                       rows_per_video, top_p, temperature, rng.has_value() ? *rng : at::Tensor());
  TORCH_CHECK(K >= 1 && K <= 16, "beam_size must be in [1, 16]");
  const int64_t H4 = wx.size(0), H = H4 / 4, V = wlog.size(0), B = vgate.size(0), R = B * K;
  TORCH_CHECK(K <= V, "beam_size > vocab_size");
  // the query of a beam row comes from its parent's h (q rows gathered by parent)
  DecodeRows d(wx, ptab, whh, wlog, blog, vgate, K, K, bos_index, att, cell, state0, up);
  const AttOperands& ao = d.ao;
  const bool has_att = ao.on;
  const int64_t C = ao.C, A = ao.A;
  const int per_frame = ao.per_frame, CPAD = ao.CPAD;
  at::Tensor& vg_rows = d.vg_rows;
  const at::TensorOptions f32 = d.f32, i64 = d.i64, i32 = d.i32;
  hipStream_t st = d.st;
  const int64_t ldl = d.ldl;
  const int n_vt = d.n_vt;
  const bool tile_topk = d.tile_topk;
  at::Tensor &logits = d.logits, &lse = d.lse, &part = d.part, &tok = d.tok;
  at::Tensor top_v = at::empty({R, K}, f32);
  at::Tensor top_i = at::empty({R, K}, i32);
  at::Tensor beam_sum = at::zeros({R}, f32);
  at::Tensor seq_hist = at::zeros({2, R, T}, i64);
  at::Tensor lp_hist = at::zeros({2, R, T}, f32);
  at::Tensor best_ppl = at::full({B}, INFINITY, f32);
  at::Tensor best_seq = at::zeros({B, T}, i64);
  at::Tensor best_lp = at::zeros({B, T}, f32);
  at::Tensor parent = at::empty({R}, i32);
  const int64_t NL = d.NL;
  at::Tensor* h = d.hl[0].data();
  at::Tensor* c = d.cl[0].data();
  const uint16_t* W = reinterpret_cast<const uint16_t*>(wlog.data_ptr());
  const uint16_t* WHH = reinterpret_cast<const uint16_t*>(whh.data_ptr());
  // (MFMA attention for the beam rows -- parent-gathered query input, the
  // decode launch's attention workgroups on their own -- measured slower,
  // 26.0k vs 29.6k videos/s at att8 beam 5, profiles/r4/README_r4.md)
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
    d.step(t, t >= 1 ? parent.data_ptr<int>() : nullptr, /*combine=*/true);
  }
  return {best_seq, best_lp};
}

}  // namespace cst
