// Around the decoder: FeatPool, the losses, the metric scorers, the flat Adam step.
#include "engine_internal.h"

namespace cst {

// FeatPool (csrc/kernels/featpool.hip): xs[f] (rows, d_f), ws[f] (H, d_f),
// bs[f] (H), all fp32 contiguous GPU tensors; returns the concatenated
// (rows, F*H) output after ReLU and dropout (mask from rng slot 0).
// idx (optional, int64 (n)): xs are then the resident tables (table rows * C,
// d_f) and the call covers the rows idx[r / C] * C + r % C, r < n * C.
static FeatPoolArgs featpool_args(const std::vector<at::Tensor>& xs,
                                  const std::vector<at::Tensor>& ws,
                                  const std::vector<at::Tensor>& bs,
                                  const c10::optional<at::Tensor>& idx = c10::nullopt,
                                  int64_t C = 1) {
  TORCH_CHECK(!xs.empty() && xs.size() <= FEATPOOL_MAX_F && ws.size() == xs.size() &&
                  (bs.empty() || bs.size() == xs.size()),
              "featpool: 1..", FEATPOOL_MAX_F, " modalities, one weight (and bias) each");
  FeatPoolArgs a{};
  a.nf = (int)xs.size();
  a.rows = (int)xs[0].size(0);
  a.H = (int)ws[0].size(0);
  const int64_t x_rows = xs[0].size(0);
  if (idx.has_value() && idx->defined()) {
    check_cuda(*idx, "featpool idx");
    TORCH_CHECK(idx->scalar_type() == at::kLong && idx->dim() == 1 && idx->is_contiguous() &&
                    idx->numel() > 0 && C >= 1 && x_rows > 0 && x_rows % C == 0 &&
                    idx->numel() * C < (1LL << 31) && idx->device() == xs[0].device(),
                "featpool: idx int64 (n) on the features' device, tables of (table rows * C) rows");
    a.idx = idx->data_ptr<int64_t>();
    a.C = (int)C;
    a.n_table = (int)(x_rows / C);
    a.rows = (int)(idx->numel() * C);
  }
  TORCH_CHECK(a.H % 64 == 0, "featpool: output size must be a multiple of 64");
  for (int f = 0; f < a.nf; ++f) {
    const at::Tensor &x = xs[f], &w = ws[f];
    // x may be a column slice of a wider row (the loader gathers every
    // modality in one pass): unit column stride, 16-byte-aligned rows
    TORCH_CHECK(x.is_cuda(), "featpool x must be a GPU tensor");
    check_cuda(w, "featpool w");
    TORCH_CHECK(x.scalar_type() == at::kFloat && w.scalar_type() == at::kFloat && x.dim() == 2 &&
                    w.dim() == 2 && x.size(0) == x_rows && w.size(0) == a.H &&
                    x.size(1) == w.size(1) && x.size(1) % 4 == 0 &&
                    (x.size(1) == 1 || x.stride(1) == 1) && x.stride(0) % 4 == 0 &&
                    x.stride(0) >= x.size(1) &&
                    reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
                "featpool: fp32 x (rows, d) with unit column stride and 16-byte-aligned rows, "
                "w (H, d), d % 4 == 0");
    a.s[f].x = x.data_ptr<float>();
    a.s[f].w = w.data_ptr<float>();
    if (!bs.empty()) {
      check_cuda(bs[f], "featpool b");
      TORCH_CHECK(bs[f].scalar_type() == at::kFloat && bs[f].numel() == a.H, "featpool: bias (H)");
      a.s[f].b = bs[f].data_ptr<float>();
    }
    a.s[f].d = (int)x.size(1);
    a.s[f].ld = (int)x.stride(0);
  }
  featpool_layout(a);
  return a;
}

at::Tensor featpool_forward(std::vector<at::Tensor> xs, std::vector<at::Tensor> ws,
                            std::vector<at::Tensor> bs, double drop_p, at::Tensor rng,
                            c10::optional<at::Tensor> idx, int64_t C) {
  TORCH_CHECK(bs.size() == xs.size(), "featpool: one bias per modality");
  FeatPoolArgs a = featpool_args(xs, ws, bs, idx, C);
  auto f32 = xs[0].options();
  at::Tensor wsp = at::empty({(int64_t)a.fwd_blocks * 64 * 64}, f32);
  at::Tensor out = at::empty({a.rows, (int64_t)a.nf * a.H}, f32);
  launch_featpool_fwd(a, wsp.data_ptr<float>(), out.data_ptr<float>(), nullptr, (float)drop_p,
                      rng_ptr(rng), cur_stream());
  return out;
}

// {out fp32 (rows, F*H), out as bf16 (round to nearest even)}: FeatPool for
// the gate GEMM that follows (bf16 operand, no conversion pass)
std::vector<at::Tensor> featpool_forward16(std::vector<at::Tensor> xs, std::vector<at::Tensor> ws,
                                           std::vector<at::Tensor> bs, double drop_p,
                                           at::Tensor rng, c10::optional<at::Tensor> idx,
                                           int64_t C) {
  TORCH_CHECK(bs.size() == xs.size(), "featpool: one bias per modality");
  FeatPoolArgs a = featpool_args(xs, ws, bs, idx, C);
  auto f32 = xs[0].options();
  at::Tensor wsp = at::empty({(int64_t)a.fwd_blocks * 64 * 64}, f32);
  at::Tensor out = at::empty({a.rows, (int64_t)a.nf * a.H}, f32);
  at::Tensor out16 = at::empty({a.rows, (int64_t)a.nf * a.H}, f32.dtype(at::kBFloat16));
  launch_featpool_fwd(a, wsp.data_ptr<float>(), out.data_ptr<float>(),
                      reinterpret_cast<uint16_t*>(out16.data_ptr()), (float)drop_p, rng_ptr(rng),
                      cur_stream());
  return {out, out16};
}

// -> {dW_0 .. dW_{F-1}, db_0 .. db_{F-1}} given dL/d(out) and the forward's out;
// written into `outs` (2F contiguous fp32 tensors, e.g. gradient-bucket
// slots) when given
std::vector<at::Tensor> featpool_backward(at::Tensor dout, at::Tensor out,
                                          std::vector<at::Tensor> xs,
                                          std::vector<at::Tensor> ws, double drop_p,
                                          std::vector<at::Tensor> outs,
                                          c10::optional<at::Tensor> idx, int64_t C) {
  FeatPoolArgs a = featpool_args(xs, ws, {}, idx, C);
  check_cuda(dout, "featpool dout");
  check_cuda(out, "featpool out");
  TORCH_CHECK(dout.scalar_type() == at::kFloat && out.scalar_type() == at::kFloat &&
                  dout.numel() == (int64_t)a.rows * a.nf * a.H && out.numel() == dout.numel(),
              "featpool: dout / out (rows, F*H) fp32");
  std::vector<at::Tensor> res;
  FeatPoolGrads g{};
  if (!outs.empty()) {
    TORCH_CHECK((int)outs.size() == 2 * a.nf, "featpool: outs = {dW_f} + {db_f}");
    for (int f = 0; f < a.nf; ++f) {
      TORCH_CHECK(outs[f].is_cuda() && outs[f].is_contiguous() &&
                      outs[f].scalar_type() == at::kFloat && outs[f].numel() == ws[f].numel() &&
                      outs[a.nf + f].is_cuda() && outs[a.nf + f].is_contiguous() &&
                      outs[a.nf + f].scalar_type() == at::kFloat && outs[a.nf + f].numel() == a.H,
                  "featpool: output slots must be contiguous fp32 (H, d) / (H)");
    }
    res = outs;
  } else {
    for (int f = 0; f < a.nf; ++f) res.push_back(at::empty_like(ws[f]));
    for (int f = 0; f < a.nf; ++f) res.push_back(at::empty({a.H}, ws[f].options()));
  }
  for (int f = 0; f < a.nf; ++f) {
    g.dw[f] = res[f].data_ptr<float>();
    g.db[f] = res[a.nf + f].data_ptr<float>();
  }
  launch_featpool_bwd(a, dout.data_ptr<float>(), out.data_ptr<float>(), (float)drop_p, g,
                      cur_stream());
  return res;
}

// SCST loss (csrc/kernels/loss.hip): seq (R, T) int64, lp (R, T) fp32,
// sample (R), greedy (R or R / gdiv) fp32 -> {loss (0-dim), out = [loss, m, b,
// sum mask], reward (R)}
std::vector<at::Tensor> scst_loss_forward(at::Tensor seq, at::Tensor lp, at::Tensor sample,
                                          at::Tensor greedy) {
  for (auto* t : {&seq, &lp, &sample, &greedy}) check_cuda(*t, "scst_loss operand");
  const int64_t R = seq.size(0), T = seq.size(1);
  TORCH_CHECK(seq.scalar_type() == at::kLong && lp.scalar_type() == at::kFloat &&
                  lp.size(0) == R && lp.size(1) == T && sample.scalar_type() == at::kFloat &&
                  sample.numel() == R && greedy.scalar_type() == at::kFloat &&
                  greedy.numel() > 0 && R % greedy.numel() == 0,
              "scst_loss: seq / lp (R, T), sample (R), greedy (R or R / rows per video)");
  auto f32 = lp.options();
  at::Tensor out = at::empty({4}, f32), reward = at::empty({R}, f32), loss = at::empty({}, f32);
  at::Tensor ws = at::zeros({scst_loss_ws_ints((int)R)}, f32.dtype(at::kInt));
  launch_scst_loss_fwd(seq.data_ptr<int64_t>(), lp.data_ptr<float>(), (int)R, (int)T,
                       sample.data_ptr<float>(), greedy.data_ptr<float>(),
                       (int)(R / greedy.numel()), reward.data_ptr<float>(), out.data_ptr<float>(),
                       loss.data_ptr<float>(), ws.data_ptr<int>(), CstBase{nullptr, 0, 0},
                       cur_stream());
  return {loss, out, reward};
}

// CST loss (the same launch, consensus baseline): scores (R) fp32 of the
// rewarded rows, S rows per video (R % S == 0, S <= 64); bref: (R) GT
// consensus scores (scb_baseline 1) or empty (scb_baseline 2: the scores
// themselves); k = scb_captions (0: reward = score) -> {loss, out, reward}
//
// objective != 0 (--rl_objective: GroupObjective of launchers.h): the group
// loss over each video's S rows instead, bref and k unused -> {loss, out,
// reward, w} with w (R) the row weights scst_loss_backward takes
std::vector<at::Tensor> cst_loss_forward(at::Tensor seq, at::Tensor lp, at::Tensor scores,
                                         at::Tensor bref, int64_t S, int64_t k, int64_t objective,
                                         double alpha, double cost_scale) {
  for (auto* t : {&seq, &lp, &scores}) check_cuda(*t, "cst_loss operand");
  const int64_t R = seq.size(0), T = seq.size(1);
  if (objective != 0) {
    TORCH_CHECK(objective >= GROUP_RISK && objective <= GROUP_MULTI_MARGIN,
                "group_loss: objective 1 (risk), 2 (softmax_margin) or 3 (multi_margin)");
    TORCH_CHECK(seq.dim() == 2 && lp.dim() == 2 && seq.scalar_type() == at::kLong &&
                    lp.scalar_type() == at::kFloat && lp.size(0) == R && lp.size(1) == T &&
                    T >= 1 && scores.scalar_type() == at::kFloat && scores.numel() == R,
                "group_loss: seq / lp (R, T), T >= 1, scores (R) fp32");
    TORCH_CHECK(S >= 2 && S <= 64 && R > 0 && R % S == 0,
                "group_loss: 2 <= S <= 64 rows per video, dividing R (got S = ", S, ", R = ", R,
                ")");
    TORCH_CHECK(std::isfinite(alpha) && alpha > 0 && std::isfinite(cost_scale) && cost_scale >= 0,
                "group_loss: alpha finite and > 0, cost_scale finite and >= 0");
    auto f32 = lp.options();
    at::Tensor out = at::empty({4}, f32), reward = at::empty({R}, f32), loss = at::empty({}, f32);
    at::Tensor w = at::empty({R}, f32);
    at::Tensor ws = at::zeros({group_loss_ws_ints((int)(R / S))}, f32.dtype(at::kInt));
    launch_group_loss_fwd(seq.data_ptr<int64_t>(), lp.data_ptr<float>(), (int)R, (int)T,
                          scores.data_ptr<float>(),
                          GroupObj{(int)objective, (int)S, (float)alpha, (float)cost_scale},
                          reward.data_ptr<float>(), w.data_ptr<float>(), out.data_ptr<float>(),
                          loss.data_ptr<float>(), ws.data_ptr<int>(), cur_stream());
    return {loss, out, reward, w};
  }
  const bool has_ref = bref.defined() && bref.numel() > 0;
  TORCH_CHECK(seq.scalar_type() == at::kLong && lp.scalar_type() == at::kFloat &&
                  lp.size(0) == R && lp.size(1) == T && scores.scalar_type() == at::kFloat &&
                  scores.numel() == R && S >= 1 && S <= 64 && R % S == 0 && k >= 0 && k <= S,
              "cst_loss: seq / lp (R, T), scores (R), 1 <= S <= 64 dividing R, 0 <= k <= S");
  if (has_ref) {
    check_cuda(bref, "cst_loss bref");
    TORCH_CHECK(bref.scalar_type() == at::kFloat && bref.numel() == R, "cst_loss: bref (R) fp32");
  }
  auto f32 = lp.options();
  at::Tensor out = at::empty({4}, f32), reward = at::empty({R}, f32), loss = at::empty({}, f32);
  at::Tensor ws = at::zeros({scst_loss_ws_ints((int)R)}, f32.dtype(at::kInt));
  launch_scst_loss_fwd(seq.data_ptr<int64_t>(), lp.data_ptr<float>(), (int)R, (int)T,
                       scores.data_ptr<float>(), scores.data_ptr<float>(), 1,
                       reward.data_ptr<float>(), out.data_ptr<float>(), loss.data_ptr<float>(),
                       ws.data_ptr<int>(),
                       CstBase{has_ref ? bref.data_ptr<float>() : nullptr, (int)S, (int)k},
                       cur_stream());
  return {loss, out, reward};
}

// row_weight (R): the group loss's row weights -- dlp = row_weight * mask *
// dloss, reward and out unused
at::Tensor scst_loss_backward(at::Tensor seq, at::Tensor reward, at::Tensor out,
                              at::Tensor dloss, c10::optional<at::Tensor> row_weight) {
  for (auto* t : {&seq, &reward, &out, &dloss}) check_cuda(*t, "scst_loss operand");
  TORCH_CHECK(dloss.scalar_type() == at::kFloat && dloss.numel() == 1, "dloss: fp32 scalar");
  const int64_t R = seq.size(0), T = seq.size(1);
  at::Tensor dlp = at::empty({R, T}, reward.options());
  if (row_weight.has_value()) {
    const at::Tensor& w = *row_weight;
    check_cuda(w, "group_loss row weights");
    TORCH_CHECK(seq.dim() == 2 && seq.scalar_type() == at::kLong &&
                    w.scalar_type() == at::kFloat && w.numel() == R,
                "group_loss backward: seq (R, T) int64, row weights (R) fp32");
    launch_group_loss_bwd(seq.data_ptr<int64_t>(), w.data_ptr<float>(), dloss.data_ptr<float>(),
                          (int)R, (int)T, dlp.data_ptr<float>(), cur_stream());
    return dlp;
  }
  launch_scst_loss_bwd(seq.data_ptr<int64_t>(), reward.data_ptr<float>(), out.data_ptr<float>(),
                       dloss.data_ptr<float>(), (int)R, (int)T, dlp.data_ptr<float>(),
                       cur_stream());
  return dlp;
}

// XE loss (csrc/kernels/loss.hip): labels (R, L) int64 -- the full label
// rows the loader's masks come from --, lp (R, T) fp32 gathered GT log-probs
// of columns off .. off + T - 1 -> {loss (0-dim), out = [loss, sum mask], cnt
// (R) counted positions per row}
std::vector<at::Tensor> xe_loss_forward(at::Tensor labels, at::Tensor lp, int64_t off) {
  check_cuda(labels, "xe_loss labels");
  check_cuda(lp, "xe_loss lp");
  const int64_t R = labels.size(0), L = labels.size(1), T = lp.size(1);
  TORCH_CHECK(labels.scalar_type() == at::kLong && lp.scalar_type() == at::kFloat &&
                  labels.dim() == 2 && lp.dim() == 2 && lp.size(0) == R && off >= 0 &&
                  off + T <= L,
              "xe_loss: labels (R, L) int64, lp (R, T) fp32 with off + T <= L");
  auto f32 = lp.options();
  at::Tensor out = at::empty({2}, f32), cnt = at::empty({R}, f32), loss = at::empty({}, f32);
  at::Tensor ws = at::zeros({scst_loss_ws_ints((int)R)}, f32.dtype(at::kInt));
  launch_xe_loss_fwd(labels.data_ptr<int64_t>(), (int)L, (int)off, lp.data_ptr<float>(), (int)R,
                     (int)T, cnt.data_ptr<float>(), out.data_ptr<float>(), loss.data_ptr<float>(),
                     ws.data_ptr<int>(), cur_stream());
  return {loss, out, cnt};
}

at::Tensor xe_loss_backward(at::Tensor cnt, at::Tensor out, at::Tensor dloss, int64_t T) {
  for (auto* t : {&cnt, &out, &dloss}) check_cuda(*t, "xe_loss operand");
  TORCH_CHECK(dloss.scalar_type() == at::kFloat && dloss.numel() == 1 &&
                  cnt.scalar_type() == at::kFloat && out.numel() == 2,
              "xe_loss_backward: fp32 cnt (R), out (2), dloss scalar");
  const int64_t R = cnt.size(0);
  at::Tensor dlp = at::empty({R, T}, cnt.options());
  launch_xe_loss_bwd(cnt.data_ptr<float>(), out.data_ptr<float>(), dloss.data_ptr<float>(), (int)R,
                     (int)T, dlp.data_ptr<float>(), cur_stream());
  return dlp;
}

// Leave-one-out scoring: the optional (N) int64 device array of the metric
// scorers, exclude[h] = the in-video index of a reference hypothesis h does not
// see (cider_common.h excluded_ref).  Null when not given.
static const int64_t* exclude_ptr(const c10::optional<at::Tensor>& exclude, int64_t N) {
  if (!exclude.has_value() || !exclude->defined()) return nullptr;
  check_cuda(*exclude, "exclude");
  TORCH_CHECK(exclude->scalar_type() == at::kLong && exclude->dim() == 1 &&
                  exclude->size(0) == N && exclude->is_contiguous(),
              "exclude: contiguous int64 (N)");
  return exclude->data_ptr<int64_t>();
}

// On-GPU CIDEr-D scores of N hypotheses.
at::Tensor cider_score(at::Tensor hyps, at::Tensor hyp_video, std::map<std::string, at::Tensor> t,
                       double log_ref_len, int64_t use_eos, bool clipped,
                       c10::optional<at::Tensor> exclude, int64_t group) {
  check_cuda(hyps, "hyps");
  if (group != 0) {
    // Peer mode (consensus / MBR decoding, kernels/cider_pairwise.hip): rows
    // [k * group, (k + 1) * group) are one pool, every row is scored against the
    // others of its pool.  Only the df hash table is read; hyp_video is ignored.
    TORCH_CHECK(hyps.scalar_type() == at::kLong && hyps.dim() == 2, "hyps: int64 (N, T)");
    const int64_t N = hyps.size(0), T = hyps.size(1);
    TORCH_CHECK(group >= 2, "cider_score: group = ", group,
                "; a peer pool has at least 2 rows (group = 0: reference tables)");
    TORCH_CHECK(clipped && !(exclude.has_value() && exclude->defined()),
                "cider_score: peer mode (group > 0) is CIDEr-D without exclude: clipped must be "
                "True and exclude None");
    TORCH_CHECK(N % group == 0, "cider_score: ", N, " rows are not whole pools of ", group);
    TORCH_CHECK(peer_cider_supported(group, T), "cider_score: a pool of group = ", group,
                " rows of T = ", T, " tokens is outside the peer kernel's limit: group <= 64, "
                "1 <= T <= 63 and group * (T + 1) <= 2048 (64 rows of 31 tokens, 32 rows of 63)");
    TORCH_CHECK(t.count("ht_keys") && t.count("ht_vals"), "tables: ht_keys and ht_vals");
    const at::Tensor& hk = t["ht_keys"];
    const at::Tensor& hv = t["ht_vals"];
    check_cuda(hk, "ht_keys");
    check_cuda(hv, "ht_vals");
    TORCH_CHECK(hk.scalar_type() == at::kLong && hv.scalar_type() == at::kFloat &&
                    hk.numel() == hv.numel() && hk.numel() > 0 &&
                    (hk.numel() & (hk.numel() - 1)) == 0,
                "df hash table: int64 keys and fp32 values of one power-of-two size");
    at::Tensor out = at::empty({N}, hyps.options().dtype(at::kFloat));
    launch_cider_pairwise(hyps.data_ptr<int64_t>(), (int)T, (int)group, (int)(N / group),
                          hk.data_ptr<int64_t>(), hv.data_ptr<float>(), (uint32_t)hk.numel(),
                          (float)log_ref_len, (int)use_eos, out.data_ptr<float>(), cur_stream());
    return out;
  }
  check_cuda(hyp_video, "hyp_video");
  TORCH_CHECK(hyps.scalar_type() == at::kLong && hyp_video.scalar_type() == at::kLong,
              "int64 inputs");
  const int64_t N = hyps.size(0), T = hyps.size(1);
  // (clipped = false: coco CIDEr of the validation scorer, up to 64 tokens)
  TORCH_CHECK(T <= (clipped ? 63 : 64), "hypotheses longer than ", clipped ? 63 : 64,
              " tokens are not supported");
  at::Tensor out = at::empty({N}, hyps.options().dtype(at::kFloat));
  (clipped ? launch_cider_d : launch_cider_unclipped)(
      hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N,
                 t["ht_keys"].data_ptr<int64_t>(), t["ht_vals"].data_ptr<float>(),
                 (uint32_t)t["ht_keys"].numel(), t["vid_ref_off"].data_ptr<int32_t>(),
                 t["ref_ng_off"].data_ptr<int32_t>(), t["ref_norm"].data_ptr<float>(),
                 t["ref_len"].data_ptr<int32_t>(), t["ng_key"].data_ptr<int64_t>(),
                 t["ng_val"].data_ptr<float>(), (float)log_ref_len, (int)use_eos,
                 exclude_ptr(exclude, N), out.data_ptr<float>(), cur_stream());
  return out;
}

// On-GPU sentence BLEU-4 / ROUGE-L scores of N hypotheses (kernels/sent_metrics.hip).
// No allocation besides the result and no synchronisation: capturable.
at::Tensor metric_score(const std::string& metric, at::Tensor hyps, at::Tensor hyp_video,
                        std::map<std::string, at::Tensor> t, int64_t use_eos,
                        c10::optional<at::Tensor> exclude) {
  check_cuda(hyps, "hyps");
  check_cuda(hyp_video, "hyp_video");
  TORCH_CHECK(hyps.dim() == 2 && hyp_video.dim() == 1 && hyp_video.size(0) == hyps.size(0),
              "hyps (N, T) and hyp_video (N)");
  TORCH_CHECK(hyps.scalar_type() == at::kLong && hyp_video.scalar_type() == at::kLong,
              "int64 inputs");
  const bool bleu = metric == "Bleu_4";
  TORCH_CHECK(bleu || metric == "ROUGE_L", "metric_score: metric must be Bleu_4 or ROUGE_L, got ",
              metric);
  const int64_t N = hyps.size(0), T = hyps.size(1);
  TORCH_CHECK(T <= 64, "hypotheses of ", T, " tokens; at most 64 are supported");
  for (const char* k : {"vid_ref_off", "ref_len", "vid_ng_off", "ng_key", "ng_cnt", "ref_tok_off",
                        "ref_tok"}) {
    TORCH_CHECK(t.count(k), "metric tables lack ", k);
    check_cuda(t[k], k);
    TORCH_CHECK(t[k].scalar_type() == (std::string(k) == "ng_key" ? at::kLong : at::kInt),
                "metric table ", k, " has the wrong dtype");
  }
  const int Nv = (int)t["vid_ref_off"].numel() - 1;
  TORCH_CHECK(Nv >= 0 && t["vid_ng_off"].numel() == Nv + 1 &&
                  t["ref_tok_off"].numel() == t["ref_len"].numel() + 1,
              "metric tables are inconsistent");
  const int64_t* ex = exclude_ptr(exclude, N);
  const int32_t *cnt2 = nullptr, *arg = nullptr;
  if (bleu && ex) {  // (leave-one-out BLEU: the clip counts without their only holder)
    for (const char* k : {"ng_cnt2", "ng_arg"}) {
      TORCH_CHECK(t.count(k), "metric tables lack ", k, " (leave-one-out BLEU)");
      check_cuda(t[k], k);
      TORCH_CHECK(t[k].scalar_type() == at::kInt && t[k].is_contiguous() &&
                      t[k].numel() == t["ng_key"].numel(),
                  "metric table ", k, " has the wrong dtype or size");
    }
    cnt2 = t["ng_cnt2"].data_ptr<int32_t>(), arg = t["ng_arg"].data_ptr<int32_t>();
  }
  at::Tensor out = at::empty({N}, hyps.options().dtype(at::kFloat));
  if (bleu)
    launch_bleu4(hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N, Nv,
                 t["vid_ref_off"].data_ptr<int32_t>(), t["ref_len"].data_ptr<int32_t>(),
                 t["vid_ng_off"].data_ptr<int32_t>(), t["ng_key"].data_ptr<int64_t>(),
                 t["ng_cnt"].data_ptr<int32_t>(), cnt2, arg, (int)use_eos, ex,
                 out.data_ptr<float>(), cur_stream());
  else
    launch_rouge_l(hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N, Nv,
                   t["vid_ref_off"].data_ptr<int32_t>(), t["ref_tok_off"].data_ptr<int32_t>(),
                   t["ref_tok"].data_ptr<int32_t>(), (int)use_eos, ex, out.data_ptr<float>(),
                   cur_stream());
  return out;
}

// Mixed-metric reward (kernels/reward_mix.hip): weights = (w_c, w_b, w_r) over
// CIDEr-D, BLEU-4, ROUGE-L; returns {out (N), parts (N, 3)}.  The tables of a
// metric of weight 0 are not read and may be None.  One launch, no allocation
// besides the results and no synchronisation: capturable.  Limits (checked
// here, before the launch): T <= 64, T <= 63 with CIDEr-D; token ids are those
// of the tables' builders (<= 65,534 in the references; a larger hypothesis
// token matches nothing, as in bleu4_kernel).
std::vector<at::Tensor> reward_mix_score(
    at::Tensor hyps, at::Tensor hyp_video,
    c10::optional<std::map<std::string, at::Tensor>> cider_tables,
    c10::optional<std::map<std::string, at::Tensor>> sent_tables, double log_ref_len,
    int64_t use_eos, std::vector<double> weights) {
  check_cuda(hyps, "hyps");
  check_cuda(hyp_video, "hyp_video");
  TORCH_CHECK(hyps.dim() == 2 && hyp_video.dim() == 1 && hyp_video.size(0) == hyps.size(0),
              "hyps (N, T) and hyp_video (N)");
  TORCH_CHECK(hyps.scalar_type() == at::kLong && hyp_video.scalar_type() == at::kLong,
              "int64 inputs");
  TORCH_CHECK(hyps.is_contiguous() && hyp_video.is_contiguous(), "contiguous inputs");
  TORCH_CHECK(weights.size() == 3, "reward_mix_score: weights = (CIDEr, Bleu_4, ROUGE_L)");
  for (double w : weights)
    TORCH_CHECK(std::isfinite(w) && w >= 0.0, "reward_mix_score: weight ", w,
                " is negative or not finite");
  const float w_c = (float)weights[0], w_b = (float)weights[1], w_r = (float)weights[2];
  TORCH_CHECK(w_c != 0.f || w_b != 0.f || w_r != 0.f, "reward_mix_score: all weights are zero");
  const int64_t N = hyps.size(0), T = hyps.size(1);
  const int64_t maxT = w_c != 0.f ? 63 : 64;
  TORCH_CHECK(T <= maxT, "hypotheses of ", T, " tokens; at most ", maxT,
              " are supported", w_c != 0.f ? " with CIDEr-D in the mix" : "");
  MixCiderArgs c;
  MixSentArgs s;
  if (w_c != 0.f) {
    TORCH_CHECK(cider_tables.has_value(), "reward_mix_score: CIDEr has a weight but no tables");
    auto& t = *cider_tables;
    for (const char* k : {"ht_keys", "ht_vals", "vid_ref_off", "ref_ng_off", "ref_norm", "ref_len",
                          "ng_key", "ng_val"}) {
      TORCH_CHECK(t.count(k), "CIDEr-D tables lack ", k);
      check_cuda(t[k], k);
      const std::string n(k);
      const auto want = (n == "ht_keys" || n == "ng_key") ? at::kLong
                        : (n == "ht_vals" || n == "ref_norm" || n == "ng_val") ? at::kFloat
                                                                               : at::kInt;
      TORCH_CHECK(t[k].scalar_type() == want && t[k].is_contiguous(), "CIDEr-D table ", k,
                  " has the wrong dtype");
    }
    const int64_t cap = t["ht_keys"].numel(), nref = t["ref_len"].numel();
    TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0 && t["ht_vals"].numel() == cap,
                "df hash table: int64 keys and fp32 values of one power-of-two size");
    TORCH_CHECK(t["vid_ref_off"].numel() >= 1 && t["ref_ng_off"].numel() == nref + 1 &&
                    t["ref_norm"].numel() == 4 * nref &&
                    t["ng_key"].numel() == t["ng_val"].numel(),
                "CIDEr-D tables are inconsistent");
    c.Nv = (int)t["vid_ref_off"].numel() - 1;
    c.ht_keys = t["ht_keys"].data_ptr<int64_t>();
    c.ht_vals = t["ht_vals"].data_ptr<float>();
    c.ht_cap = (uint32_t)cap;
    c.vid_ref_off = t["vid_ref_off"].data_ptr<int32_t>();
    c.ref_ng_off = t["ref_ng_off"].data_ptr<int32_t>();
    c.ref_norm = t["ref_norm"].data_ptr<float>();
    c.ref_len = t["ref_len"].data_ptr<int32_t>();
    c.ng_key = t["ng_key"].data_ptr<int64_t>();
    c.ng_val = t["ng_val"].data_ptr<float>();
    c.log_ref_len = (float)log_ref_len;
  }
  if (w_b != 0.f || w_r != 0.f) {
    TORCH_CHECK(sent_tables.has_value(),
                "reward_mix_score: Bleu_4 / ROUGE_L has a weight but no tables");
    auto& t = *sent_tables;
    for (const char* k : {"vid_ref_off", "ref_len", "vid_ng_off", "ng_key", "ng_cnt",
                          "ref_tok_off", "ref_tok"}) {
      TORCH_CHECK(t.count(k), "metric tables lack ", k);
      check_cuda(t[k], k);
      TORCH_CHECK(t[k].scalar_type() == (std::string(k) == "ng_key" ? at::kLong : at::kInt) &&
                      t[k].is_contiguous(),
                  "metric table ", k, " has the wrong dtype");
    }
    s.Nv = (int)t["vid_ref_off"].numel() - 1;
    TORCH_CHECK(s.Nv >= 0 && t["vid_ng_off"].numel() == s.Nv + 1 &&
                    t["ref_tok_off"].numel() == t["ref_len"].numel() + 1 &&
                    t["ng_cnt"].numel() == t["ng_key"].numel(),
                "metric tables are inconsistent");
    s.vid_ref_off = t["vid_ref_off"].data_ptr<int32_t>();
    s.ref_len = t["ref_len"].data_ptr<int32_t>();
    s.vid_ng_off = t["vid_ng_off"].data_ptr<int32_t>();
    s.ng_key = t["ng_key"].data_ptr<int64_t>();
    s.ng_cnt = t["ng_cnt"].data_ptr<int32_t>();
    s.ref_tok_off = t["ref_tok_off"].data_ptr<int32_t>();
    s.ref_tok = t["ref_tok"].data_ptr<int32_t>();
  }
  at::Tensor out = at::empty({N}, hyps.options().dtype(at::kFloat));
  at::Tensor parts = at::empty({N, 3}, hyps.options().dtype(at::kFloat));
  launch_reward_mix(hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N, c, s,
                    (int)use_eos, w_c, w_b, w_r, out.data_ptr<float>(), parts.data_ptr<float>(),
                    cur_stream());
  return {out, parts};
}

// Peer scores under a mixed utility (kernels/peer_mix.hip; consensus / MBR
// decoding): rows [k * group, (k + 1) * group) of hyps are one pool, every row is
// scored against the others of its pool.  weights = (w_c, w_b, w_r) over CIDEr-D,
// BLEU-4, ROUGE-L; returns {out (N), parts (N, 3)}.  Only the df hash table
// (ht_keys / ht_vals of `df`) is read, and only when w_c > 0: it may be None
// otherwise.  One launch, no allocation besides the results and no
// synchronisation: capturable.  Everything is checked here, before the launch.
std::vector<at::Tensor> peer_mix_score(at::Tensor hyps,
                                       c10::optional<std::map<std::string, at::Tensor>> df,
                                       double log_ref_len, int64_t use_eos,
                                       std::vector<double> weights, int64_t group) {
  check_cuda(hyps, "hyps");
  TORCH_CHECK(hyps.scalar_type() == at::kLong && hyps.dim() == 2 && hyps.is_contiguous(),
              "hyps: contiguous int64 (N, T)");
  const int64_t N = hyps.size(0), T = hyps.size(1);
  TORCH_CHECK(group >= 2, "metric_score: group = ", group,
              "; a peer pool has at least 2 rows (group = 0: reference tables)");
  TORCH_CHECK(N % group == 0, "metric_score: ", N, " rows are not whole pools of ", group);
  TORCH_CHECK(peer_cider_supported(group, T), "metric_score: a pool of group = ", group,
              " rows of T = ", T, " tokens is outside the peer kernel's limit: group <= 64, "
              "1 <= T <= 63 and group * (T + 1) <= 2048 (64 rows of 31 tokens, 32 rows of 63)");
  TORCH_CHECK(weights.size() == 3, "metric_score: weights = (CIDEr, Bleu_4, ROUGE_L)");
  for (double w : weights)
    TORCH_CHECK(std::isfinite(w) && w >= 0.0, "metric_score: weight ", w,
                " is negative or not finite");
  const float w_c = (float)weights[0], w_b = (float)weights[1], w_r = (float)weights[2];
  TORCH_CHECK(w_c != 0.f || w_b != 0.f || w_r != 0.f, "metric_score: all weights are zero");
  const int64_t* hk = nullptr;
  const float* hv = nullptr;
  uint32_t cap = 0;
  if (w_c != 0.f) {
    TORCH_CHECK(df.has_value() && df->count("ht_keys") && df->count("ht_vals"),
                "metric_score: CIDEr has a weight but no df tables (cider_tables: ht_keys and "
                "ht_vals)");
    const at::Tensor& k = df->at("ht_keys");
    const at::Tensor& v = df->at("ht_vals");
    check_cuda(k, "ht_keys");
    check_cuda(v, "ht_vals");
    TORCH_CHECK(k.scalar_type() == at::kLong && v.scalar_type() == at::kFloat &&
                    k.is_contiguous() && v.is_contiguous() && k.numel() == v.numel() &&
                    k.numel() > 0 && (k.numel() & (k.numel() - 1)) == 0,
                "df hash table: int64 keys and fp32 values of one power-of-two size");
    hk = k.data_ptr<int64_t>(), hv = v.data_ptr<float>(), cap = (uint32_t)k.numel();
  }
  at::Tensor out = at::empty({N}, hyps.options().dtype(at::kFloat));
  at::Tensor parts = at::empty({N, 3}, hyps.options().dtype(at::kFloat));
  launch_peer_mix(hyps.data_ptr<int64_t>(), (int)T, (int)group, (int)(N / group), hk, hv, cap,
                  (float)log_ref_len, (int)use_eos, w_c, w_b, w_r, out.data_ptr<float>(),
                  parts.data_ptr<float>(), cur_stream());
  return {out, parts};
}

// Validation scorer (kernels/corpus_metrics.hip): per-hypothesis statistics of
// corpus BLEU ((N, 10) int32) or METEOR ((N, 6) int32 and the (N) fp64 segment
// scores) against the tables of metric_build_tables (METEOR: built with stem
// ids, which are passed again for the hypothesis tokens).
static int check_corpus_inputs(at::Tensor& hyps, at::Tensor& hyp_video,
                               std::map<std::string, at::Tensor>& t,
                               std::initializer_list<const char*> keys) {
  check_cuda(hyps, "hyps");
  check_cuda(hyp_video, "hyp_video");
  TORCH_CHECK(hyps.dim() == 2 && hyp_video.dim() == 1 && hyp_video.size(0) == hyps.size(0),
              "hyps (N, T) and hyp_video (N)");
  TORCH_CHECK(hyps.scalar_type() == at::kLong && hyp_video.scalar_type() == at::kLong &&
                  hyps.is_contiguous() && hyp_video.is_contiguous(),
              "contiguous int64 inputs");
  TORCH_CHECK(hyps.size(1) <= 64, "hypotheses of ", hyps.size(1),
              " tokens; at most 64 are supported");
  for (const char* k : keys) {
    TORCH_CHECK(t.count(k), "metric tables lack ", k);
    check_cuda(t[k], k);
    TORCH_CHECK(t[k].scalar_type() == (std::string(k) == "ng_key" ? at::kLong : at::kInt) &&
                    t[k].is_contiguous(),
                "metric table ", k, " has the wrong dtype or layout");
  }
  const int Nv = (int)t["vid_ref_off"].numel() - 1;
  TORCH_CHECK(Nv >= 0, "metric tables are inconsistent");
  return Nv;
}

at::Tensor bleu_stats(at::Tensor hyps, at::Tensor hyp_video, std::map<std::string, at::Tensor> t) {
  const int Nv = check_corpus_inputs(hyps, hyp_video, t,
                                     {"vid_ref_off", "ref_len", "vid_ng_off", "ng_key", "ng_cnt"});
  TORCH_CHECK(t["vid_ng_off"].numel() == Nv + 1 && t["ng_cnt"].numel() == t["ng_key"].numel(),
              "metric tables are inconsistent");
  const int64_t N = hyps.size(0), T = hyps.size(1);
  at::Tensor out = at::empty({N, 10}, hyps.options().dtype(at::kInt));
  launch_bleu_stats(hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N, Nv,
                    t["vid_ref_off"].data_ptr<int32_t>(), t["ref_len"].data_ptr<int32_t>(),
                    t["vid_ng_off"].data_ptr<int32_t>(), t["ng_key"].data_ptr<int64_t>(),
                    t["ng_cnt"].data_ptr<int32_t>(), out.data_ptr<int32_t>(), cur_stream());
  return out;
}

std::vector<at::Tensor> meteor_stats(at::Tensor hyps, at::Tensor hyp_video,
                                     std::map<std::string, at::Tensor> t, at::Tensor stem_ids,
                                     c10::optional<at::Tensor> exclude) {
  const int Nv = check_corpus_inputs(hyps, hyp_video, t,
                                     {"vid_ref_off", "ref_len", "ref_tok_off", "ref_tok",
                                      "ref_stem"});
  check_cuda(stem_ids, "stem_ids");
  TORCH_CHECK(stem_ids.scalar_type() == at::kInt && stem_ids.dim() == 1 &&
                  stem_ids.is_contiguous(),
              "stem_ids: contiguous int32 (V)");
  TORCH_CHECK(t["ref_tok_off"].numel() == t["ref_len"].numel() + 1 &&
                  t["ref_stem"].numel() == t["ref_tok"].numel(),
              "metric tables are inconsistent (built without stem ids?)");
  const int64_t N = hyps.size(0), T = hyps.size(1);
  at::Tensor stats = at::empty({N, 6}, hyps.options().dtype(at::kInt));
  at::Tensor score = at::empty({N}, hyps.options().dtype(at::kDouble));
  launch_meteor_stats(hyps.data_ptr<int64_t>(), (int)T, hyp_video.data_ptr<int64_t>(), (int)N, Nv,
                      t["vid_ref_off"].data_ptr<int32_t>(), t["ref_tok_off"].data_ptr<int32_t>(),
                      t["ref_tok"].data_ptr<int32_t>(), t["ref_stem"].data_ptr<int32_t>(),
                      stem_ids.data_ptr<int32_t>(), (int)stem_ids.numel(), exclude_ptr(exclude, N),
                      stats.data_ptr<int32_t>(), score.data_ptr<double>(), cur_stream());
  return {stats, score};
}

// Shadow-copy segments from Python: meta = int64 CPU (n, 8) rows {off, n,
// kind, cols, H, E, ld2, slots}; dsts = 2 tensors per row (dst, dst2; undefined or
// empty when unused).
static ShadowSegs make_shadow_segs(const at::Tensor& meta, const std::vector<at::Tensor>& dsts) {
  ShadowSegs ss{};
  if (!meta.defined() || meta.numel() == 0) return ss;
  TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.dim() == 2 &&
                  meta.size(1) == 8 && meta.size(0) <= SHADOW_MAX_SEGS,
              "shadow meta must be an int64 CPU (n <= ", SHADOW_MAX_SEGS, ", 8) tensor");
  TORCH_CHECK((int64_t)dsts.size() == 2 * meta.size(0), "two destination tensors per segment");
  auto m = meta.accessor<int64_t, 2>();
  ss.n = (int)meta.size(0);
  for (int k = 0; k < ss.n; ++k) {
    ShadowSeg& g = ss.s[k];
    g.off = m[k][0], g.n = m[k][1], g.kind = (int)m[k][2], g.cols = (int)m[k][3];
    g.H = (int)m[k][4], g.E = (int)m[k][5], g.ld2 = (int)m[k][6], g.slots = (int)m[k][7];
    const at::Tensor& d = dsts[2 * k];
    const at::Tensor& d2 = dsts[2 * k + 1];
    TORCH_CHECK(d.is_cuda() && d.scalar_type() == at::kBFloat16, "shadow dst must be bf16 GPU");
    g.dst = reinterpret_cast<uint16_t*>(d.data_ptr());
    g.dst2 = d2.defined() && d2.numel() ? reinterpret_cast<uint16_t*>(d2.data_ptr()) : nullptr;
    if (g.kind == SHADOW_PLAIN) {
      TORCH_CHECK(d.numel() >= g.n, "plain shadow too small");
    } else {
      const int64_t rows = g.cols > 0 ? g.n / g.cols : 0;
      const int64_t gates = g.H > 0 ? rows / g.H : 0;
      TORCH_CHECK(g.H > 0 && g.cols > 0 && g.n % g.cols == 0 && rows % g.H == 0 &&
                      (gates == 1 || gates == 3 || gates == 4) &&
                      d.numel() >= 4 * (int64_t)g.H * (g.E + g.H),
                  "gate-weight shadow segment shape");
      for (int q = 0; q < gates; ++q)
        for (int q2 = 0; q2 < q; ++q2)
          TORCH_CHECK(((g.slots >> (2 * q)) & 3) != ((g.slots >> (2 * q2)) & 3),
                      "gate slot map must be injective");
      if (g.kind == SHADOW_GATES_HH)
        TORCH_CHECK(g.dst2 != nullptr && g.cols == g.H && d2.numel() >= 4 * (int64_t)g.H * g.ld2,
                    "W_hh shadow needs its packed copy");
      if (g.kind == SHADOW_GATES_IH && g.dst2 != nullptr)
        TORCH_CHECK(g.cols > g.E && g.ld2 >= g.cols - g.E && d2.numel() >= 4 * (int64_t)g.H * g.ld2,
                    "W_ih video-column shadow shape");
    }
  }
  return ss;
}

// hyper (device fp32): [lr, step before, skipped, step after] (kernels/adam.hip).
// phase: 0 = both passes; 1 = sum of squares only (the caller all-reduces the
// partials of a sharded update before phase 2); 2 = update only.
at::Tensor flat_adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                          at::Tensor partials, at::Tensor scal, at::Tensor skip, at::Tensor hyper,
                          double b1, double b2, double eps, double clip, double gscale,
                          int64_t phase, at::Tensor shadow_meta,
                          std::vector<at::Tensor> shadow_dst, c10::optional<at::Tensor> ema,
                          double ema_decay) {
  check_cuda(p, "p");
  for (auto* t : {&g, &m, &v}) {
    check_cuda(*t, "adam operand");
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == p.numel(), "adam operand shape");
  }
  TORCH_CHECK(partials.numel() >= 1024 && scal.numel() >= 2, "workspace too small");
  TORCH_CHECK(hyper.is_cuda() && hyper.scalar_type() == at::kFloat && hyper.numel() >= 4,
              "hyper must be fp32 [lr, step, skipped, step after] on the GPU");
  TORCH_CHECK(phase >= 0 && phase <= 2, "phase: 0 both, 1 sumsq, 2 update");
  const ShadowSegs ss = make_shadow_segs(shadow_meta, shadow_dst);
  for (int k = 0; k < ss.n; ++k)
    TORCH_CHECK(ss.s[k].off >= 0 && ss.s[k].off + ss.s[k].n <= p.numel(), "shadow range");
  // parameter EMA kept by the update pass (undefined or empty: off)
  float* ema_ptr = nullptr;
  float one_minus_d = 0.f;
  if (ema.has_value() && ema->defined() && ema->numel() > 0) {
    check_cuda(*ema, "ema");
    TORCH_CHECK(ema->scalar_type() == at::kFloat && ema->numel() == p.numel(),
                "ema must be fp32 with the numel of p");
    TORCH_CHECK(ema_decay >= 0.0 && ema_decay < 1.0, "ema_decay must be in [0, 1), got ",
                ema_decay);
    ema_ptr = ema->data_ptr<float>();
    TORCH_CHECK(reinterpret_cast<uintptr_t>(ema_ptr) % 16 == 0, "ema must be 16-byte aligned");
    one_minus_d = (float)(1.0 - ema_decay);
  }
  launch_flat_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                   v.data_ptr<float>(), p.numel(), partials.data_ptr<float>(),
                   skip.data_ptr<bool>(), scal.data_ptr<float>(), hyper.data_ptr<float>(),
                   (float)b1, (float)b2, (float)eps, (float)clip, (float)gscale, (int)phase, ss,
                   ema_ptr, one_minus_d, cur_stream());
  return scal.narrow(0, 0, 1).squeeze(0);
}

// swap_with given: p and swap_with are exchanged element by element and the
// shadows are written from the new p, in one pass (FlatAdam.swap_ema)
void refresh_shadows(at::Tensor p, at::Tensor shadow_meta, std::vector<at::Tensor> shadow_dst,
                     c10::optional<at::Tensor> swap_with) {
  check_cuda(p, "p");
  const ShadowSegs ss = make_shadow_segs(shadow_meta, shadow_dst);
  for (int k = 0; k < ss.n; ++k)
    TORCH_CHECK(ss.s[k].off >= 0 && ss.s[k].off + ss.s[k].n <= p.numel(), "shadow range");
  if (swap_with.has_value() && swap_with->defined()) {
    const at::Tensor& q = *swap_with;
    check_cuda(q, "swap_with");
    TORCH_CHECK(p.scalar_type() == at::kFloat && q.scalar_type() == at::kFloat &&
                    q.numel() == p.numel(),
                "swap_with must be fp32 with the numel of p");
    float* pp = p.data_ptr<float>();
    float* qq = q.data_ptr<float>();
    TORCH_CHECK(reinterpret_cast<uintptr_t>(pp) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(qq) % 16 == 0,
                "p and swap_with must be 16-byte aligned");
    TORCH_CHECK(pp + p.numel() <= qq || qq + q.numel() <= pp, "p and swap_with overlap");
    launch_swap_refresh(pp, qq, p.numel(), ss, cur_stream());
    return;
  }
  launch_shadow_refresh(p.data_ptr<float>(), ss, cur_stream());
}

}  // namespace cst
