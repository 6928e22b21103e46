// Python bindings of the native extension cst_captioning_amd._C.
#include <torch/extension.h>

#include "engine.h"
#include "host/cider_host.h"
#include "host/metric_host.h"
#include "launchers.h"

namespace cst {

template <class T>
static at::Tensor to_tensor(const std::vector<T>& v, at::ScalarType st) {
  at::Tensor t = at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(st));
  if (!v.empty()) std::memcpy(t.data_ptr(), v.data(), v.size() * sizeof(T));
  return t;
}

static std::map<std::string, at::Tensor> cider_build_tables(at::Tensor labels, at::Tensor start,
                                                            at::Tensor end, at::Tensor df_keys,
                                                            at::Tensor df_vals,
                                                            double log_ref_len, int64_t use_eos) {
  TORCH_CHECK(!labels.is_cuda(), "host builder takes CPU tensors");
  labels = labels.contiguous().to(at::kLong);
  start = start.contiguous().to(at::kLong);
  end = end.contiguous().to(at::kLong);
  df_keys = df_keys.contiguous().to(at::kLong);
  df_vals = df_vals.contiguous().to(at::kFloat);
  CiderTables t = build_cider_tables(labels.data_ptr<int64_t>(), (int)labels.size(0),
                                     (int)labels.size(1), start.data_ptr<int64_t>(),
                                     end.data_ptr<int64_t>(), (int)start.numel(),
                                     df_keys.data_ptr<int64_t>(), df_vals.data_ptr<float>(),
                                     (int)df_keys.numel(), log_ref_len, (int)use_eos);
  return {{"ht_keys", to_tensor(t.ht_keys, at::kLong)},
          {"ht_vals", to_tensor(t.ht_vals, at::kFloat)},
          {"vid_ref_off", to_tensor(t.vid_ref_off, at::kInt)},
          {"ref_ng_off", to_tensor(t.ref_ng_off, at::kInt)},
          {"ref_norm", to_tensor(t.ref_norm, at::kFloat)},
          {"ref_len", to_tensor(t.ref_len, at::kInt)},
          {"ng_key", to_tensor(t.ng_key, at::kLong)},
          {"ng_val", to_tensor(t.ng_val, at::kFloat)}};
}

// the CPU scorers' hypotheses: hyps (N, T), hyp_video (N), as contiguous int64
static void cpu_hyps(at::Tensor& hyps, at::Tensor& hyp_video) {
  TORCH_CHECK(!hyps.is_cuda() && hyps.dim() == 2 && hyp_video.dim() == 1 &&
                  hyp_video.size(0) == hyps.size(0),
              "CPU hyps (N, T) and hyp_video (N)");
  hyps = hyps.contiguous().to(at::kLong);
  hyp_video = hyp_video.contiguous().to(at::kLong);
}

// the CPU scorers' optional leave-one-out array: (N) as contiguous int64 (`keep`
// owns the converted copy), null when not given
static const int64_t* cpu_exclude(const c10::optional<at::Tensor>& exclude, int64_t N,
                                  at::Tensor& keep) {
  if (!exclude.has_value() || !exclude->defined()) return nullptr;
  TORCH_CHECK(!exclude->is_cuda() && exclude->dim() == 1 && exclude->size(0) == N,
              "exclude: CPU (N)");
  keep = exclude->contiguous().to(at::kLong);
  return keep.data_ptr<int64_t>();
}

static at::Tensor cider_score_cpu(at::Tensor hyps, at::Tensor hyp_video,
                                  std::map<std::string, at::Tensor> t, double log_ref_len,
                                  int64_t use_eos, bool clipped,
                                  c10::optional<at::Tensor> exclude, int64_t group) {
  if (group != 0) {  // peer mode: every row against the others of its pool of `group`
    TORCH_CHECK(!hyps.is_cuda() && hyps.dim() == 2, "CPU hyps (N, T)");
    TORCH_CHECK(group >= 2, "cider_score_cpu: group = ", group,
                "; a peer pool has at least 2 rows (group = 0: reference tables)");
    TORCH_CHECK(clipped && !(exclude.has_value() && exclude->defined()),
                "cider_score_cpu: peer mode (group > 0) is CIDEr-D without exclude: clipped must "
                "be True and exclude None");
    TORCH_CHECK(hyps.size(0) % group == 0, "cider_score_cpu: ", hyps.size(0),
                " rows are not whole pools of ", group);
    TORCH_CHECK(t.count("ht_keys") && t.count("ht_vals"), "tables: ht_keys and ht_vals");
    hyps = hyps.contiguous().to(at::kLong);
    at::Tensor hk = t["ht_keys"].contiguous().to(at::kLong);
    at::Tensor hv = t["ht_vals"].contiguous().to(at::kFloat);
    TORCH_CHECK(!hk.is_cuda() && !hv.is_cuda() && hk.numel() == hv.numel() && hk.numel() > 0 &&
                    (hk.numel() & (hk.numel() - 1)) == 0,
                "df hash table: CPU keys and values of one power-of-two size");
    at::Tensor out = at::empty({hyps.size(0)}, at::TensorOptions().dtype(at::kFloat));
    cider_peers_host(hyps.data_ptr<int64_t>(), (int)hyps.size(0), (int)hyps.size(1), (int)group,
                     hk.data_ptr<int64_t>(), hv.data_ptr<float>(), (uint32_t)hk.numel(),
                     log_ref_len, (int)use_eos, out.data_ptr<float>());
    return out;
  }
  hyps = hyps.contiguous().to(at::kLong);
  hyp_video = hyp_video.contiguous().to(at::kLong);
  at::Tensor ex_keep;
  const int64_t* ex = cpu_exclude(exclude, hyps.size(0), ex_keep);
  CiderTablesView v{(uint32_t)t["ht_keys"].numel(), t["ht_keys"].data_ptr<int64_t>(),
                    t["ht_vals"].data_ptr<float>(), t["vid_ref_off"].data_ptr<int32_t>(),
                    t["ref_ng_off"].data_ptr<int32_t>(), t["ref_norm"].data_ptr<float>(),
                    t["ref_len"].data_ptr<int32_t>(), t["ng_key"].data_ptr<int64_t>(),
                    t["ng_val"].data_ptr<float>()};
  at::Tensor out = at::empty({hyps.size(0)}, at::TensorOptions().dtype(at::kFloat));
  cider_score_host(hyps.data_ptr<int64_t>(), (int)hyps.size(0), (int)hyps.size(1),
                   hyp_video.data_ptr<int64_t>(), v, log_ref_len, (int)use_eos,
                   out.data_ptr<float>(), clipped, ex);
  return out;
}

// Sentence BLEU-4 / ROUGE-L: per-dataset tables (CPU tensors) and the native CPU
// scorer; the host code's std::invalid_argument (over-limit inputs) surfaces as
// ValueError.
static std::map<std::string, at::Tensor> metric_build_tables(
    at::Tensor labels, at::Tensor start, at::Tensor end, int64_t use_eos,
    c10::optional<at::Tensor> stem_ids) {
  TORCH_CHECK(!labels.is_cuda() && labels.dim() == 2, "host builder takes a CPU (M, L) label table");
  TORCH_CHECK(start.numel() == end.numel(), "one label range per video");
  labels = labels.contiguous().to(at::kLong);
  start = start.contiguous().to(at::kLong);
  end = end.contiguous().to(at::kLong);
  at::Tensor stems;
  if (stem_ids.has_value()) {
    TORCH_CHECK(!stem_ids->is_cuda() && stem_ids->dim() == 1, "stem_ids: CPU (V)");
    stems = stem_ids->contiguous().to(at::kInt);
  }
  MetricTables t = build_metric_tables(
      labels.data_ptr<int64_t>(), (int)labels.size(0), (int)labels.size(1),
      start.data_ptr<int64_t>(), end.data_ptr<int64_t>(), (int)start.numel(), (int)use_eos,
      stems.defined() ? stems.data_ptr<int32_t>() : nullptr,
      stems.defined() ? (int)stems.numel() : 0);
  std::map<std::string, at::Tensor> out = {
      {"vid_ref_off", to_tensor(t.vid_ref_off, at::kInt)},
      {"ref_len", to_tensor(t.ref_len, at::kInt)},
      {"vid_ng_off", to_tensor(t.vid_ng_off, at::kInt)},
      {"ng_key", to_tensor(t.ng_key, at::kLong)},
      {"ng_cnt", to_tensor(t.ng_cnt, at::kInt)},
      {"ng_cnt2", to_tensor(t.ng_cnt2, at::kInt)},
      {"ng_arg", to_tensor(t.ng_arg, at::kInt)},
      {"ref_tok_off", to_tensor(t.ref_tok_off, at::kInt)},
      {"ref_tok", to_tensor(t.ref_tok, at::kInt)}};
  if (stems.defined())  // (validation scorer: the references' stem rows as well)
    out["ref_stem"] = to_tensor(t.ref_stem, at::kInt);
  return out;
}

static MetricTablesView metric_view(std::map<std::string, at::Tensor>& t) {
  MetricTablesView v{(int)t.at("vid_ref_off").numel() - 1,
                     t.at("vid_ref_off").data_ptr<int32_t>(), t.at("ref_len").data_ptr<int32_t>(),
                     t.at("vid_ng_off").data_ptr<int32_t>(), t.at("ng_key").data_ptr<int64_t>(),
                     t.at("ng_cnt").data_ptr<int32_t>(), t.at("ref_tok_off").data_ptr<int32_t>(),
                     t.at("ref_tok").data_ptr<int32_t>()};
  if (t.count("ng_cnt2") && t.count("ng_arg") &&
      t.at("ng_cnt2").numel() == t.at("ng_key").numel() &&
      t.at("ng_arg").numel() == t.at("ng_key").numel()) {
    v.ng_cnt2 = t.at("ng_cnt2").data_ptr<int32_t>();
    v.ng_arg = t.at("ng_arg").data_ptr<int32_t>();
  }
  return v;
}

static at::Tensor metric_score_cpu(const std::string& metric, at::Tensor hyps,
                                   at::Tensor hyp_video, std::map<std::string, at::Tensor> t,
                                   int64_t use_eos, c10::optional<at::Tensor> exclude) {
  const bool bleu = metric == "Bleu_4";
  TORCH_CHECK(bleu || metric == "ROUGE_L", "metric_score_cpu: metric must be Bleu_4 or ROUGE_L, got ",
              metric);
  cpu_hyps(hyps, hyp_video);
  at::Tensor ex_keep;
  const int64_t* ex = cpu_exclude(exclude, hyps.size(0), ex_keep);
  at::Tensor out = at::empty({hyps.size(0)}, at::TensorOptions().dtype(at::kFloat));
  (bleu ? bleu4_score_host : rouge_l_score_host)(
      hyps.data_ptr<int64_t>(), (int)hyps.size(0), (int)hyps.size(1),
      hyp_video.data_ptr<int64_t>(), metric_view(t), (int)use_eos, out.data_ptr<float>(), ex);
  return out;
}

// Peer mode of metric_score_cpu (metric mix, group = G >= 2): the native twin of
// kernels/peer_mix.hip, [out (N), parts (N, 3)].  df: the df hash table
// (ht_keys / ht_vals, CPU), None when CIDEr has weight 0.
static std::vector<at::Tensor> peer_mix_score_cpu(
    at::Tensor hyps, c10::optional<std::map<std::string, at::Tensor>> df, double log_ref_len,
    int64_t use_eos, const std::vector<double>& weights, int64_t group) {
  TORCH_CHECK(!hyps.is_cuda() && hyps.dim() == 2, "CPU hyps (N, T)");
  TORCH_CHECK(group >= 2, "metric_score_cpu: group = ", group,
              "; a peer pool has at least 2 rows (group = 0: reference tables)");
  TORCH_CHECK(hyps.size(0) % group == 0, "metric_score_cpu: ", hyps.size(0),
              " rows are not whole pools of ", group);
  TORCH_CHECK(weights.size() == 3, "metric_score_cpu: weights = (CIDEr, Bleu_4, ROUGE_L)");
  hyps = hyps.contiguous().to(at::kLong);
  at::Tensor hk, hv;
  if ((float)weights[0] != 0.f) {
    TORCH_CHECK(df.has_value() && df->count("ht_keys") && df->count("ht_vals"),
                "metric_score_cpu: CIDEr has a weight but no df tables (cider_tables: ht_keys "
                "and ht_vals)");
    hk = df->at("ht_keys").contiguous().to(at::kLong);
    hv = df->at("ht_vals").contiguous().to(at::kFloat);
    TORCH_CHECK(!hk.is_cuda() && !hv.is_cuda() && hk.numel() == hv.numel() && hk.numel() > 0 &&
                    (hk.numel() & (hk.numel() - 1)) == 0,
                "df hash table: CPU keys and values of one power-of-two size");
  }
  const int64_t N = hyps.size(0);
  at::Tensor out = at::empty({N}, at::TensorOptions().dtype(at::kFloat));
  at::Tensor parts = at::empty({N, 3}, at::TensorOptions().dtype(at::kFloat));
  peer_mix_host(hyps.data_ptr<int64_t>(), (int)N, (int)hyps.size(1), (int)group,
                hk.defined() ? hk.data_ptr<int64_t>() : nullptr,
                hv.defined() ? hv.data_ptr<float>() : nullptr,
                hk.defined() ? (uint32_t)hk.numel() : 0u, log_ref_len, (int)use_eos,
                weights.data(), out.data_ptr<float>(), parts.data_ptr<float>());
  return {out, parts};
}

// Validation scorer on the CPU: the host twins of kernels/corpus_metrics.hip.
static at::Tensor bleu_stats_cpu(at::Tensor hyps, at::Tensor hyp_video,
                                 std::map<std::string, at::Tensor> t) {
  cpu_hyps(hyps, hyp_video);
  at::Tensor out = at::empty({hyps.size(0), 10}, at::TensorOptions().dtype(at::kInt));
  bleu_stats_host(hyps.data_ptr<int64_t>(), (int)hyps.size(0), (int)hyps.size(1),
                  hyp_video.data_ptr<int64_t>(), metric_view(t), out.data_ptr<int32_t>());
  return out;
}

static std::vector<at::Tensor> meteor_stats_cpu(at::Tensor hyps, at::Tensor hyp_video,
                                                std::map<std::string, at::Tensor> t,
                                                at::Tensor stem_ids,
                                                c10::optional<at::Tensor> exclude) {
  cpu_hyps(hyps, hyp_video);
  at::Tensor ex_keep;
  const int64_t* ex = cpu_exclude(exclude, hyps.size(0), ex_keep);
  TORCH_CHECK(t.count("ref_stem") && t.at("ref_stem").numel() == t.at("ref_tok").numel(),
              "metric tables were built without stem ids");
  stem_ids = stem_ids.contiguous().to(at::kInt);
  at::Tensor stats = at::empty({hyps.size(0), 6}, at::TensorOptions().dtype(at::kInt));
  at::Tensor score = at::empty({hyps.size(0)}, at::TensorOptions().dtype(at::kDouble));
  meteor_stats_host(hyps.data_ptr<int64_t>(), (int)hyps.size(0), (int)hyps.size(1),
                    hyp_video.data_ptr<int64_t>(), metric_view(t),
                    t.at("ref_stem").data_ptr<int32_t>(), stem_ids.data_ptr<int32_t>(),
                    (int)stem_ids.numel(), stats.data_ptr<int32_t>(), score.data_ptr<double>(),
                    ex);
  return {stats, score};
}
}  // namespace cst

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "cst_captioning_amd native extension: gfx950 HIP kernels + C++ decoder executor";
  // ls_eps / ls_wbar (label smoothing, kernels/label_smooth.hip): g_xe becomes the smoothed
  // target log-prob; ls_wbar, fp32 (>= H + 1), receives the mean logit row and bias the
  // backward takes back
  m.def("decoder_forward", &cst::decoder_forward, py::arg("wx"), py::arg("emb"), py::arg("ptab"),
        py::arg("whh"), py::arg("wlog"), py::arg("blog"), py::arg("vgate"), py::arg("vgate_div"),
        py::arg("labels"), py::arg("bos"), py::arg("R"), py::arg("T"), py::arg("modes"),
        py::arg("ss_prob"), py::arg("drop_p"), py::arg("temperature"), py::arg("rng"),
        py::arg("save"), py::arg("want_xe"), py::arg("use_counts"), py::arg("use_unfinished"),
        py::arg("att"), py::arg("cell"), py::arg("state0"), py::arg("up"), py::arg("store_exp"),
        py::arg("xe_rows"), py::arg("lab_idx"), py::arg("ls_eps") = 0.0,
        py::arg("ls_wbar") = py::none());
  m.def("decoder_backward", &cst::decoder_backward, py::arg("wx"), py::arg("wlog"), py::arg("emb"),
        py::arg("lse"), py::arg("logits16"), py::arg("hdrop_all"), py::arg("gates_all"),
        py::arg("c_all"), py::arg("h_all"), py::arg("seq"), py::arg("labels"), py::arg("toks"),
        py::arg("dg_sel"), py::arg("dg_xe"), py::arg("drop_p"), py::arg("rng"),
        py::arg("out_wlog"), py::arg("out_blog"), py::arg("comm_stream"), py::arg("att"),
        py::arg("out_emb"), py::arg("ds_bias"), py::arg("cell"), py::arg("state0"), py::arg("up"),
        py::arg("blog"), py::arg("fix_total"), py::arg("vgate_div"), py::arg("xw"),
        py::arg("vg_bwd"), py::arg("vg_nf"), py::arg("vg_p"), py::arg("x_wait") = 0,
        py::arg("exp_zero_off") = false, py::arg("dw_slots") = std::vector<at::Tensor>(),
        py::arg("vg_idx") = py::none(), py::arg("vg_C") = 1, py::arg("ls_eps") = 0.0,
        py::arg("ls_wbar") = py::none());
  m.def("cider_build_tables", &cst::cider_build_tables);
  // clipped = false: coco CIDEr (no clipping, no length penalty), the validation metric
  // exclude (here and in the metric scorers below): optional (N) int64, the
  // in-video index of a reference each hypothesis leaves out (leave-one-out
  // scoring of GT captions, ops/consensus.py); negative entries leave none out
  // group = G >= 2: peer mode (consensus / MBR decoding, ops/mbr.py): hyps is B
  // pools of G rows, every row scored against the others of its pool; only
  // ht_keys / ht_vals of tables are read, hyp_video is ignored (0: as before)
  m.def("cider_score", &cst::cider_score, py::arg("hyps"), py::arg("hyp_video"),
        py::arg("tables"), py::arg("log_ref_len"), py::arg("use_eos"),
        py::arg("clipped") = true, py::arg("exclude") = py::none(), py::arg("group") = 0);
  m.def("cider_score_cpu", &cst::cider_score_cpu, py::arg("hyps"), py::arg("hyp_video"),
        py::arg("tables"), py::arg("log_ref_len"), py::arg("use_eos"),
        py::arg("clipped") = true, py::arg("exclude") = py::none(), py::arg("group") = 0);
  m.def("metric_build_tables", &cst::metric_build_tables, py::arg("labels"), py::arg("start"),
        py::arg("end"), py::arg("use_eos"), py::arg("stem_ids") = py::none(),
        "sentence BLEU-4 / ROUGE-L reference tables of a dataset (dict of CPU tensors); with "
        "stem_ids (V) also the references' stem rows (METEOR)");
  m.def("bleu_stats", &cst::bleu_stats, py::arg("hyps"), py::arg("hyp_video"), py::arg("tables"),
        "corpus BLEU statistics per hypothesis on the GPU: (N, 10) int32");
  m.def("bleu_stats_cpu", &cst::bleu_stats_cpu, py::arg("hyps"), py::arg("hyp_video"),
        py::arg("tables"));
  m.def("meteor_stats", &cst::meteor_stats, py::arg("hyps"), py::arg("hyp_video"),
        py::arg("tables"), py::arg("stem_ids"), py::arg("exclude") = py::none(),
        "METEOR alignment statistics per hypothesis on the GPU: (N, 6) int32, (N) fp64");
  m.def("meteor_stats_cpu", &cst::meteor_stats_cpu, py::arg("hyps"), py::arg("hyp_video"),
        py::arg("tables"), py::arg("stem_ids"), py::arg("exclude") = py::none());
  // metric = "mix" (--reward_mix; kernels/reward_mix.hip): weights = (w_c, w_b, w_r)
  // over CIDEr-D, Bleu_4, ROUGE_L; tables = the sentence-metric tables and
  // cider_tables / log_ref_len those of cider_score, each None when its metrics
  // have weight 0; returns [out (N), parts (N, 3)] of ONE launch
  // (cst::reward_mix_score).  The extension's set of bound names is pinned, so
  // the mixed reward is a mode of this op, as peer mode is one of cider_score.
  m.def(
      "metric_score",
      [](const std::string& metric, at::Tensor hyps, at::Tensor hyp_video,
         c10::optional<std::map<std::string, at::Tensor>> tables, int64_t use_eos,
         c10::optional<at::Tensor> exclude,
         c10::optional<std::map<std::string, at::Tensor>> cider_tables, double log_ref_len,
         c10::optional<std::vector<double>> weights, int64_t group) -> py::object {
        if (group != 0) {
          // peer mode (--mbr_mix; kernels/peer_mix.hip): hyps is B pools of G rows,
          // every row scored against the others of its pool; cider_tables = the df
          // hash table (ht_keys / ht_vals; None when w_c = 0), tables / hyp_video
          // are not read
          TORCH_CHECK(metric == "mix", "metric_score: peer mode (group > 0) is metric mix, got ",
                      metric);
          TORCH_CHECK(weights.has_value(), "metric_score: metric mix needs weights");
          TORCH_CHECK(!(exclude.has_value() && exclude->defined()),
                      "metric_score: peer mode (group > 0) takes no exclude");
          return py::cast(cst::peer_mix_score(hyps, cider_tables, log_ref_len, use_eos, *weights,
                                              group));
        }
        if (metric == "mix") {
          TORCH_CHECK(weights.has_value(), "metric_score: metric mix needs weights");
          TORCH_CHECK(!(exclude.has_value() && exclude->defined()),
                      "metric_score: metric mix takes no exclude");
          return py::cast(cst::reward_mix_score(hyps, hyp_video, cider_tables, tables,
                                                log_ref_len, use_eos, *weights));
        }
        TORCH_CHECK(tables.has_value(), "metric_score: tables must be given");
        TORCH_CHECK(!weights.has_value() && !cider_tables.has_value(),
                    "metric_score: weights / cider_tables go with metric mix only");
        return py::cast(cst::metric_score(metric, hyps, hyp_video, *tables, use_eos, exclude));
      },
      py::arg("metric"), py::arg("hyps"), py::arg("hyp_video"), py::arg("tables"),
      py::arg("use_eos"), py::arg("exclude") = py::none(), py::arg("cider_tables") = py::none(),
      py::arg("log_ref_len") = 0.0, py::arg("weights") = py::none(), py::arg("group") = 0,
      "Bleu_4 | ROUGE_L sentence scores on the GPU, or their weighted mix with CIDEr-D "
      "(metric mix; group = G >= 2: every row against the others of its pool of G); one "
      "launch, capturable");
  // group = G >= 2 with metric mix: the native twin of the peer mode above,
  // [out (N), parts (N, 3)], any G; group = 0: the sentence scorers, as before
  m.def(
      "metric_score_cpu",
      [](const std::string& metric, at::Tensor hyps, at::Tensor hyp_video,
         c10::optional<std::map<std::string, at::Tensor>> tables, int64_t use_eos,
         c10::optional<at::Tensor> exclude,
         c10::optional<std::map<std::string, at::Tensor>> cider_tables, double log_ref_len,
         c10::optional<std::vector<double>> weights, int64_t group) -> py::object {
        if (group != 0) {
          TORCH_CHECK(metric == "mix",
                      "metric_score_cpu: peer mode (group > 0) is metric mix, got ", metric);
          TORCH_CHECK(weights.has_value(), "metric_score_cpu: metric mix needs weights");
          TORCH_CHECK(!(exclude.has_value() && exclude->defined()),
                      "metric_score_cpu: peer mode (group > 0) takes no exclude");
          return py::cast(cst::peer_mix_score_cpu(hyps, cider_tables, log_ref_len, use_eos,
                                                  *weights, group));
        }
        TORCH_CHECK(!weights.has_value() && !cider_tables.has_value(),
                    "metric_score_cpu: weights / cider_tables go with peer mode (metric mix, "
                    "group > 0) only");
        TORCH_CHECK(tables.has_value(), "metric_score_cpu: tables must be given");
        return py::cast(cst::metric_score_cpu(metric, hyps, hyp_video, *tables, use_eos, exclude));
      },
      py::arg("metric"), py::arg("hyps"), py::arg("hyp_video"), py::arg("tables"),
      py::arg("use_eos"), py::arg("exclude") = py::none(), py::arg("cider_tables") = py::none(),
      py::arg("log_ref_len") = 0.0, py::arg("weights") = py::none(), py::arg("group") = 0);
  // ema (none or empty: off) / ema_decay: the parameter EMA kept by the update pass
  m.def("flat_adam_step", &cst::flat_adam_step, py::arg("p"), py::arg("g"), py::arg("m"),
        py::arg("v"), py::arg("partials"), py::arg("scal"), py::arg("skip"), py::arg("hyper"),
        py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("clip"), py::arg("gscale"),
        py::arg("phase"), py::arg("shadow_meta"), py::arg("shadow_dst"),
        py::arg("ema") = py::none(), py::arg("ema_decay") = 0.0);
  // swap_with: p and swap_with are exchanged, the shadows written from the new p
  m.def("refresh_shadows", &cst::refresh_shadows, py::arg("p"), py::arg("shadow_meta"),
        py::arg("shadow_dst"), py::arg("swap_with") = py::none());
  m.def("vocab_fwd_bench", &cst::vocab_fwd_bench);
  m.def("vgrad_colsum_bench", &cst::vgrad_colsum_bench);
  m.def("token_sort_bench", &cst::token_sort_bench);
  m.def("att_bench", &cst::att_bench);
  m.def("token_sort", &cst::token_sort);
  m.def("token_group_sum", &cst::token_group_sum);
  // top_k > 0: the VF_TOPK vocab launch + topk_sample_kernel -> (tok, lse, lp)
  // ens_logits given: kernels/ensemble.hip alone instead (cst::ensemble_topk_test; the
  // other operands are not read) -> (top_v, top_i[, tok, lp, next_tok])
  m.def(
      "vocab_select",
      [](at::Tensor hd, at::Tensor wlog, at::Tensor blog, at::Tensor rng, int64_t mode,
         double temperature, int64_t step, int64_t top_k, double top_p,
         std::vector<at::Tensor> ens_logits, std::vector<at::Tensor> ens_lse,
         std::vector<double> ens_logw, int64_t ens_V, int64_t ens_K,
         c10::optional<at::Tensor> ens_unfinished, bool ens_baseline) {
        if (!ens_logits.empty() || !ens_lse.empty() || !ens_logw.empty())
          return cst::ensemble_topk_test(ens_logits, ens_lse, ens_logw, ens_V, ens_K,
                                         ens_unfinished, ens_baseline);
        return cst::vocab_select(hd, wlog, blog, rng, mode, temperature, step, top_k, top_p);
      },
      py::arg("hd"), py::arg("wlog"), py::arg("blog"), py::arg("rng"), py::arg("mode"),
      py::arg("temperature"), py::arg("step"), py::arg("top_k") = 0, py::arg("top_p") = 1.0,
      py::arg("ens_logits") = std::vector<at::Tensor>(),
      py::arg("ens_lse") = std::vector<at::Tensor>(),
      py::arg("ens_logw") = std::vector<double>(), py::arg("ens_V") = 0, py::arg("ens_K") = 0,
      py::arg("ens_unfinished") = py::none(), py::arg("ens_baseline") = false);
  m.def("decode_step_test", &cst::decode_step_test, py::arg("hd"), py::arg("h"), py::arg("wlog"),
        py::arg("blog"), py::arg("whh"), py::arg("vgate"), py::arg("vdiv"), py::arg("tgt"),
        py::arg("eoff"), py::arg("save"), py::arg("mode"), py::arg("step"), py::arg("rng"),
        py::arg("ptab"), py::arg("c_prev"), py::arg("drop_p"), py::arg("cell"), py::arg("eos"),
        py::arg("unfinished"), py::arg("ss_prob"), py::arg("want_xe") = true);
  m.def("gemm_bf16_tuned", &cst::gemm_bf16_tuned, py::arg("out"), py::arg("a"), py::arg("ta"),
        py::arg("b"), py::arg("tb"), py::arg("n_cand") = 24);
  m.def("gemm_bf16_tuned_batched", &cst::gemm_bf16_tuned_batched, py::arg("out"), py::arg("a"),
        py::arg("ta"), py::arg("b"), py::arg("tb"), py::arg("n_cand") = 24);
  m.def("gemm_tuned_timings", &cst::gemm_tuned_timings);
  m.def("gemm_tuned_choices", &cst::gemm_tuned_choices);
  m.def("set_grad_events", &cst::set_grad_events);
  m.def("grad_event_wait", &cst::grad_event_wait);
  m.def("grad_event_record", &cst::grad_event_record);
  m.def("grad_event_count", &cst::grad_event_count);
  m.def("set_poll_bound", &cst::set_poll_bound,
        "polls of a bounded cross-workgroup wait before it gives up (tests: 0)");
  m.def("set_bwd_loop", &cst::set_bwd_loop,
        "reverse LSTM loop: 1 one persistent launch, row-read form (default); 2 persistent, "
        "K-split team GEMM; 0 one launch per step");
  m.def("lstm_bwd_loop_bench", &cst::lstm_bwd_loop_bench, py::arg("R"), py::arg("H"), py::arg("T"),
        py::arg("iters"), py::arg("phases"), py::arg("dbg") = 0,
        "persistent reverse loop alone on random operands: us per launch (+ phase stamps)");
  m.def("set_att_fuse", &cst::set_att_fuse,
        "attention backward fused into the reverse step (true, default) or a launch per step");
  m.def("device_errors", &cst::device_errors,
        "failed cross-workgroup hand-offs counted on the device (synchronous read)");
  m.def("reset_device_errors", &cst::reset_device_errors);
  m.def("att_mfma_fwd", &cst::att_mfma_fwd, py::arg("h"), py::arg("wq"), py::arg("P"),
        py::arg("wa"), py::arg("ba"), py::arg("gv"), py::arg("whole") = -1);
  // rows_per_video > 0: truncated sampling instead (K = top_k, see beam_search.cpp)
  m.def("beam_search", &cst::beam_search, py::arg("wx"), py::arg("ptab"), py::arg("whh"),
        py::arg("wlog"), py::arg("blog"), py::arg("vgate"), py::arg("K"), py::arg("T"),
        py::arg("bos_index"), py::arg("att"), py::arg("cell"), py::arg("state0"), py::arg("up"),
        py::arg("rows_per_video") = 0, py::arg("top_p") = 1.0, py::arg("temperature") = 1.0,
        py::arg("rng") = py::none(),
        // ens_weights given (M log-weights, host): ensemble decoding, this call's operands
        // are member 0 and ensemble = the packs of members 1..M-1 ({wx, ptab, whh, wlog,
        // blog, vgate, meta, att.., state0.., up..}); ens_greedy: greedy decode, K unused
        py::arg("ensemble") = std::vector<std::vector<at::Tensor>>(),
        py::arg("ens_weights") = std::vector<double>(), py::arg("ens_greedy") = false);
  // idx / C: optional int64 row index into resident feature tables (C frames per row)
  m.def("featpool_forward", &cst::featpool_forward, py::arg("xs"), py::arg("ws"), py::arg("bs"),
        py::arg("drop_p"), py::arg("rng"), py::arg("idx") = py::none(), py::arg("C") = 1);
  m.def("featpool_forward16", &cst::featpool_forward16, py::arg("xs"), py::arg("ws"),
        py::arg("bs"), py::arg("drop_p"), py::arg("rng"), py::arg("idx") = py::none(),
        py::arg("C") = 1);
  m.def("scst_loss_forward", &cst::scst_loss_forward);
  // objective 1 risk / 2 softmax_margin / 3 multi_margin: the group loss over each video's S
  // rows (bref, k unused), a 4th result = the row weights scst_loss_backward's row_weight takes
  m.def("cst_loss_forward", &cst::cst_loss_forward, py::arg("seq"), py::arg("lp"),
        py::arg("scores"), py::arg("bref"), py::arg("S"), py::arg("k"), py::arg("objective") = 0,
        py::arg("alpha") = 1.0, py::arg("cost_scale") = 1.0);
  m.def("scst_loss_backward", &cst::scst_loss_backward, py::arg("seq"), py::arg("reward"),
        py::arg("out"), py::arg("dloss"), py::arg("row_weight") = py::none());
  m.def("xe_loss_forward", &cst::xe_loss_forward);
  m.def("xe_loss_backward", &cst::xe_loss_backward);
  m.def("featpool_backward", &cst::featpool_backward, py::arg("dout"), py::arg("out"),
        py::arg("xs"), py::arg("ws"), py::arg("drop_p"), py::arg("outs"),
        py::arg("idx") = py::none(), py::arg("C") = 1);
  m.def("set_stamp_base", &cst::set_stamp_base);
  m.def("stamp_buffer", &cst::stamp_buffer);
  m.def("stamp_now", &cst::stamp_now);
  m.def("busy_copy", &cst::busy_copy,
        "stand-in for a collective's kernel: copying workgroups for a given time");
  m.def("wall_clock_khz", &cst::wall_clock_khz);
  m.def("vocab_x", &cst::vocab_x);
  m.def("att_mfma_phases", &cst::att_mfma_phases);
  m.def("wgrad_tn", &cst::wgrad_tn);
  m.def("wgrad_tn_colsum", &cst::wgrad_tn_colsum);
  m.def("wgrad_tn_rows", &cst::wgrad_tn_rows);
  // the backward's gradient-assembly kernels one by one (tests); empty tensors = not given
  m.def("vgrad_fold", &cst::vgrad_fold, py::arg("E"), py::arg("lse"), py::arg("y_sel"),
        py::arg("dg_sel"), py::arg("labels"), py::arg("dg_xe"), py::arg("V"),
        py::arg("zero_off"), py::arg("hd"), py::arg("wlog"), py::arg("blog"),
        py::arg("fix_total"), py::arg("forward_x"), py::arg("X"), py::arg("ls_eps") = 0.0,
        py::arg("ls_wbar") = py::none());
  m.def("vgrad_rows", &cst::vgrad_rows, py::arg("alpha"), py::arg("hd"), py::arg("ldhs"),
        py::arg("dhd"));
  // ls_mode 1 / 2 / 3: label smoothing's column mean, rank-1 sums (+ the broadcast add) and
  // smoothed log-prob kernels (dev_entries.cpp)
  m.def("vgrad_colsum", &cst::vgrad_colsum, py::arg("E"), py::arg("alpha"), py::arg("V"),
        py::arg("ls_mode") = 0, py::arg("ls_eps") = 0.0, py::arg("ls_dg") = py::none(),
        py::arg("ls_dw") = py::none(), py::arg("ls_db") = py::none());
  m.def("video_gate_grad", &cst::video_gate_grad);
  // the reverse recurrence's kernels one by one (tests); None / empty tensors = not given
  m.def("lstm_step_bwd_test", &cst::lstm_step_bwd_test, py::arg("dg_next"), py::arg("whhT"),
        py::arg("dh_logit"), py::arg("dc_carry"), py::arg("gates"), py::arg("c_t"),
        py::arg("c_prev"), py::arg("drop_p"), py::arg("rng"), py::arg("step"), py::arg("cell"),
        py::arg("KD"), py::arg("sentinel"), py::arg("dh_scale") = py::none(),
        py::arg("oh_W") = py::none(), py::arg("oh_a") = py::none(), py::arg("oh_ys") = py::none(),
        py::arg("oh_b") = py::none(), py::arg("oh_yx") = py::none(),
        py::arg("gvb16") = py::none(), py::arg("vdiv") = 1, py::arg("C") = 0);
  m.def("lstm_bwd_loop_test", &cst::lstm_bwd_loop_test, py::arg("whhT"), py::arg("dh"),
        py::arg("gates"), py::arg("c_all"), py::arg("drop_p"), py::arg("rng"), py::arg("cell"),
        py::arg("form"), py::arg("scale") = py::none(), py::arg("oh_W") = py::none(),
        py::arg("oh_a") = py::none(), py::arg("oh_ys") = py::none(), py::arg("oh_b") = py::none(),
        py::arg("oh_yx") = py::none());
}
