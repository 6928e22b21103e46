// Native host side of the sentence-level BLEU-4 / ROUGE-L rewards (no torch
// dependency).
//
//  * build_metric_tables: once per dataset, reduces every GT label row as
//    utils/text.py::sequence_tokens does (BOS dropped anywhere, stop at the
//    first EOS, that 0 kept when use_eos) and builds, per video, the sorted
//    union of the references' packed n-grams with their clip counts (BLEU; and
//    for leave-one-out scoring the clip count without its only holder) and the
//    ragged reference token rows (ROUGE).
//  * bleu4_score_host / rouge_l_score_host: the scorers of eval/metrics.py
//    (Bleu per-sentence scores, Rouge.calc_score) on those tables, integer
//    counts and fp64 formulas rounded once to fp32.  They are the
//    backend='cpu' scorer and a second oracle of the GPU kernels
//    (csrc/kernels/sent_metrics.hip).
//  * bleu_stats_host / meteor_stats_host: the validation scorer's per-hypothesis
//    statistics (twins of csrc/kernels/corpus_metrics.hip).
#include "metric_host.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>

#include "../cider_common.h"

namespace cst {

static void reduce_tokens(const int64_t* row, int T, int use_eos, bool check_pack,
                          const char* what, std::vector<int>& out) {
  out.clear();
  for (int i = 0; i < T; ++i) {
    const int64_t t = row[i];
    if (t == 0) {
      if (use_eos) out.push_back(0);
      return;
    }
    if (t == 1) continue;
    if (t < 0 || (check_pack && t > METRIC_MAX_TOKEN))
      throw std::invalid_argument(std::string(what) + " token id " + std::to_string(t) +
                                  " outside [0, 65534]: the packed n-gram keys hold 16 bits "
                                  "per token");
    out.push_back((int)t);
  }
}

static void count_ngrams(const std::vector<int>& toks, std::map<uint64_t, int>& cnt) {
  cnt.clear();
  const int W = (int)toks.size();
  for (int n = 1; n <= 4; ++n)
    for (int i = 0; i + n <= W; ++i) {
      uint64_t key = 0;
      for (int j = 0; j < n; ++j) key |= (uint64_t)(toks[i + j] + 1) << (16 * j);
      cnt[key] += 1;
    }
}

MetricTables build_metric_tables(const int64_t* labels, int M, int L, const int64_t* start,
                                 const int64_t* end, int Nv, int use_eos,
                                 const int32_t* stem_ids, int V) {
  MetricTables t;
  t.vid_ref_off.resize(Nv + 1);
  t.vid_ng_off.resize(Nv + 1);
  t.ref_tok_off.push_back(0);
  std::vector<int> toks;
  std::map<uint64_t, int> grams;
  struct Clip {
    int m1 = 0, m2 = 0, arg = -1;  // max count, the others' max, its only holder
  };
  std::map<uint64_t, Clip> maxc;
  int nref = 0;
  for (int v = 0; v < Nv; ++v) {
    t.vid_ref_off[v] = nref;
    t.vid_ng_off[v] = (int32_t)t.ng_key.size();
    if (start[v] < 0 || end[v] > M)
      throw std::invalid_argument("label range of video " + std::to_string(v) +
                                  " lies outside the label table");
    maxc.clear();
    for (int64_t r = start[v]; r < end[v]; ++r) {
      reduce_tokens(labels + r * L, L, use_eos, true, "reference", toks);
      if ((int)toks.size() > METRIC_MAXT)
        throw std::invalid_argument("reference " + std::to_string(r) + " has " +
                                    std::to_string(toks.size()) + " tokens; at most 64 are "
                                    "supported");
      count_ngrams(toks, grams);
      const int idx = (int)(r - start[v]);
      for (auto& g : grams) {
        Clip& c = maxc[g.first];
        if (g.second > c.m1)
          c.m2 = c.m1, c.m1 = g.second, c.arg = idx;
        else if (g.second == c.m1)
          c.m2 = c.m1, c.arg = -1;
        else
          c.m2 = std::max(c.m2, g.second);
      }
      t.ref_len.push_back((int32_t)toks.size());
      t.ref_tok.insert(t.ref_tok.end(), toks.begin(), toks.end());
      if (stem_ids) {
        for (int tok : toks) {
          if (tok >= V)
            throw std::invalid_argument("reference token id " + std::to_string(tok) +
                                        " outside the vocabulary of " + std::to_string(V) +
                                        " stem ids");
          t.ref_stem.push_back(stem_ids[tok]);
        }
      }
      t.ref_tok_off.push_back((int32_t)t.ref_tok.size());
      ++nref;
    }
    for (auto& g : maxc) {  // (std::map: ascending keys)
      t.ng_key.push_back((int64_t)g.first);
      t.ng_cnt.push_back(g.second.m1);
      t.ng_cnt2.push_back(g.second.m2);
      t.ng_arg.push_back(g.second.arg);
    }
  }
  t.vid_ref_off[Nv] = nref;
  t.vid_ng_off[Nv] = (int32_t)t.ng_key.size();
  return t;
}

static void check_hyps(int T, const int64_t* hyp_video, int N, int Nv) {
  if (T > METRIC_MAXT)
    throw std::invalid_argument("hypotheses of " + std::to_string(T) +
                                " tokens; at most 64 are supported");
  for (int i = 0; i < N; ++i)
    if (hyp_video[i] < 0 || hyp_video[i] >= Nv)
      throw std::invalid_argument("video index " + std::to_string(hyp_video[i]) +
                                  " outside the tables");
}

// correct[4], tlen, rlen of one reduced hypothesis against video v (with
// references): clipped n-gram matches against the union table, closest
// reference length with ties to the shorter.  ex: the (absolute) reference left
// out, -1 for none.
static void bleu_counts(const std::vector<int>& toks, const MetricTablesView& t, int v,
                        std::map<uint64_t, int>& grams, int correct[4], int& tlen, int& rlen,
                        int ex = -1) {
  const int r0 = t.vid_ref_off[v], r1 = t.vid_ref_off[v + 1];
  count_ngrams(toks, grams);
  const int64_t* k0 = t.ng_key + t.vid_ng_off[v];
  const int64_t* k1 = t.ng_key + t.vid_ng_off[v + 1];
  for (int k = 0; k < 4; ++k) correct[k] = 0;
  for (auto& g : grams) {
    // (ascending as uint64: a 4-gram whose last token is >= 32767 has bit 63 set)
    const int64_t* p = std::lower_bound(
        k0, k1, (int64_t)g.first,
        [](int64_t a, int64_t b) { return (uint64_t)a < (uint64_t)b; });
    if (p != k1 && *p == (int64_t)g.first) {
      const int64_t at = p - t.ng_key;
      const int clip = (ex >= 0 && t.ng_arg[at] == ex - r0) ? t.ng_cnt2[at] : t.ng_cnt[at];
      correct[ngram_order(g.first) - 1] += std::min(g.second, clip);
    }
  }
  tlen = (int)toks.size();
  // closest reference length, ties to the shorter: min over (|len_r - tlen|, len_r)
  int best_d = 1 << 30;
  rlen = 0;
  for (int r = r0; r < r1; ++r) {
    if (r == ex) continue;
    const int d = std::abs(t.ref_len[r] - tlen);
    if (d < best_d || (d == best_d && t.ref_len[r] < rlen)) best_d = d, rlen = t.ref_len[r];
  }
}

void bleu4_score_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                      const MetricTablesView& t, int use_eos, float* out,
                      const int64_t* exclude) {
  check_hyps(T, hyp_video, N, t.Nv);
  // (an empty n-gram table has no rows to hold them)
  if (exclude && (!t.ng_cnt2 || !t.ng_arg) && t.vid_ng_off[t.Nv] > 0)
    throw std::invalid_argument("leave-one-out BLEU needs tables with ng_cnt2 / ng_arg");
  const double tiny = 1e-15, small = 1e-9;
  std::vector<int> toks;
  std::map<uint64_t, int> grams;
  for (int i = 0; i < N; ++i) {
    reduce_tokens(hyps + (int64_t)i * T, T, use_eos, true, "hypothesis", toks);
    const int v = (int)hyp_video[i];
    if (t.vid_ref_off[v + 1] <= t.vid_ref_off[v]) {
      out[i] = 0.f;
      continue;
    }
    int correct[4], tlen, rlen;
    bleu_counts(toks, t, v, grams, correct, tlen, rlen,
                excluded_ref(exclude, i, t.vid_ref_off[v], t.vid_ref_off[v + 1]));
    double b = 1.0;
    for (int k = 0; k < 4; ++k) b *= (correct[k] + tiny) / (std::max(0, tlen - k) + small);
    double s = std::pow(b, 0.25);
    const double ratio = (tlen + tiny) / (rlen + small);
    if (ratio < 1) s *= std::exp(1 - 1 / ratio);
    out[i] = (float)s;
  }
}

void bleu_stats_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                     const MetricTablesView& t, int32_t* out) {
  check_hyps(T, hyp_video, N, t.Nv);
  std::vector<int> toks;
  std::map<uint64_t, int> grams;
  for (int i = 0; i < N; ++i) {
    reduce_tokens(hyps + (int64_t)i * T, T, 0, true, "hypothesis", toks);
    const int v = (int)hyp_video[i];
    int correct[4] = {0, 0, 0, 0}, tlen = (int)toks.size(), rlen = 0;
    if (t.vid_ref_off[v + 1] > t.vid_ref_off[v]) bleu_counts(toks, t, v, grams, correct, tlen, rlen);
    int32_t* o = out + (int64_t)i * 10;
    for (int k = 0; k < 4; ++k) o[k] = correct[k], o[4 + k] = std::max(0, tlen - k);
    o[8] = tlen;
    o[9] = rlen;
  }
}

// Meteor._score (eval/metrics.py): alpha .85, beta .2, gamma .6, stem weight .6
double meteor_score_host(int n_exact, int n_stem, int len_h, int len_r, int chunks) {
  const int np = n_exact + n_stem;
  const double m = (double)n_exact + 0.6 * (double)n_stem;
  if (np <= 0 || len_h <= 0 || len_r <= 0) return 0.0;
  const double P = m / (double)len_h, R = m / (double)len_r;
  const double fmean = P * R / (0.85 * P + (1.0 - 0.85) * R);
  const double frag = (double)chunks / (double)np;
  const double pen = 0.6 * std::pow(frag, 0.2);
  return (1.0 - pen) * fmean;
}

void meteor_stats_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                       const MetricTablesView& t, const int32_t* ref_stem,
                       const int32_t* stem_ids, int V, int32_t* out_stats, double* out_score,
                       const int64_t* exclude) {
  check_hyps(T, hyp_video, N, t.Nv);
  std::vector<int> toks, hkey, pair_j;
  std::vector<char> used;
  for (int i = 0; i < N; ++i) {
    reduce_tokens(hyps + (int64_t)i * T, T, 0, false, "hypothesis", toks);
    const int W = (int)toks.size();
    const int v = (int)hyp_video[i];
    const int r0 = t.vid_ref_off[v], r1 = t.vid_ref_off[v + 1];
    int best[4] = {0, 0, 0, 0};  // n_exact, n_stem, len_r, chunks
    double best_score = -1.0;
    const int ex = excluded_ref(exclude, i, r0, r1);
    for (int r = r0; r < r1; ++r) {
      if (r == ex) continue;
      const int o0 = t.ref_tok_off[r];
      const int n = t.ref_tok_off[r + 1] - o0;
      pair_j.assign(W, -1);
      used.assign(n, 0);
      int cnt[2] = {0, 0};
      for (int stage = 0; stage < 2; ++stage) {
        const int32_t* rkey = (stage ? ref_stem : t.ref_tok) + o0;
        hkey.resize(W);
        for (int a = 0; a < W; ++a)  // (-1: no stem known, matches nothing)
          hkey[a] = !stage ? toks[a] : (toks[a] < V ? stem_ids[toks[a]] : -1);
        for (int a = 0; a < W; ++a) {
          if (pair_j[a] >= 0 || hkey[a] < 0) continue;
          int want = 0;
          for (int p = a - 1; p >= 0; --p)
            if (pair_j[p] >= 0) {
              want = pair_j[p] + 1;
              break;
            }
          int bj = -1, bd = 1 << 30;
          for (int j = 0; j < n; ++j) {  // (ascending j: the smaller j on equal distance)
            if (used[j] || rkey[j] != hkey[a]) continue;
            const int d = std::abs(j - want);
            if (d < bd) bd = d, bj = j;
          }
          if (bj < 0) continue;
          used[bj] = 1;
          pair_j[a] = bj;
          cnt[stage] += 1;
        }
      }
      int chunks = 0;
      for (int a = 0; a < W; ++a)
        if (pair_j[a] >= 0 && !(a > 0 && pair_j[a - 1] >= 0 && pair_j[a - 1] + 1 == pair_j[a]))
          ++chunks;
      const double sc = meteor_score_host(cnt[0], cnt[1], W, n, chunks);
      if (sc > best_score) {
        best_score = sc;
        best[0] = cnt[0], best[1] = cnt[1], best[2] = n, best[3] = chunks;
      }
    }
    int32_t* o = out_stats + (int64_t)i * 6;
    const bool any = r1 > r0;
    o[0] = best[0], o[1] = best[1], o[2] = any ? W : 0, o[3] = best[2], o[4] = best[3];
    o[5] = best[0] + best[1];
    out_score[i] = any ? best_score : 0.0;
  }
}

void rouge_l_score_host(const int64_t* hyps, int N, int T, const int64_t* hyp_video,
                        const MetricTablesView& t, int use_eos, float* out,
                        const int64_t* exclude) {
  check_hyps(T, hyp_video, N, t.Nv);
  const double beta = 1.2, b2 = beta * beta;
  std::vector<int> toks, prev, cur;
  for (int i = 0; i < N; ++i) {
    reduce_tokens(hyps + (int64_t)i * T, T, use_eos, false, "hypothesis", toks);
    const int v = (int)hyp_video[i];
    const int W = (int)toks.size();
    double p = 0, rc = 0;
    const int ex = excluded_ref(exclude, i, t.vid_ref_off[v], t.vid_ref_off[v + 1]);
    for (int r = t.vid_ref_off[v]; r < t.vid_ref_off[v + 1]; ++r) {
      if (r == ex) continue;
      const int32_t* ref = t.ref_tok + t.ref_tok_off[r];
      const int n = t.ref_tok_off[r + 1] - t.ref_tok_off[r];
      prev.assign(W + 1, 0);
      for (int a = 0; a < n; ++a) {
        cur.assign(W + 1, 0);
        for (int j = 0; j < W; ++j)
          cur[j + 1] = ref[a] == toks[j] ? prev[j] + 1 : std::max(prev[j + 1], cur[j]);
        prev.swap(cur);
      }
      const int l = prev[W];
      if (W > 0) p = std::max(p, l / (double)W);
      if (n > 0) rc = std::max(rc, l / (double)n);
    }
    out[i] = (p != 0 && rc != 0) ? (float)(((1 + b2) * p * rc) / (rc + b2 * p)) : 0.f;
  }
}

}  // namespace cst
