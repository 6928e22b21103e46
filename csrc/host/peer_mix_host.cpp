// Native twin of csrc/kernels/peer_mix.hip (no torch dependency): peer scores
// under a mixed utility for consensus / MBR decoding (--mbr_mix).  The
// references of a row are the other rows of its pool, so no table is built:
// CIDEr-D is cider_peers_host, BLEU-4 and ROUGE-L are computed directly from
// the pool's n-gram counts and token rows, integer statistics and the fp64
// formulas of bleu4_score_host / rouge_l_score_host rounded once to fp32.
// Declared in metric_host.h.
#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>

#include "../cider_common.h"
#include "cider_host.h"
#include "metric_host.h"

namespace cst {

// (as metric_host.cpp: BOS dropped anywhere, stop at the first EOS, that 0 kept
// when use_eos; check_pack: a token the 16-bit packing cannot hold is refused)
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

void peer_mix_host(const int64_t* hyps, int N, int T, int G, const int64_t* ht_keys,
                   const float* ht_vals, uint32_t ht_cap, double log_ref_len, int use_eos,
                   const double w[3], float* out, float* parts) {
  if (G < 2 || N < 0 || N % G != 0)
    throw std::invalid_argument("peer_mix_host: N rows in pools of G >= 2");
  if (T > METRIC_MAXT)
    throw std::invalid_argument("hypotheses of " + std::to_string(T) +
                                " tokens; at most 64 are supported");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(w[k]) || w[k] < 0)
      throw std::invalid_argument("peer_mix_host: weight " + std::to_string(w[k]) +
                                  " is negative or not finite");
  const float wf[3] = {(float)w[0], (float)w[1], (float)w[2]};
  const bool has_c = wf[0] != 0.f, has_b = wf[1] != 0.f, has_r = wf[2] != 0.f;
  if (!has_c && !has_b && !has_r)
    throw std::invalid_argument("peer_mix_host: all weights are zero");
  if (has_c && (!ht_keys || !ht_vals || ht_cap == 0))
    throw std::invalid_argument("peer_mix_host: CIDEr has a weight but no df table");
  for (int64_t i = 0; i < (int64_t)N * 3; ++i) parts[i] = 0.f;
  std::vector<std::vector<int>> toks((size_t)G);
  if (has_c) {
    // (the packed keys of CIDEr-D hold 16 bits per token, as BLEU's)
    for (int i = 0; i < N; ++i)
      reduce_tokens(hyps + (int64_t)i * T, T, use_eos, true, "hypothesis", toks[0]);
    std::vector<float> c((size_t)N);
    cider_peers_host(hyps, N, T, G, ht_keys, ht_vals, ht_cap, log_ref_len, use_eos, c.data());
    for (int i = 0; i < N; ++i) parts[(int64_t)i * 3] = c[i];
  }
  const double tiny = 1e-15, small = 1e-9, beta = 1.2, b2 = beta * beta;
  std::vector<std::map<uint64_t, int>> grams((size_t)G);
  std::vector<int> prev, cur;
  for (int p0 = 0; p0 < N && (has_b || has_r); p0 += G) {
    for (int r = 0; r < G; ++r) {
      reduce_tokens(hyps + (int64_t)(p0 + r) * T, T, use_eos, has_b, "hypothesis", toks[r]);
      if (has_b) count_ngrams(toks[r], grams[r]);
    }
    for (int i = 0; i < G; ++i) {
      const std::vector<int>& h = toks[i];
      const int W = (int)h.size();
      float* o = parts + (int64_t)(p0 + i) * 3;
      if (has_b) {
        int correct[4] = {0, 0, 0, 0};
        for (auto& g : grams[i]) {
          int clip = 0;  // the largest count of the n-gram among the peers
          for (int j = 0; j < G; ++j) {
            if (j == i) continue;
            auto it = grams[j].find(g.first);
            if (it != grams[j].end()) clip = std::max(clip, it->second);
          }
          correct[ngram_order(g.first) - 1] += std::min(g.second, clip);
        }
        // closest peer length, ties to the shorter
        int best_d = 1 << 30, rlen = 0;
        for (int j = 0; j < G; ++j) {
          if (j == i) continue;
          const int lr = (int)toks[j].size(), d = std::abs(lr - W);
          if (d < best_d || (d == best_d && lr < rlen)) best_d = d, rlen = lr;
        }
        double b = 1.0;
        for (int k = 0; k < 4; ++k) b *= (correct[k] + tiny) / (std::max(0, W - k) + small);
        double s = std::pow(b, 0.25);
        const double ratio = (W + tiny) / (rlen + small);
        if (ratio < 1) s *= std::exp(1 - 1 / ratio);
        o[1] = (float)s;
      }
      if (has_r) {
        double p = 0, rc = 0;
        for (int j = 0; j < G; ++j) {
          if (j == i) continue;
          const std::vector<int>& ref = toks[j];
          const int n = (int)ref.size();
          prev.assign(W + 1, 0);
          for (int a = 0; a < n; ++a) {
            cur.assign(W + 1, 0);
            for (int q = 0; q < W; ++q)
              cur[q + 1] = ref[a] == h[q] ? prev[q] + 1 : std::max(prev[q + 1], cur[q]);
            prev.swap(cur);
          }
          const int l = prev[W];
          if (W > 0) p = std::max(p, l / (double)W);
          if (n > 0) rc = std::max(rc, l / (double)n);
        }
        o[2] = (p != 0 && rc != 0) ? (float)(((1 + b2) * p * rc) / (rc + b2 * p)) : 0.f;
      }
    }
  }
  for (int i = 0; i < N; ++i) {  // (fp32, each product and sum rounded once, as the kernel)
    const float* o = parts + (int64_t)i * 3;
    const volatile float pc = wf[0] * o[0], pb = wf[1] * o[1], pr = wf[2] * o[2];
    const volatile float cb = pc + pb;
    out[i] = cb + pr;
  }
}

}  // namespace cst
