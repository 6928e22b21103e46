// Host-side driver for peer scoring under a mixed utility
// (csrc/host/peer_mix_host.cpp: peer_mix_host, the twin of
// csrc/kernels/peer_mix.hip), built with AddressSanitizer + UBSan by
// tests/test_native_peer_mix_sanitizers.py.
//
// Every pool is scored twice: by peer_mix_host, and by the construction that
// defines the feature -- the pool rows as the reference table of one video
// (build_metric_tables), every row scored by bleu4_score_host / rouge_l_score_host
// with its own row excluded (exclude[i] = i mod G).  Both routes count the same
// integers and close with the same fp64 formulas, so BLEU-4 and ROUGE-L agree
// exactly; the CIDEr-D column is cider_peers_host's and the blend is recomputed.
// Pools of 2, 3, 5, 21, 64 and 100 rows, widths 1, 5, 31, 63 and 64, a tiny
// vocabulary (tf > 1, duplicate rows), empty rows, rows of BOS only, full-width
// rows without EOS, empty batches, both use_eos settings, zero weights.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "host/cider_host.h"
#include "host/metric_host.h"

using namespace cst;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

int main() {
  std::mt19937 rng(4321);
  // df table over unigrams and bigrams of tokens 2..9 (the rest: df 0)
  std::vector<int64_t> df_keys;
  std::vector<float> df_vals;
  for (int a = 2; a < 10; ++a) {
    df_keys.push_back(a + 1);
    df_vals.push_back((float)(1 + rng() % 40));
    for (int b = 2; b < 10; b += 2) {
      df_keys.push_back((int64_t)(a + 1) | ((int64_t)(b + 1) << 16));
      df_vals.push_back((float)(1 + rng() % 10));
    }
  }
  const double log_ref_len = std::log(50.0);
  CiderTables ct = build_cider_tables(nullptr, 0, 1, nullptr, nullptr, 0, df_keys.data(),
                                      df_vals.data(), (int)df_keys.size(), log_ref_len, 0);
  const int Gs[] = {2, 3, 5, 21, 64, 100};
  const int Ts[] = {1, 5, 31, 63, 64};
  const double W[][3] = {{1, 5, 5}, {0, 3, 0}, {1, 0, 0}};
  int pools = 0;
  for (int use_eos = 0; use_eos < 2; ++use_eos) {
    for (int G : Gs) {
      for (int T : Ts) {
        if (G == 100 && T != 5 && T != 64) continue;  // (the large pools: two widths)
        const int B = G > 21 ? 1 : 3, N = B * G;
        std::vector<int64_t> hyps((size_t)N * T);
        for (int i = 0; i < N; ++i) {
          const int kind = (int)(rng() % 10);
          const int len = kind == 0 ? 0 : kind == 1 ? T : (int)(rng() % (T + 1));
          for (int t = 0; t < T; ++t) {
            int64_t tok = t < len ? 2 + (int64_t)(rng() % 12) : 0;  // (1: a BOS now and then)
            if (t < len && rng() % 9 == 0) tok = 1;
            if (kind == 2) tok = 1;  // BOS only
            hyps[(size_t)i * T + t] = tok;
          }
          if (i % G && rng() % 4 == 0)  // a duplicate of the previous row of the pool
            for (int t = 0; t < T; ++t) hyps[(size_t)i * T + t] = hyps[(size_t)(i - 1) * T + t];
        }
        std::vector<int64_t> start(B), end(B), vid(N), ex(N);
        for (int b = 0; b < B; ++b) start[b] = (int64_t)b * G, end[b] = (int64_t)(b + 1) * G;
        for (int i = 0; i < N; ++i) vid[i] = i / G, ex[i] = i % G;
        MetricTables mt = build_metric_tables(hyps.data(), N, T, start.data(), end.data(), B,
                                              use_eos);
        const MetricTablesView mv = view_of(mt);
        std::vector<float> wb(N, -1.f), wr(N, -1.f), wc(N, -1.f);
        bleu4_score_host(hyps.data(), N, T, vid.data(), mv, use_eos, wb.data(), ex.data());
        rouge_l_score_host(hyps.data(), N, T, vid.data(), mv, use_eos, wr.data(), ex.data());
        cider_peers_host(hyps.data(), N, T, G, ct.ht_keys.data(), ct.ht_vals.data(), ct.ht_cap,
                         log_ref_len, use_eos, wc.data());
        for (const double* w : W) {
          std::vector<float> out(N, -2.f), parts((size_t)N * 3, -2.f);
          const bool df = w[0] != 0;  // (no CIDEr: no df table is passed at all)
          peer_mix_host(hyps.data(), N, T, G, df ? ct.ht_keys.data() : nullptr,
                        df ? ct.ht_vals.data() : nullptr, df ? ct.ht_cap : 0, log_ref_len,
                        use_eos, w, out.data(), parts.data());
          for (int i = 0; i < N; ++i) {
            const float c = parts[(size_t)i * 3], b = parts[(size_t)i * 3 + 1],
                        r = parts[(size_t)i * 3 + 2];
            CHECK(c == (w[0] != 0 ? wc[i] : 0.f), "G %d T %d eos %d row %d: CIDEr-D %.9g, want %.9g",
                  G, T, use_eos, i, c, wc[i]);
            CHECK(b == (w[1] != 0 ? wb[i] : 0.f), "G %d T %d eos %d row %d: BLEU %.9g, table %.9g",
                  G, T, use_eos, i, b, wb[i]);
            CHECK(r == (w[2] != 0 ? wr[i] : 0.f), "G %d T %d eos %d row %d: ROUGE %.9g, table %.9g",
                  G, T, use_eos, i, r, wr[i]);
            CHECK(b >= 0.f && b <= 1.f && r >= 0.f && r <= 1.f, "row %d out of range", i);
            const double want = w[0] * c + w[1] * b + w[2] * r;
            CHECK(std::fabs((double)out[i] - want) <= std::ldexp(want, -21),
                  "row %d: blend %.9g of %.9g", i, out[i], want);
          }
        }
        ++pools;
      }
    }
  }
  {
    const double w[3] = {1, 5, 5};
    // empty batches: nothing is read or written
    peer_mix_host(nullptr, 0, 8, 4, ct.ht_keys.data(), ct.ht_vals.data(), ct.ht_cap, log_ref_len,
                  0, w, nullptr, nullptr);
    // a pool of identical rows: every row's peers are itself
    const int G = 4, T = 6;
    std::vector<int64_t> hyps((size_t)G * T);
    for (int i = 0; i < G; ++i)
      for (int t = 0; t < T; ++t) hyps[(size_t)i * T + t] = t < 4 ? 3 + t : 0;
    std::vector<float> out(G), parts((size_t)G * 3);
    peer_mix_host(hyps.data(), G, T, G, ct.ht_keys.data(), ct.ht_vals.data(), ct.ht_cap,
                  log_ref_len, 0, w, out.data(), parts.data());
    for (int i = 0; i < G; ++i) {
      CHECK(std::fabs(parts[i * 3] - 10.f) < 1e-5f, "identical: CIDEr-D %.7f", parts[i * 3]);
      CHECK(std::fabs(parts[i * 3 + 1] - 1.f) < 1e-6f, "identical: BLEU %.7f", parts[i * 3 + 1]);
      CHECK(parts[i * 3 + 2] == 1.f, "identical: ROUGE %.7f", parts[i * 3 + 2]);
      CHECK(std::fabs(out[i] - 20.f) < 1e-4f, "identical: blend %.7f", out[i]);
    }
    // argument errors
    auto throws = [&](int g, int t, const double* ww, bool df, int64_t tok) {
      std::vector<int64_t> h((size_t)G * t, tok);
      try {
        peer_mix_host(h.data(), G, t, g, df ? ct.ht_keys.data() : nullptr,
                      df ? ct.ht_vals.data() : nullptr, df ? ct.ht_cap : 0, log_ref_len, 0, ww,
                      out.data(), parts.data());
      } catch (const std::invalid_argument&) {
        return true;
      }
      return false;
    };
    const double zero[3] = {0, 0, 0}, neg[3] = {1, -1, 0}, nan[3] = {1, std::nan(""), 0};
    const double rouge[3] = {0, 0, 1}, bleu[3] = {0, 1, 0};
    for (int bad : {1, 0, 3}) CHECK(throws(bad, T, w, true, 5), "G = %d accepted", bad);
    CHECK(throws(2, 65, w, true, 5), "T = 65 accepted");
    CHECK(throws(2, T, zero, true, 5), "zero weights accepted");
    CHECK(throws(2, T, neg, true, 5), "negative weight accepted");
    CHECK(throws(2, T, nan, true, 5), "NaN weight accepted");
    CHECK(throws(2, T, w, false, 5), "CIDEr-D without a df table accepted");
    CHECK(throws(2, T, bleu, false, 70000), "BLEU: token 70000 accepted");
    CHECK(!throws(2, T, rouge, false, 70000), "ROUGE: token 70000 refused");
    CHECK(!throws(2, T, rouge, false, 5), "ROUGE without a df table refused");
  }
  std::printf("%d pools, %d failures\n", pools, failures);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
