// Host-side driver for peer CIDEr-D scoring (csrc/host/cider_host.cpp:
// cider_peers_host, the twin of csrc/kernels/cider_pairwise.hip), built with
// AddressSanitizer + UBSan by tests/test_native_mbr_sanitizers.py.
//
// Every pool is scored twice: by cider_peers_host, and by the construction that
// defines the feature -- the pool rows as the reference table of one video
// (build_cider_tables), every row scored by cider_score_host with the reference
// PHYSICALLY PRESENT and its own row excluded (exclude[i] = i mod G).  The
// reference table holds its values in fp32 and the peer scorer keeps fp64, so
// the two agree to 1e-4 * max(1, score), the bound of the kernel's tests.
// Pools of 2, 3, 5, 21, 64 and 100 rows (beyond the kernel's LDS limit), widths
// 1, 5, 31 and 63, a tiny vocabulary (tf > 1, duplicate rows), empty rows, rows
// of BOS only and full-width rows without EOS, both use_eos settings.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "host/cider_host.h"

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
  std::mt19937 rng(1234);
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
  const int Gs[] = {2, 3, 5, 21, 64, 100};
  const int Ts[] = {1, 5, 31, 63};
  int pools = 0;
  for (int use_eos = 0; use_eos < 2; ++use_eos) {
    for (int G : Gs) {
      for (int T : Ts) {
        const int B = 3, N = B * G;
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
        CiderTables t = build_cider_tables(hyps.data(), N, T, start.data(), end.data(), B,
                                           df_keys.data(), df_vals.data(), (int)df_keys.size(),
                                           log_ref_len, use_eos);
        CiderTablesView v{t.ht_cap,           t.ht_keys.data(), t.ht_vals.data(),
                          t.vid_ref_off.data(), t.ref_ng_off.data(), t.ref_norm.data(),
                          t.ref_len.data(),   t.ng_key.data(),  t.ng_val.data()};
        std::vector<float> want(N, -1.f), got(N, -2.f);
        cider_score_host(hyps.data(), N, T, vid.data(), v, log_ref_len, use_eos, want.data(), true,
                         ex.data());
        cider_peers_host(hyps.data(), N, T, G, t.ht_keys.data(), t.ht_vals.data(), t.ht_cap,
                         log_ref_len, use_eos, got.data());
        for (int i = 0; i < N; ++i) {
          const double tol = 1e-4 * std::fmax(1.0, (double)want[i]);
          CHECK(std::fabs((double)got[i] - (double)want[i]) < tol,
                "G %d T %d eos %d row %d: peers %.7f, excluded reference %.7f", G, T, use_eos, i,
                got[i], want[i]);
          CHECK(got[i] >= 0.f && got[i] <= 10.0001f, "row %d: score %.7f out of range", i, got[i]);
        }
        ++pools;
      }
    }
  }
  // a pool of identical rows: every row's peers are itself, 10 when it has n-grams
  {
    const int G = 4, T = 6;
    std::vector<int64_t> hyps((size_t)G * T);
    for (int i = 0; i < G; ++i)
      for (int t = 0; t < T; ++t) hyps[(size_t)i * T + t] = t < 4 ? 3 + t : 0;
    CiderTables t = build_cider_tables(hyps.data(), 0, T, nullptr, nullptr, 0, df_keys.data(),
                                       df_vals.data(), (int)df_keys.size(), log_ref_len, 0);
    std::vector<float> got(G);
    cider_peers_host(hyps.data(), G, T, G, t.ht_keys.data(), t.ht_vals.data(), t.ht_cap,
                     log_ref_len, 0, got.data());
    for (int i = 0; i < G; ++i) CHECK(std::fabs(got[i] - 10.f) < 1e-5f, "identical: %.7f", got[i]);
    // argument errors: G < 2, rows that are no whole pools
    for (int bad : {1, 0, 3}) {
      bool threw = false;
      try {
        cider_peers_host(hyps.data(), G, T, bad, t.ht_keys.data(), t.ht_vals.data(), t.ht_cap,
                         log_ref_len, 0, got.data());
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      CHECK(threw, "G = %d accepted", bad);
    }
  }
  std::printf("%d pools, %d failures\n", pools, failures);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
