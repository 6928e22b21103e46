// Host-side driver for the leave-one-out (`exclude`) paths of the native
// scorers (csrc/host/metric_host.cpp: bleu4_score_host, rouge_l_score_host,
// meteor_stats_host and the ng_cnt2 / ng_arg rows of the table builder;
// csrc/host/cider_host.cpp: cider_score_host), built with AddressSanitizer +
// UBSan by tests/test_native_consensus_sanitizers.py.
//
// Every hypothesis is scored twice: against the video's full tables with
// exclude = e, and against tables built from the video's label rows with row e
// PHYSICALLY REMOVED and no exclusion.  The two must agree bit for bit (the
// scorers walk the remaining references in the same order).  Videos have 1, 2,
// 3, 20, 70 and 100 references (more than 64; excluded indices >= 64), a tiny
// vocabulary (clip counts above 1, ties, duplicate captions), empty and
// full-width references.  Entries that leave nothing out (negative, past the
// end, a single reference) must give the bits of a null `exclude`.
#include <cmath>
#include <cstdio>
#include <cstring>
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

struct Scores {
  float bleu, rouge, cider, cider_u;
  int32_t met[6];
  double met_score;
};

static CiderTablesView cview(const CiderTables& t) {
  return {t.ht_cap,           t.ht_keys.data(), t.ht_vals.data(), t.vid_ref_off.data(),
          t.ref_ng_off.data(), t.ref_norm.data(), t.ref_len.data(), t.ng_key.data(),
          t.ng_val.data()};
}

struct Setup {
  int use_eos;
  std::vector<int32_t> stem;
  std::vector<int64_t> df_keys;
  std::vector<float> df_vals;
  double log_ref_len;
};

// the tables of one video: `ncap` label rows of width L
struct Tables {
  MetricTables mt, st;
  CiderTables ct;
  Tables(const Setup& s, const int64_t* rows, int ncap, int L) {
    const int64_t start = 0, end = ncap;
    mt = build_metric_tables(rows, ncap, L, &start, &end, 1, s.use_eos);
    st = build_metric_tables(rows, ncap, L, &start, &end, 1, 0, s.stem.data(),
                             (int)s.stem.size());
    ct = build_cider_tables(rows, ncap, L, &start, &end, 1, s.df_keys.data(), s.df_vals.data(),
                            (int)s.df_keys.size(), s.log_ref_len, s.use_eos);
  }
};

// one hypothesis against a video's tables, leaving out `exclude` (nullptr: none)
static Scores score(const Setup& c, const Tables& t, const int64_t* hyp, int T,
                    const int64_t* exclude) {
  const int64_t vid = 0;
  Scores s;
  bleu4_score_host(hyp, 1, T, &vid, view_of(t.mt), c.use_eos, &s.bleu, exclude);
  rouge_l_score_host(hyp, 1, T, &vid, view_of(t.mt), c.use_eos, &s.rouge, exclude);
  meteor_stats_host(hyp, 1, T, &vid, view_of(t.st), t.st.ref_stem.data(), c.stem.data(),
                    (int)c.stem.size(), s.met, &s.met_score, exclude);
  cider_score_host(hyp, 1, T, &vid, cview(t.ct), c.log_ref_len, c.use_eos, &s.cider, true,
                   exclude);
  cider_score_host(hyp, 1, T, &vid, cview(t.ct), c.log_ref_len, c.use_eos, &s.cider_u, false,
                   exclude);
  return s;
}

static bool same(const Scores& a, const Scores& b) {
  return std::memcmp(&a.bleu, &b.bleu, sizeof(float)) == 0 &&
         std::memcmp(&a.rouge, &b.rouge, sizeof(float)) == 0 &&
         std::memcmp(&a.cider, &b.cider, sizeof(float)) == 0 &&
         std::memcmp(&a.cider_u, &b.cider_u, sizeof(float)) == 0 &&
         std::memcmp(a.met, b.met, sizeof(a.met)) == 0 &&
         std::memcmp(&a.met_score, &b.met_score, sizeof(double)) == 0;
}

static void run(uint32_t seed, int L, int V, int use_eos, const std::vector<int>& ncaps) {
  std::mt19937 rng(seed);
  Setup cfg;
  cfg.use_eos = use_eos;
  cfg.stem.resize(V);
  for (int t = 0; t < V; ++t) cfg.stem[t] = (int32_t)(rng() % 4);
  // a df table of unigrams and some bigrams (values as a corpus would give)
  for (int a = 0; a < V; ++a) {
    cfg.df_keys.push_back(a + 1);
    cfg.df_vals.push_back((float)(1 + rng() % 5));
    for (int b = 0; b < V; b += 2) {
      cfg.df_keys.push_back((int64_t)(a + 1) | ((int64_t)(b + 1) << 16));
      cfg.df_vals.push_back((float)(1 + rng() % 3));
    }
  }
  cfg.log_ref_len = std::log(6.0);
  long changed = 0, total = 0;
  for (int ncap : ncaps) {
    std::vector<int64_t> rows((size_t)ncap * L);
    for (int c = 0; c < ncap; ++c) {
      const int kind = (int)(rng() % 12);
      const int len = kind == 0 ? 0 : (kind == 1 ? L : 1 + (int)(rng() % (L - 1)));
      for (int i = 0; i < L; ++i)
        rows[(size_t)c * L + i] = i < len ? 2 + (int64_t)(rng() % (V - 2)) : 0;
      if (kind == 2 && c > 0)  // a duplicate of the previous caption
        std::memcpy(&rows[(size_t)c * L], &rows[(size_t)(c - 1) * L], L * sizeof(int64_t));
      if (kind == 3) rows[(size_t)c * L] = 1;  // BOS first, as label files have it
    }
    // hypotheses: every caption leaving itself out, then random rows with
    // exclusions that hit, miss or leave nothing out
    const Tables full(cfg, rows.data(), ncap, L);
    const int n_random = 24;
    for (int h = 0; h < ncap + n_random; ++h) {
      std::vector<int64_t> hyp(L, 0);
      int64_t e;
      if (h < ncap) {
        std::memcpy(hyp.data(), &rows[(size_t)h * L], L * sizeof(int64_t));
        e = h;
      } else {
        const int len = (int)(rng() % (L + 1));
        for (int i = 0; i < len; ++i) hyp[i] = 2 + (int64_t)(rng() % (V - 2));
        const int64_t pick[] = {-1, (int64_t)ncap, (int64_t)ncap + 5, -(1ll << 40), 1ll << 40,
                                0, (int64_t)ncap - 1, (int64_t)(rng() % ncap)};
        e = pick[h % 8];
      }
      const Scores with = score(cfg, full, hyp.data(), L, &e);
      const Scores none = score(cfg, full, hyp.data(), L, nullptr);
      const bool hits = e >= 0 && e < ncap && ncap > 1;
      if (!hits) {
        CHECK(same(with, none), "ncap %d hyp %d exclude %lld: a no-op changed the scores", ncap,
              h, (long long)e);
        continue;
      }
      std::vector<int64_t> rest;
      for (int c = 0; c < ncap; ++c)
        if (c != e) rest.insert(rest.end(), &rows[(size_t)c * L], &rows[(size_t)c * L] + L);
      const Scores want = score(cfg, Tables(cfg, rest.data(), ncap - 1, L), hyp.data(), L, nullptr);
      CHECK(same(with, want),
            "ncap %d hyp %d exclude %lld: bleu %g/%g rouge %g/%g cider %g/%g meteor %g/%g", ncap,
            h, (long long)e, with.bleu, want.bleu, with.rouge, want.rouge, with.cider,
            want.cider, with.met_score, want.met_score);
      ++total;
      changed += !same(with, none);
    }
  }
  // (an `exclude` that is read but ignored would pass everything above only if
  // leaving a reference out never mattered)
  CHECK(changed * 2 > total, "exclusion changed %ld of %ld scores", changed, total);
}

int main() {
  run(1, 12, 8, 0, {1, 2, 3, 20, 70, 100});
  run(2, 12, 8, 1, {1, 2, 3, 20, 70, 100});
  run(3, 64, 40, 0, {3, 66});           // full-width rows (64 tokens)
  run(4, 5, 4, 1, {1, 2, 3, 20, 70});   // very short captions: many duplicates and ties
  // a view without ng_cnt2 / ng_arg: scores without exclusion, refuses one
  {
    const int64_t rows[] = {2, 3, 0, 3, 3, 0}, start = 0, end = 2, vid = 0, e = 0;
    MetricTables t = build_metric_tables(rows, 2, 3, &start, &end, 1, 0);
    MetricTablesView v{1,
                       t.vid_ref_off.data(),
                       t.ref_len.data(),
                       t.vid_ng_off.data(),
                       t.ng_key.data(),
                       t.ng_cnt.data(),
                       t.ref_tok_off.data(),
                       t.ref_tok.data()};
    float a = -1, b = -2;
    bleu4_score_host(rows, 1, 3, &vid, v, 0, &a);
    bleu4_score_host(rows, 1, 3, &vid, view_of(t), 0, &b);
    CHECK(a == b, "old-style view: %g vs %g", a, b);
    bool threw = false;
    try {
      bleu4_score_host(rows, 1, 3, &vid, v, 0, &a, &e);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw, "leave-one-out BLEU on a view without ng_cnt2 did not throw");
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
