// Host-side stress driver for the validation scorer's host code
// (csrc/host/metric_host.cpp: bleu_stats_host, meteor_stats_host, the stem rows
// of the table builder; csrc/host/cider_host.cpp: the unclipped flag), built
// with AddressSanitizer + UBSan by tests/test_native_corpus_sanitizers.py.
// Random datasets plus edge cases (videos without references, empty / BOS-only
// references, empty hypotheses, maximal lengths, tiny vocabularies with many
// repeated words); the statistics are checked against a naive BLEU count and a
// naive METEOR alignment (a list of pairs, as eval/metrics.py keeps them)
// written here from the raw label rows, without the tables.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <stdexcept>
#include <vector>

#include "host/cider_host.h"
#include "host/metric_host.h"

using namespace cst;

typedef std::vector<int> Toks;

static Toks reduce(const int64_t* row, int n) {
  Toks out;
  for (int i = 0; i < n; ++i) {
    if (row[i] == 0) break;
    if (row[i] != 1) out.push_back((int)row[i]);
  }
  return out;
}

static std::map<Toks, int> grams_of(const Toks& t) {
  std::map<Toks, int> c;
  for (int n = 1; n <= 4; ++n)
    for (int i = 0; i + n <= (int)t.size(); ++i) c[Toks(t.begin() + i, t.begin() + i + n)] += 1;
  return c;
}

static void naive_bleu_stats(const Toks& h, const std::vector<Toks>& refs, int out[10]) {
  std::map<Toks, int> maxc;
  for (auto& r : refs)
    for (auto& g : grams_of(r)) maxc[g.first] = std::max(maxc[g.first], g.second);
  for (int k = 0; k < 10; ++k) out[k] = 0;
  for (auto& g : grams_of(h)) {
    auto it = maxc.find(g.first);
    if (it != maxc.end()) out[g.first.size() - 1] += std::min(g.second, it->second);
  }
  const int tlen = (int)h.size();
  std::pair<int, int> best(1 << 30, 0);
  for (auto& r : refs)
    best = std::min(best, std::make_pair(std::abs((int)r.size() - tlen), (int)r.size()));
  for (int k = 0; k < 4; ++k) out[4 + k] = std::max(0, tlen - k);
  out[8] = tlen;
  out[9] = refs.empty() ? 0 : best.second;
}

struct Pair {
  int i, j, stage;
};

// Meteor._align / _stats: n_exact, n_stem, len_h, len_r, chunks, n_pairs
static void naive_meteor(const Toks& h, const Toks& r, const std::vector<int32_t>& stem,
                         int out[6]) {
  std::vector<Pair> pairs;
  std::vector<bool> used(r.size(), false);
  for (int stage = 0; stage < 2; ++stage)
    for (int i = 0; i < (int)h.size(); ++i) {
      bool paired = false;
      for (auto& p : pairs) paired = paired || p.i == i;
      if (paired) continue;
      const int kw = stage ? stem[h[i]] : h[i];
      const Pair* prev = nullptr;
      for (auto& p : pairs)
        if (p.i < i && (!prev || p.i > prev->i)) prev = &p;
      const int want = prev ? prev->j + 1 : 0;
      int bj = -1;
      for (int j = 0; j < (int)r.size(); ++j) {
        if (used[j] || (stage ? stem[r[j]] : r[j]) != kw) continue;
        if (bj < 0 || std::make_pair(std::abs(j - want), j) < std::make_pair(std::abs(bj - want), bj))
          bj = j;
      }
      if (bj < 0) continue;
      used[bj] = true;
      pairs.push_back({i, bj, stage});
    }
  std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.i < b.i; });
  int chunks = pairs.empty() ? 0 : 1;
  for (size_t k = 1; k < pairs.size(); ++k)
    if (!(pairs[k].i == pairs[k - 1].i + 1 && pairs[k].j == pairs[k - 1].j + 1)) ++chunks;
  out[0] = out[1] = 0;
  for (auto& p : pairs) out[p.stage] += 1;
  out[2] = (int)h.size(), out[3] = (int)r.size(), out[4] = chunks, out[5] = (int)pairs.size();
}

static int run(uint32_t seed, int Nv, int L, int T, int V, int n_stems) {
  std::mt19937 rng(seed);
  std::vector<int32_t> stem(V);
  for (int t = 0; t < V; ++t) stem[t] = (int32_t)(rng() % n_stems);
  std::vector<int64_t> start(Nv), end(Nv), labels;
  int M = 0;
  for (int v = 0; v < Nv; ++v) {
    const int ncap = (v % 7 == 3) ? 0 : 1 + (int)(rng() % 80);  // some videos have no refs
    start[v] = M;
    for (int c = 0; c < ncap; ++c, ++M) {
      const int len = (int)(rng() % (L + 1));
      const int kind = (int)(rng() % 16);
      for (int i = 0; i < L; ++i) {
        int64_t tok = i < len ? 2 + (int64_t)(rng() % (V - 2)) : 0;
        if (kind == 0) tok = 0;                  // empty reference
        if (kind == 1) tok = i < len ? 1 : 0;    // BOS only: empty after reduction
        if (kind == 2 && i == len / 2) tok = 1;  // BOS inside
        if (kind == 3) tok = tok ? tok : V - 1;  // no EOS: full width
        labels.push_back(tok);
      }
    }
    end[v] = M;
  }
  MetricTables t = build_metric_tables(labels.data(), M, L, start.data(), end.data(), Nv, 0,
                                       stem.data(), V);
  if (t.ref_stem.size() != t.ref_tok.size()) {
    std::printf("seed %u: %zu stem entries for %zu tokens\n", seed, t.ref_stem.size(),
                t.ref_tok.size());
    return 1;
  }
  const MetricTablesView view = view_of(t);
  const int N = 4 * Nv;
  std::vector<int64_t> hyps((size_t)N * T, 0), hv(N);
  for (int i = 0; i < N; ++i) {
    const int v = i % Nv;
    hv[i] = v;
    const int kind = i % 4;  // random full width / reference copy / empty / short random
    const int len = kind == 3 ? (int)(rng() % (T + 1)) : T;
    for (int j = 0; j < T; ++j) {
      int64_t tok = 0;
      if ((kind == 0 || kind == 3) && j < len) tok = 1 + (int64_t)(rng() % (V - 1));
      if (kind == 1 && end[v] > start[v] && j < L) tok = labels[(size_t)start[v] * L + j];
      hyps[(size_t)i * T + j] = tok;
    }
  }
  std::vector<int32_t> bs((size_t)N * 10, -1), ms((size_t)N * 6, -1);
  std::vector<double> sc(N, -1.0);
  bleu_stats_host(hyps.data(), N, T, hv.data(), view, bs.data());
  meteor_stats_host(hyps.data(), N, T, hv.data(), view, t.ref_stem.data(), stem.data(), V,
                    ms.data(), sc.data());
  for (int i = 0; i < N; ++i) {
    const int v = (int)hv[i];
    std::vector<Toks> refs;
    for (int64_t r = start[v]; r < end[v]; ++r) refs.push_back(reduce(&labels[(size_t)r * L], L));
    const Toks h = reduce(&hyps[(size_t)i * T], T);
    int wb[10];
    naive_bleu_stats(h, refs, wb);
    for (int k = 0; k < 10; ++k)
      if (bs[(size_t)i * 10 + k] != wb[k]) {
        std::printf("seed %u hyp %d: bleu stat %d is %d, want %d\n", seed, i, k,
                    bs[(size_t)i * 10 + k], wb[k]);
        return 1;
      }
    int best[6] = {0, 0, 0, 0, 0, 0};
    double best_score = refs.empty() ? 0.0 : -1.0;
    for (auto& r : refs) {
      int st[6];
      naive_meteor(h, r, stem, st);
      const double s = meteor_score_host(st[0], st[1], st[2], st[3], st[4]);
      if (s > best_score) {
        best_score = s;
        std::copy(st, st + 6, best);
      }
    }
    bool same = sc[i] == best_score && sc[i] >= 0.0 && sc[i] <= 1.0;
    for (int k = 0; k < 6; ++k) same = same && ms[(size_t)i * 6 + k] == best[k];
    if (!same) {
      std::printf("seed %u hyp %d: meteor %d %d %d %d %d %d score %.17g, want %d %d %d %d %d %d "
                  "score %.17g\n", seed, i, ms[(size_t)i * 6], ms[(size_t)i * 6 + 1],
                  ms[(size_t)i * 6 + 2], ms[(size_t)i * 6 + 3], ms[(size_t)i * 6 + 4],
                  ms[(size_t)i * 6 + 5], sc[i], best[0], best[1], best[2], best[3], best[4],
                  best[5], best_score);
      return 1;
    }
  }
  return 0;
}

// The unclipped CIDEr flag: equal to the clipped score times the inverse
// penalty where no count is clipped (a hypothesis that copies its only
// reference), never below the clipped score, finite.
static int cider_flag(uint32_t seed) {
  std::mt19937 rng(seed);
  const int Nv = 9, L = 20, V = 12;
  std::vector<int64_t> start(Nv), end(Nv), labels;
  int M = 0;
  for (int v = 0; v < Nv; ++v) {
    start[v] = M;
    const int ncap = 1 + (int)(rng() % 5);
    for (int c = 0; c < ncap; ++c, ++M) {
      const int len = 1 + (int)(rng() % (L - 1));
      for (int i = 0; i < L; ++i) labels.push_back(i < len ? 2 + (int64_t)(rng() % (V - 2)) : 0);
    }
    end[v] = M;
  }
  std::vector<int64_t> df_keys;
  std::vector<float> df_vals;
  for (int a = 2; a < V; ++a) {
    df_keys.push_back(a + 1);
    df_vals.push_back(1.f + (float)(rng() % 4));
  }
  const double lrl = std::log((double)Nv);
  CiderTables t = build_cider_tables(labels.data(), M, L, start.data(), end.data(), Nv,
                                     df_keys.data(), df_vals.data(), (int)df_keys.size(), lrl, 0);
  const CiderTablesView view{t.ht_cap,          t.ht_keys.data(), t.ht_vals.data(),
                             t.vid_ref_off.data(), t.ref_ng_off.data(), t.ref_norm.data(),
                             t.ref_len.data(),  t.ng_key.data(),  t.ng_val.data()};
  const int N = 2 * Nv, T = 24;
  std::vector<int64_t> hyps((size_t)N * T, 0), hv(N);
  for (int i = 0; i < N; ++i) {
    hv[i] = i % Nv;
    for (int j = 0; j < T; ++j)
      hyps[(size_t)i * T + j] = i < Nv ? (j < L ? labels[(size_t)start[hv[i]] * L + j] : 0)
                                       : (int64_t)(rng() % V);
  }
  std::vector<float> clipped(N, -1.f), plain(N, -1.f), dflt(N, -2.f);
  cider_score_host(hyps.data(), N, T, hv.data(), view, lrl, 0, clipped.data(), true);
  cider_score_host(hyps.data(), N, T, hv.data(), view, lrl, 0, plain.data(), false);
  cider_score_host(hyps.data(), N, T, hv.data(), view, lrl, 0, dflt.data());
  for (int i = 0; i < N; ++i) {
    if (!(std::isfinite(plain[i]) && plain[i] >= 0.f) || dflt[i] != clipped[i] ||
        plain[i] < clipped[i] * (1.f - 1e-6f)) {
      std::printf("cider seed %u hyp %d: clipped %.9g unclipped %.9g default %.9g\n", seed, i,
                  clipped[i], plain[i], dflt[i]);
      return 1;
    }
  }
  return 0;
}

template <class F>
static int must_throw(const char* what, F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return 0;
  }
  std::printf("no error for %s\n", what);
  return 1;
}

static int limits() {
  int bad = 0;
  const int64_t st = 0, en = 1, hv = 0;
  std::vector<int32_t> stem(8, 0);
  std::vector<int64_t> row65(65, 7), row64(65, 7);
  row64[64] = 0;
  std::vector<int64_t> oov = {5, 8, 0};
  bad |= must_throw("a reference token without a stem id",
                    [&] { build_metric_tables(oov.data(), 1, 3, &st, &en, 1, 0, stem.data(), 8); });
  MetricTables t = build_metric_tables(row64.data(), 1, 65, &st, &en, 1, 0, stem.data(), 8);
  const MetricTablesView view = view_of(t);
  int32_t bs[10], ms[6];
  double sc = -1;
  bad |= must_throw("T = 65", [&] { bleu_stats_host(row65.data(), 1, 65, &hv, view, bs); });
  bad |= must_throw("T = 65", [&] {
    meteor_stats_host(row65.data(), 1, 65, &hv, view, t.ref_stem.data(), stem.data(), 8, ms, &sc);
  });
  const int64_t hv_bad = 1;
  bad |= must_throw("video index past the tables", [&] {
    meteor_stats_host(oov.data(), 1, 3, &hv_bad, view, t.ref_stem.data(), stem.data(), 8, ms, &sc);
  });
  // a hypothesis token past the stem table matches nothing in the stem stage
  meteor_stats_host(oov.data(), 1, 3, &hv, view, t.ref_stem.data(), stem.data(), 8, ms, &sc);
  if (ms[0] != 0 || ms[1] != 1 || ms[2] != 2 || ms[3] != 64) {
    std::printf("token past the stem table: %d %d %d %d\n", ms[0], ms[1], ms[2], ms[3]);
    bad = 1;
  }
  // 64 equal tokens against 64 equal tokens: every pair (i, i), one chunk
  meteor_stats_host(row64.data(), 1, 64, &hv, view, t.ref_stem.data(), stem.data(), 8, ms, &sc);
  if (ms[0] != 64 || ms[1] != 0 || ms[2] != 64 || ms[3] != 64 || ms[4] != 1 || ms[5] != 64) {
    std::printf("64 equal tokens: %d %d %d %d %d %d\n", ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
    bad = 1;
  }
  return bad;
}

int main() {
  int bad = limits();
  for (uint32_t s = 0; s < 4; ++s) {
    bad |= run(s, 20 + 9 * (int)s, 30, 30, 40 + 50 * (int)s, 19 + 10 * (int)s);
    bad |= run(100 + s, 5, 64, 64, 6, 3);         // maximal lengths, tiny vocabulary
    bad |= run(200 + s, 4, 64, 64, 65535, 4000);  // token ids up to 65,534
    bad |= cider_flag(300 + s);
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
