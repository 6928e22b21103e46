// Host-side stress driver for csrc/host/metric_host.cpp (the sentence BLEU-4 /
// ROUGE-L table builder and CPU scorers), built with AddressSanitizer + UBSan
// by tests/test_native_metric_sanitizers.py.  Random datasets plus edge cases
// (videos without references, empty / BOS-only references, empty hypotheses,
// maximal lengths and token ids, use_eos on and off); every score is checked
// against a naive BLEU / LCS written here from the raw label rows, without the
// tables.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <stdexcept>
#include <vector>

#include "host/metric_host.h"

using namespace cst;

typedef std::vector<int> Toks;

static Toks reduce(const int64_t* row, int n, int use_eos) {
  Toks out;
  for (int i = 0; i < n; ++i) {
    if (row[i] == 0) {
      if (use_eos) out.push_back(0);
      break;
    }
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

static double naive_bleu(const Toks& h, const std::vector<Toks>& refs) {
  if (refs.empty()) return 0.0;
  std::map<Toks, int> maxc;
  for (auto& r : refs)
    for (auto& g : grams_of(r)) maxc[g.first] = std::max(maxc[g.first], g.second);
  int correct[4] = {0, 0, 0, 0};
  for (auto& g : grams_of(h)) {
    auto it = maxc.find(g.first);
    if (it != maxc.end()) correct[g.first.size() - 1] += std::min(g.second, it->second);
  }
  const int tlen = (int)h.size();
  std::pair<int, int> best(1 << 30, 0);
  for (auto& r : refs)
    best = std::min(best, std::make_pair(std::abs((int)r.size() - tlen), (int)r.size()));
  double b = 1.0;
  for (int k = 0; k < 4; ++k) b *= (correct[k] + 1e-15) / (std::max(0, tlen - k) + 1e-9);
  double s = std::pow(b, 0.25);
  const double ratio = (tlen + 1e-15) / (best.second + 1e-9);
  if (ratio < 1) s *= std::exp(1 - 1 / ratio);
  return s;
}

static int naive_lcs(const Toks& a, const Toks& b) {  // full table
  std::vector<std::vector<int>> d(a.size() + 1, std::vector<int>(b.size() + 1, 0));
  for (size_t i = 0; i < a.size(); ++i)
    for (size_t j = 0; j < b.size(); ++j)
      d[i + 1][j + 1] = a[i] == b[j] ? d[i][j] + 1 : std::max(d[i][j + 1], d[i + 1][j]);
  return d[a.size()][b.size()];
}

static double naive_rouge(const Toks& h, const std::vector<Toks>& refs) {
  double p = 0, rc = 0;
  for (auto& r : refs) {
    const int l = naive_lcs(r, h);
    if (!h.empty()) p = std::max(p, l / (double)h.size());
    if (!r.empty()) rc = std::max(rc, l / (double)r.size());
  }
  const double beta = 1.2, b2 = beta * beta;
  return (p != 0 && rc != 0) ? ((1 + b2) * p * rc) / (rc + b2 * p) : 0.0;
}

static int run(uint32_t seed, int Nv, int L, int T, int V, int use_eos) {
  std::mt19937 rng(seed);
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
        if (kind == 0) tok = 0;                      // empty reference
        if (kind == 1) tok = i < len ? 1 : 0;        // BOS only: empty after reduction
        if (kind == 2 && i == len / 2) tok = 1;      // BOS inside
        if (kind == 3 && use_eos == 0) tok = tok ? tok : V - 1;  // no EOS: full width
        labels.push_back(tok);
      }
    }
    end[v] = M;
  }
  MetricTables t = build_metric_tables(labels.data(), M, L, start.data(), end.data(), Nv, use_eos);
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
  std::vector<float> bleu(N, -1.f), rouge(N, -1.f);
  bleu4_score_host(hyps.data(), N, T, hv.data(), view, use_eos, bleu.data());
  rouge_l_score_host(hyps.data(), N, T, hv.data(), view, use_eos, rouge.data());
  for (int i = 0; i < N; ++i) {
    const int v = (int)hv[i];
    std::vector<Toks> refs;
    for (int64_t r = start[v]; r < end[v]; ++r) refs.push_back(reduce(&labels[(size_t)r * L], L, use_eos));
    const Toks h = reduce(&hyps[(size_t)i * T], T, use_eos);
    const float wb = (float)naive_bleu(h, refs), wr = (float)naive_rouge(h, refs);
    if (bleu[i] != wb || rouge[i] != wr || !(rouge[i] >= 0.f && rouge[i] <= 1.f)) {
      std::printf("seed %u hyp %d: bleu %.9g want %.9g, rouge %.9g want %.9g\n", seed, i, bleu[i],
                  wb, rouge[i], wr);
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
  std::vector<int64_t> row65(65, 7), row64(65, 7);
  row64[64] = 0;
  bad |= must_throw("a 65-token reference",
                    [&] { build_metric_tables(row65.data(), 1, 65, &st, &en, 1, 0); });
  bad |= must_throw("64 tokens + kept EOS",
                    [&] { build_metric_tables(row64.data(), 1, 65, &st, &en, 1, 1); });
  std::vector<int64_t> big = {5, 65535, 0};
  bad |= must_throw("reference token 65535",
                    [&] { build_metric_tables(big.data(), 1, 3, &st, &en, 1, 0); });
  MetricTables t = build_metric_tables(row64.data(), 1, 65, &st, &en, 1, 0);
  const MetricTablesView view = view_of(t);
  float out = -1.f;
  bad |= must_throw("T = 65", [&] { bleu4_score_host(row65.data(), 1, 65, &hv, view, 0, &out); });
  bad |= must_throw("T = 65", [&] { rouge_l_score_host(row65.data(), 1, 65, &hv, view, 0, &out); });
  bad |= must_throw("hypothesis token 65535",
                    [&] { bleu4_score_host(big.data(), 1, 3, &hv, view, 0, &out); });
  const int64_t hv_bad = 1;
  bad |= must_throw("video index past the tables",
                    [&] { rouge_l_score_host(big.data(), 1, 3, &hv_bad, view, 0, &out); });
  return bad;
}

int main() {
  int bad = limits();
  for (uint32_t s = 0; s < 4; ++s)
    for (int use_eos = 0; use_eos < 2; ++use_eos) {
      bad |= run(s, 20 + 9 * (int)s, 30, 30, 40 + 50 * (int)s, use_eos);
      bad |= run(100 + s, 5, 63, 64, 6, use_eos);       // maximal lengths, tiny vocabulary
      bad |= run(200 + s, 4, 64 - use_eos, 64, 65535, use_eos);  // token ids up to 65,534
    }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
