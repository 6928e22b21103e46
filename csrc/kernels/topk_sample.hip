// K3: truncated (top-k / nucleus) sampling step of the consensus decode.
//
// One launch selects one decode step's token for R rows from what the vocab
// launch leaves under VF_TOPK: the (n_vt, R) tile partials and the (n_vt, R,
// K) tile candidates, K <= 8.  Per row (one wavefront, 4 rows per workgroup,
// as beam_topk_cand_kernel):
//   * LSE of the row from the tile partials (lane-strided merge, then a
//     shuffle tree; lane 0's value is the row's);
//   * the n_vt * K candidates merged into the row's global top-K, by value
//     descending, ties to the smaller index (padding slots: -inf, 0x7fffffff);
//   * weights w_i = exp((x_i - x_0) / tau) -- the LSE cancels, so the logits
//     serve as the log-probs --, the nucleus m = the smallest prefix with
//     w_0 + .. + w_{m-1} >= top_p * sum w, and one uniform draw from the
//     counter hash keyed by (sampling seed, step, row) over that prefix;
//   * the end-of-sequence rule of the combine's finish_row (vocab.hip): a row
//     stays unfinished while it draws non-EOS tokens; a finished row emits 0
//     and feeds 0; the log-prob written is the drawn candidate's either way.
// Outputs: the token (into the sequence column), the next input token, and
// lp = x_i - LSE, the model's untruncated log-prob at temperature 1.
//
// No atomics, no block barrier, no LDS; the candidate registers are indexed
// by unrolled selects only.  Every sum runs in a fixed order, so a relaunch
// with the same seeds gives the same bits.
#include <cmath>

#include "../common.h"
#include "../launchers.h"
#include "vocab_common.h"

namespace cst {

namespace {

constexpr int TS_ROWS = 4;  // rows (wavefronts) per workgroup
constexpr int TS_MK = VF_TOPK_MAXK;

__device__ __forceinline__ void ts_wave_argmax(float& best, int& besti) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ov > best || (ov == best && oi < besti)) best = ov, besti = oi;
  }
}

__device__ __forceinline__ void ts_lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - M)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - M));
  m = M;
}

}  // namespace

__global__ __launch_bounds__(64 * TS_ROWS) void topk_sample_kernel(TopkSampleArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * TS_ROWS + (threadIdx.x >> 6);
  if (r >= a.R) return;
  const int K = a.K, R = a.R;
  // the row's LSE: tiles lane, lane + 64, .. in order, then the shuffle tree
  float m = -INFINITY, s = 0.f;
  for (int t = lane; t < a.n_vt; t += 64) {
    const VocabPartial& p = a.part[(int64_t)t * R + r];
    ts_lse_merge(m, s, p.m, p.s);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) ts_lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  // (the two lanes of a pair may contract the sum differently: lane 0 decides)
  const float lse = __shfl(m + __logf(s), 0, 64);
  // lane-local sorted top-K of the lane's candidates (static register indices)
  float bv[TS_MK];
  int bi[TS_MK];
#pragma unroll
  for (int k = 0; k < TS_MK; ++k) bv[k] = -INFINITY, bi[k] = 0x7fffffff;
  const int n = a.n_vt * K;
  float thr = -INFINITY;
  for (int c0 = lane; c0 < n; c0 += 64 * 4) {
    float2 xs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + 64 * u;
      // candidate c = (tile c / K, rank c % K) of row r
      xs[u] = c < n ? a.cand[((int64_t)(c / K) * R + r) * K + c % K]
                    : make_float2(-INFINITY, __int_as_float(0x7fffffff));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float cv = xs[u].x;
      int ci = __float_as_int(xs[u].y);
      if (!(cv > thr || (cv == thr && ci < 0x7fffffff))) continue;
#pragma unroll
      for (int p = 0; p < TS_MK; ++p) {
        if (p < K && (cv > bv[p] || (cv == bv[p] && ci < bi[p]))) {
          const float tv = bv[p];
          const int tix = bi[p];
          bv[p] = cv, bi[p] = ci;
          cv = tv, ci = tix;
        }
      }
#pragma unroll
      for (int p = 0; p < TS_MK; ++p) thr = p == K - 1 ? bv[p] : thr;
    }
  }
  // K rounds of wave arg-max over the lanes' list heads: the row's candidates
  // in order, the same in every lane
  float cv[TS_MK];
  int ci[TS_MK];
#pragma unroll
  for (int k = 0; k < TS_MK; ++k) {
    cv[k] = -INFINITY, ci[k] = 0x7fffffff;
    if (k < K) {  // (uniform)
      float best = bv[0];
      int besti = bi[0];
      ts_wave_argmax(best, besti);
      if (bi[0] == besti) {
#pragma unroll
        for (int p = 0; p + 1 < TS_MK; ++p) bv[p] = bv[p + 1], bi[p] = bi[p + 1];
        bv[TS_MK - 1] = -INFINITY, bi[TS_MK - 1] = 0x7fffffff;
      }
      cv[k] = best, ci[k] = besti;
    }
  }
  if (lane != 0) return;
  // temperature weights against the best candidate, summed in rank order
  float w[TS_MK], tot = 0.f;
#pragma unroll
  for (int k = 0; k < TS_MK; ++k) {
    w[k] = k < K ? __expf((cv[k] - cv[0]) * a.inv_tau) : 0.f;
    tot += w[k];
  }
  // nucleus: the shortest prefix whose mass reaches top_p of the total (top_p
  // = 1: the same sum in the same order, so all K)
  const float need = a.top_p * tot;
  float cum = 0.f, mass = 0.f;
  bool full = false;
#pragma unroll
  for (int k = 0; k < TS_MK; ++k) {
    cum += w[k];
    if (k < K && !full) mass = cum, full = cum >= need;
  }
  // one uniform in (0, 1] per (seed, step, row); the first rank whose
  // cumulative weight reaches u * mass (rank m - 1 always does)
  const uint32_t seed = rng_seed(a.rng, RNG_SLOT_SAMPLE);
  const uint32_t key = mix32(seed ^ mix32((uint32_t)r * 0x9E3779B1u + (uint32_t)a.step * 0x85EBCA77u) ^
                             0x3C6EF372u);
  const float target = u01(mix32(key ^ 0xA54FF53Au)) * mass;
  float sel_v = cv[0];
  int sel_i = ci[0];
  bool found = false;
  cum = 0.f;
#pragma unroll
  for (int k = 0; k < TS_MK; ++k) {
    cum += w[k];
    if (k < K && !found && cum >= target) sel_v = cv[k], sel_i = ci[k], found = true;
  }
  int64_t tok = (unsigned)sel_i < (unsigned)a.V ? sel_i : 0;
  // per-row finished mask, as finish_row: sticky once the row drew EOS (0)
  if (a.unfinished != nullptr) {
    const uint8_t u = a.unfinished[r] != 0 && tok > 0;
    a.unfinished[r] = u;
    if (!u) tok = 0;
  }
  a.tok_out[(int64_t)r * a.tok_stride] = tok;
  if (a.next_tok != nullptr) a.next_tok[r] = tok;
  a.lp_out[(int64_t)r * a.lp_stride] = sel_v - lse;
  if (a.lse_out != nullptr) a.lse_out[r] = lse;
}

void launch_topk_sample(const TopkSampleArgs& a, hipStream_t stream) {
  if (a.K < 1 || a.K > TS_MK) throw std::runtime_error("topk_sample: top_k must be in [1, 8]");
  if (a.K > a.V) throw std::runtime_error("topk_sample: top_k > vocab_size");
  if (!(a.top_p > 0.f && a.top_p <= 1.f) || !(a.inv_tau > 0.f) || !std::isfinite(a.inv_tau))
    throw std::runtime_error("topk_sample: top_p in (0, 1], temperature > 0");
  if (a.R < 1) return;
  hipLaunchKernelGGL(topk_sample_kernel, dim3((a.R + TS_ROWS - 1) / TS_ROWS), dim3(64 * TS_ROWS),
                     0, stream, a);
  post_launch("topk_sample_kernel", stream);
}

}  // namespace cst
