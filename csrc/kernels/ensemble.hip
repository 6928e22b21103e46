// K11: top-K of an ensemble's mixture log-probability, one decode step.
//
// M member models (1 <= M <= 8) have each left one decode step's dense fp32
// logits (R, ldl_m) and row LSEs (R).  Per row r this kernel forms
//   lp_ens[v] = logsumexp_m(log w_m + (z_m[v] - lse_m))
// -- the log of the weighted arithmetic mean of the members' probabilities --
// for every column v < V and leaves its K largest values, largest first, with
// their column indices (ties to the smaller index) in top_v / top_i: the
// contract of beam_topk_kernel (beam.hip), whose output beam_step_kernel
// consumes unchanged.
//
// Arithmetic, fp32, one fixed order (a relaunch is bit-equal, no atomics):
//   a_m = (z_m - lse_m) + logw_m;  mx = max_m a_m;
//   e   = mx + logf(sum_m expf(a_m - mx))      summed in member order
// with the precise expf / logf (the pass is memory-bound; tests/ensemble_cases.py
// derives its bound from their documented error).  M = 1: no logw, no exp /
// log -- the scan ranks the raw logits and the value is z - lse, bit-equal to
// beam_topk_kernel.
//
// Shape, as beam_topk_kernel: one 256-thread workgroup per row; EN_U columns x
// M members of independent loads are issued before the (mostly rejecting)
// insertions into a lane-local sorted list (static register indices only);
// K rounds of wave arg-max per wave, then wave 0 merges the 4 waves' lists.
// The members' row pointers, LSE pointers and log-weights travel by value in
// the kernel-argument struct: no device-side pointer table, no extra copy.
// Columns V..ldl are never read.  Loads are 4-byte, lane-strided (coalesced);
// 16-byte loads were not measured (profiles/ensemble/README.md).  The list
// insertion, the wave arg-max and the merge are beam_topk_kernel's own
// (topk_common.h), so the two cannot drift apart in their tie rule.
//
// Greedy epilogue (K = 1, seq_out given): lane 0 applies the end-of-sequence
// rule of topk_sample.hip -- unfinished[r] is sticky once a row draws 0 -- and
// writes the sequence column, the next input token and the log-prob; a row
// that had already finished emits 0 with log-prob 0.  Greedy decoding needs no
// further launch per step.
//
// Resources (hipcc -O3, gfx950, code-object metadata): ensemble_topk_kernel<1>
// 87 VGPRs, <2> 96, <4> 90, <8> 102; scratch 0 and no spills in all four;
// LDS 512 B.
#include <cmath>

#include "../common.h"
#include "../launchers.h"
#include "topk_common.h"

namespace cst {

constexpr int EN_MAXK = 16;

template <int MT>
__global__ __launch_bounds__(256) void ensemble_topk_kernel(EnsembleTopkArgs a) {
  __shared__ float s_v[4 * EN_MAXK];
  __shared__ int s_i[4 * EN_MAXK];
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x;
  const int K = a.K, V = a.V, M = a.M;
  const float* x[MT];
  float L[MT], lw[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mm = m < M ? m : 0;  // (slots >= M: masked below, their values never used)
    x[m] = a.logits[mm] + (int64_t)r * a.ldl[mm];
    L[m] = a.lse[mm][r];
    lw[m] = a.logw[mm];
  }
  float bv[EN_MAXK];
  int bi[EN_MAXK];
#pragma unroll
  for (int k = 0; k < EN_MAXK; ++k) bv[k] = -INFINITY, bi[k] = 0x7fffffff;
  float thr = -INFINITY;  // the list's K-th value
  // EN_U columns x M members in flight per chunk (8..32 independent loads)
  constexpr int EN_U = MT <= 2 ? 8 : 4;
  for (int v0 = threadIdx.x; v0 < V; v0 += 256 * EN_U) {
    float xs[EN_U][MT];
#pragma unroll
    for (int u = 0; u < EN_U; ++u) {
      const int v = v0 + 256 * u;
#pragma unroll
      for (int m = 0; m < MT; ++m) xs[u][m] = (v < V && m < M) ? x[m][v] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < EN_U; ++u) {
      float cv;
      if constexpr (MT == 1) {
        cv = xs[u][0];  // ranked on the raw logit, the LSE leaves at the end
      } else {
        float am[MT], mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          am[m] = (xs[u][m] - L[m]) + lw[m];
          if (m < M) mx = fmaxf(mx, am[m]);
        }
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
          if (m < M) s += expf(am[m] - mx);
        cv = mx + logf(s);
      }
      if (v0 + 256 * u >= V) cv = -INFINITY;
      if (!(cv > thr)) continue;
      topk_list_insert<EN_MAXK>(bv, bi, thr, K, cv, v0 + 256 * u);
    }
  }
  topk_block_select<EN_MAXK>(bv, bi, K, s_v, s_i, [&](int k, float best, int besti) {
    if (lane != 0) return;
    const float val = MT == 1 ? best - L[0] : best;
    if (a.top_v != nullptr) {
      a.top_v[(int64_t)r * K + k] = val;
      a.top_i[(int64_t)r * K + k] = besti;
    }
    if (a.seq_out != nullptr) {  // greedy epilogue (K = 1)
      const bool was = a.unfinished[r] != 0;
      int64_t tok = besti;
      a.unfinished[r] = was && tok > 0;  // sticky once the row drew EOS (0)
      if (!was) tok = 0;
      a.seq_out[(int64_t)r * a.out_stride] = tok;
      a.lp_out[(int64_t)r * a.out_stride] = was ? val : 0.f;
      a.next_tok[r] = tok;
    }
  });
}

void launch_ensemble_topk(const EnsembleTopkArgs& a, hipStream_t stream) {
  if (a.M < 1 || a.M > ENS_MAXM) throw std::runtime_error("ensemble_topk: 1 <= M <= 8 members");
  if (a.K < 1 || a.K > EN_MAXK) throw std::runtime_error("ensemble_topk: K must be in [1, 16]");
  if (a.K > a.V) throw std::runtime_error("ensemble_topk: K > vocab_size");
  if (a.seq_out != nullptr &&
      (a.K != 1 || a.unfinished == nullptr || a.lp_out == nullptr || a.next_tok == nullptr))
    throw std::runtime_error("ensemble_topk: the greedy epilogue needs K = 1 and all its outputs");
  if (a.seq_out == nullptr && (a.top_v == nullptr || a.top_i == nullptr))
    throw std::runtime_error("ensemble_topk: no output");
  for (int m = 0; m < a.M; ++m)
    if (a.logits[m] == nullptr || a.lse[m] == nullptr || a.ldl[m] < a.V || !std::isfinite(a.logw[m]))
      throw std::runtime_error("ensemble_topk: member operands (ldl >= V, finite log-weight)");
  if (a.R < 1) return;
  const dim3 grid(a.R), block(256);
  if (a.M == 1)
    hipLaunchKernelGGL((ensemble_topk_kernel<1>), grid, block, 0, stream, a);
  else if (a.M == 2)
    hipLaunchKernelGGL((ensemble_topk_kernel<2>), grid, block, 0, stream, a);
  else if (a.M <= 4)
    hipLaunchKernelGGL((ensemble_topk_kernel<4>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((ensemble_topk_kernel<8>), grid, block, 0, stream, a);
  post_launch("ensemble_topk_kernel", stream);
}

}  // namespace cst
