// Pieces of the per-row top-K of a 256-thread workgroup, shared by
// beam_topk_kernel (beam.hip) and ensemble_topk_kernel (ensemble.hip) so that
// the two keep one tie rule (ties to the smaller index): the wave arg-max, the
// lane-local sorted list's insertion, and the selection (K rounds of wave
// arg-max per wave, then wave 0 merges the 4 waves' candidates).
#pragma once
#include "../common.h"

namespace cst {

__device__ __forceinline__ void wave_argmax(float& best, int& besti) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (ov > best || (ov == best && oi < besti)) best = ov, besti = oi;
  }
}

// (cv, ci) into the lane's sorted list bv / bi (K live slots of MAXK; static
// register indices only).  Strict >: of equal values the one inserted earlier
// -- the smaller index, as a lane meets its columns in increasing order --
// stays ahead.  thr: the list's K-th value; callers skip values not above it.
template <int MAXK>
__device__ __forceinline__ void topk_list_insert(float (&bv)[MAXK], int (&bi)[MAXK], float& thr,
                                                 int K, float cv, int ci) {
#pragma unroll
  for (int p = 0; p < MAXK; ++p) {
    if (p < K && cv > bv[p]) {
      const float tv = bv[p];
      const int ti = bi[p];
      bv[p] = cv, bi[p] = ci;
      cv = tv, ci = ti;
    }
  }
#pragma unroll
  for (int p = 0; p < MAXK; ++p) thr = p == K - 1 ? bv[p] : thr;
}

// The workgroup's K best from its 256 lanes' lists, largest first: emit(k,
// value, index) runs on every lane of wave 0 with the same arguments; the
// other waves return false after the barrier.  s_v / s_i: 4 * MAXK LDS slots.
template <int MAXK, class Emit>
__device__ __forceinline__ bool topk_block_select(float (&bv)[MAXK], int (&bi)[MAXK], int K,
                                                  float* s_v, int* s_i, Emit emit) {
  static_assert(4 * MAXK == 64, "one lane of wave 0 per candidate");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // K rounds of wave arg-max over the lanes' list heads; the winner shifts
  for (int k = 0; k < K; ++k) {
    float best = bv[0];
    int besti = bi[0];
    wave_argmax(best, besti);
    if (bi[0] == besti) {
#pragma unroll
      for (int p = 0; p + 1 < MAXK; ++p) bv[p] = bv[p + 1], bi[p] = bi[p + 1];
      bv[MAXK - 1] = -INFINITY, bi[MAXK - 1] = 0x7fffffff;
    }
    if (lane == 0) s_v[w * MAXK + k] = best, s_i[w * MAXK + k] = besti;
  }
  __syncthreads();
  if (w != 0) return false;
  // the 4 waves' sorted candidate lists: lane l holds candidate l
  const int ww = lane / MAXK, kk = lane % MAXK;
  const bool have = kk < K;
  float cv = have ? s_v[ww * MAXK + kk] : -INFINITY;
  int ci = have ? s_i[ww * MAXK + kk] : 0x7fffffff;
  for (int k = 0; k < K; ++k) {
    float best = cv;
    int besti = ci;
    wave_argmax(best, besti);
    if (ci == besti && cv == best) cv = -INFINITY, ci = 0x7fffffff;
    emit(k, best, besti);
  }
  return true;
}

}  // namespace cst
