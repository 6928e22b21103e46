// Validation metrics in token space, on the GPU: the per-hypothesis sufficient
// statistics of corpus BLEU-1..4 and of METEOR (exact + stem stages), from
// which the host evaluates the corpus formulas in fp64
// (cst_captioning_amd/ops/corpus_metrics.py).  ROUGE-L comes from
// rouge_l_kernel (sent_metrics.hip), coco CIDEr from cider_unclipped_kernel
// (cider_d.hip).  Semantics follow cst_captioning_amd/eval/metrics.py
// (Bleu.compute_score, Meteor._align / _stats / _score); the reference tables
// are built once per split by csrc/host/metric_host.cpp.
//
// Work split as in sent_metrics.hip: ONE WAVEFRONT PER HYPOTHESIS, four per
// 256-thread block (grid = ceil(N / 4)); each wave owns its LDS slice, so there
// is no block barrier, no atomics and no communication between waves or
// workgroups.  Outputs are integers (and METEOR's fp64 segment score): the
// corpus sums are exact and do not depend on a reduction order.
#include "../common.h"
#include "../cider_common.h"

namespace cst {

constexpr int CM_MAXT = 64;
constexpr int CM_WAVES = 4;  // hypotheses per block

namespace {
__device__ __forceinline__ int cm_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int cm_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
}  // namespace

// BLEU statistics: the counting part of bleu4_kernel (steps 1-4 there: hypothesis
// n-gram keys and first-occurrence term frequencies in LDS, lanes stride over
// the video's union n-grams adding min(tf, clip count), closest reference
// length).  out[hyp] = correct[4], guess[4], tlen, rlen (10 x int32); a video
// outside the tables or without references gets correct = 0 and rlen = 0.
__global__ __launch_bounds__(64 * CM_WAVES) void bleu_stats_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    int Nv, const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_len,
    const int32_t* __restrict__ vid_ng_off, const int64_t* __restrict__ ng_key,
    const int32_t* __restrict__ ng_cnt, int32_t* __restrict__ out) {
  __shared__ int s_tok[CM_WAVES][CM_MAXT];
  __shared__ uint64_t s_key[CM_WAVES][4][CM_MAXT];
  __shared__ int s_tf[CM_WAVES][4][CM_MAXT];

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x * CM_WAVES + w;
  if (hyp >= N) return;  // (whole wave; no block-level barrier below)

  const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, 0, s_tok[w]);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    uint64_t key = 0;
    if (lane < W - n) {
      bool ok = true;
#pragma unroll
      for (int i = 0; i <= n; ++i) {
        const int t = s_tok[w][lane + i];
        ok = ok && t >= 0 && t < 65535;
        key |= (uint64_t)((t + 1) & 0xffff) << (16 * i);
      }
      if (!ok) key = 0;  // (matches no table entry: a guess, never correct)
    }
    s_key[w][n][lane] = key;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int cnt = W - n;
    int tf = 0;
    if (lane < cnt) {
      const uint64_t key = s_key[w][n][lane];
      bool first = true;
      for (int j = 0; j < cnt; ++j) {
        const bool eq = s_key[w][n][j] == key;
        tf += eq;
        first = first && !(eq && j < lane);
      }
      if (!first) tf = 0;
    }
    s_tf[w][n][lane] = tf;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  const int64_t v64 = hyp_video[hyp];
  const bool vok = v64 >= 0 && v64 < Nv;
  const int v = vok ? (int)v64 : 0;
  const int r0 = vid_ref_off[v], r1 = vok ? vid_ref_off[v + 1] : r0;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  const int g0 = vid_ng_off[v], g1 = vok ? vid_ng_off[v + 1] : g0;
  for (int g = g0 + lane; g < g1; g += 64) {
    const uint64_t key = (uint64_t)ng_key[g];
    const int clip = ng_cnt[g];
    const int n = ngram_order(key) - 1;
    const int cnt = W - n;
    int c = 0;
    for (int j = 0; j < cnt; ++j) {
      if (s_key[w][n][j] == key) c += min(s_tf[w][n][j], clip);
    }
    c0 += n == 0 ? c : 0;
    c1 += n == 1 ? c : 0;
    c2 += n == 2 ? c : 0;
    c3 += n == 3 ? c : 0;
  }
  c0 = cm_wave_sum(c0), c1 = cm_wave_sum(c1), c2 = cm_wave_sum(c2), c3 = cm_wave_sum(c3);
  int best = 0x7fffffff;  // min over (|len_r - len_h|, len_r), both fields <= 64
  for (int r = r0 + lane; r < r1; r += 64) {
    const int lr = ref_len[r];
    best = min(best, (abs(lr - W) << 8) | lr);
  }
  best = cm_wave_min(best);
  if (lane == 0) {
    int32_t* o = out + (int64_t)hyp * 10;
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[4 + k] = max(0, W - k);
    o[8] = W;
    o[9] = r1 > r0 ? (best & 0xff) : 0;
  }
}

// METEOR score of one alignment (Meteor._score): alpha .85, beta .2, gamma .6,
// stem weight .6.  No contraction, so the host twin evaluates the same
// expression tree.
__device__ __forceinline__ double meteor_score(int n_exact, int n_stem, int len_h, int len_r,
                                               int chunks) {
#pragma clang fp contract(off)
  const int np = n_exact + n_stem;
  const double m = (double)n_exact + 0.6 * (double)n_stem;
  if (np <= 0 || len_h <= 0 || len_r <= 0) return 0.0;
  const double P = m / (double)len_h, R = m / (double)len_r;
  const double fmean = P * R / (0.85 * P + (1.0 - 0.85) * R);
  const double frag = (double)chunks / (double)np;
  const double pen = 0.6 * pow(frag, 0.2);
  return (1.0 - pen) * fmean;
}

// METEOR statistics.  Lane i holds hypothesis token i and its stem id, lane j
// token j of the current reference (at most 64 each).  Per reference two stages
// (exact on the token id, then the stem id); inside a stage a WAVE-UNIFORM loop
// over the hypothesis positions i that are not paired yet:
//   candidates = ballot(ref key == key of i) & ~used      (64-bit, bit j)
//   prev = the highest paired position below i            (clz on `paired`)
//   want = j of prev + 1, 0 without one                   (readlane; may be 64)
//   j    = the candidate with the smallest (|j - want|, j): the lowest
//          candidate bit at or above `want` against the highest below it, the
//          lower one on equal distance.
// Chunks: a paired position starts a chunk unless position i - 1 is paired
// with j - 1.  The reference with the largest score wins, the first on ties.
// Leave-one-out: exclude[hyp] = e skips reference e of the video (excluded_ref,
// cider_common.h); best and first-on-ties are over the remaining references.
// out_stats[hyp] = n_exact, n_stem, len_h, len_r, chunks, n_pairs (6 x int32),
// out_score[hyp] the segment score (fp64).
__global__ __launch_bounds__(64 * CM_WAVES) void meteor_stats_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    int Nv, const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_tok_off,
    const int32_t* __restrict__ ref_tok, const int32_t* __restrict__ ref_stem,
    const int32_t* __restrict__ stem_ids, int V, const int64_t* __restrict__ exclude,
    int32_t* __restrict__ out_stats, double* __restrict__ out_score) {
  __shared__ int s_tok[CM_WAVES][CM_MAXT];

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x * CM_WAVES + w;
  if (hyp >= N) return;

  const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, 0, s_tok[w]);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // (-1: past the end, or no stem known: equal to no reference key, which are >= 0)
  const int htok = lane < W ? s_tok[w][lane] : -1;
  const int hstem = (htok >= 0 && htok < V) ? stem_ids[htok] : -1;

  const int64_t v64 = hyp_video[hyp];
  const bool vok = v64 >= 0 && v64 < Nv;
  const int v = vok ? (int)v64 : 0;
  const int r0 = vid_ref_off[v], r1 = vok ? vid_ref_off[v + 1] : r0;

  int b_exact = 0, b_stem = 0, b_lr = 0, b_chunks = 0;
  double b_score = -1.0;
  const int ex = excluded_ref(exclude, hyp, r0, r1);  // (leave-one-out: -1 = none)
  for (int r = r0; r < r1; ++r) {
    if (r == ex) continue;  // (wave-uniform)
    const int o0 = ref_tok_off[r];
    const int n = min(ref_tok_off[r + 1] - o0, 64);
    const int rtok = lane < n ? ref_tok[o0 + lane] : -2;
    const int rstem = lane < n ? ref_stem[o0 + lane] : -2;
    uint64_t used = 0, paired = 0;
    int pj = 0;  // lane i: the reference position paired with hypothesis position i
    int cnt[2] = {0, 0};
#pragma unroll
    for (int stage = 0; stage < 2; ++stage) {
      const int hk_l = stage ? hstem : htok;
      const int rk_l = stage ? rstem : rtok;
      for (int i = 0; i < W; ++i) {
        if ((paired >> i) & 1) continue;
        const int hk = __builtin_amdgcn_readlane(hk_l, i);
        const uint64_t c = __ballot(rk_l == hk) & ~used;
        if (hk < 0 || !c) continue;
        const uint64_t below = paired & ((1ull << i) - 1ull);
        int want = 0;
        if (below) want = __builtin_amdgcn_readlane(pj, 63 - __clzll((long long)below)) + 1;
        const uint64_t lo = want >= 64 ? c : (c & ((1ull << want) - 1ull));
        const uint64_t hi = want >= 64 ? 0ull : (c >> want);
        int j;
        if (!hi) {
          j = 63 - __clzll((long long)lo);
        } else {
          j = want + (__ffsll((long long)hi) - 1);
          if (lo) {
            const int jb = 63 - __clzll((long long)lo);
            if (want - jb <= j - want) j = jb;
          }
        }
        used |= 1ull << j;
        paired |= 1ull << i;
        if (lane == i) pj = j;
        cnt[stage] += 1;
      }
    }
    const bool mine = (paired >> lane) & 1;
    const int pj_prev = __shfl_up(pj, 1, 64);
    const bool cont = lane > 0 && ((paired >> (lane - 1)) & 1) && pj_prev + 1 == pj;
    const int chunks = __popcll(__ballot(mine && !cont));
    const double sc = meteor_score(cnt[0], cnt[1], W, n, chunks);
    if (sc > b_score) {
      b_score = sc;
      b_exact = cnt[0], b_stem = cnt[1], b_lr = n, b_chunks = chunks;
    }
  }
  if (lane == 0) {
    int32_t* o = out_stats + (int64_t)hyp * 6;
    const bool any = r1 > r0;
    o[0] = b_exact, o[1] = b_stem, o[2] = any ? W : 0, o[3] = b_lr, o[4] = b_chunks;
    o[5] = b_exact + b_stem;
    out_score[hyp] = any ? b_score : 0.0;
  }
}

void launch_bleu_stats(const int64_t* hyps, int T, const int64_t* hyp_video, int N, int Nv,
                       const int32_t* vid_ref_off, const int32_t* ref_len,
                       const int32_t* vid_ng_off, const int64_t* ng_key, const int32_t* ng_cnt,
                       int32_t* out, hipStream_t stream) {
  if (N <= 0) return;
  dim3 grid((N + CM_WAVES - 1) / CM_WAVES), block(64 * CM_WAVES);
  hipLaunchKernelGGL(bleu_stats_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, Nv,
                     vid_ref_off, ref_len, vid_ng_off, ng_key, ng_cnt, out);
  post_launch("bleu_stats_kernel", stream);
}

void launch_meteor_stats(const int64_t* hyps, int T, const int64_t* hyp_video, int N, int Nv,
                         const int32_t* vid_ref_off, const int32_t* ref_tok_off,
                         const int32_t* ref_tok, const int32_t* ref_stem,
                         const int32_t* stem_ids, int V, const int64_t* exclude,
                         int32_t* out_stats, double* out_score, hipStream_t stream) {
  if (N <= 0) return;
  dim3 grid((N + CM_WAVES - 1) / CM_WAVES), block(64 * CM_WAVES);
  hipLaunchKernelGGL(meteor_stats_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, Nv,
                     vid_ref_off, ref_tok_off, ref_tok, ref_stem, stem_ids, V, exclude, out_stats,
                     out_score);
  post_launch("meteor_stats_kernel", stream);
}

}  // namespace cst
