// Sentence-level BLEU-4 and ROUGE-L of sampled captions, on the GPU: the
// --eval_metric Bleu_4 / ROUGE_L rewards of SCST / CST training without a host
// round trip (one launch, safe inside graph capture).  Scores follow
// cst_captioning_amd/eval/metrics.py (Bleu per-sentence scores, Rouge.calc_score).
// The reference tables are built once per dataset by csrc/host/metric_host.cpp.
//
// Work split, both kernels: ONE WAVEFRONT PER HYPOTHESIS, four per 256-thread
// block (grid = ceil(N / 4)).  Unlike cider_d_kernel (one block per hypothesis,
// float tf-idf work per reference) the per-hypothesis work here is a few
// hundred integer compares, so a block per hypothesis would leave three waves
// idle behind wave-level reductions; a wave per hypothesis needs no
// __syncthreads at all (each wave owns its LDS slice) and the step's 1,344
// hypotheses give 336 blocks for 256 CUs.  Waves past N exit at once.
//
// Deterministic: integer counts, fixed-order wave reductions, no atomics, no
// communication between waves or workgroups.  The final formulas are evaluated
// in double by one lane and rounded once to fp32.
#include "../common.h"
#include "../cider_common.h"

namespace cst {

constexpr int SM_MAXT = 64;
constexpr int SM_WAVES = 4;  // hypotheses per block

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// BLEU-4.  Per wave:
//   1. compaction (compact_hypothesis, shared with cider_d_kernel);
//   2. per order n the packed keys of the hypothesis n-grams in LDS and their
//      term frequency, kept at the first occurrence only (later duplicates get
//      0, so a reference n-gram that finds several equal keys adds tf once).
//      An n-gram with a token the 16-bit packing cannot hold gets key 0, which
//      no table entry has: it counts as a guess and never as a match;
//   3. lanes stride over the video's union n-grams (ascending keys: grouped by
//      order), look each up among the hypothesis keys of its order (broadcast
//      LDS reads) and add min(tf, clip count) to correct[order];
//   4. closest reference length = min over (|len_r - len_h|, len_r), packed
//      into one int (both fields <= 64);
//   5. lane 0: prod_k (correct_k + 1e-15) / (guess_k + 1e-9), ^(1/4), brevity
//      penalty exp(1 - 1/ratio) when ratio < 1; a video without references: 0.
// Leave-one-out (exclude[hyp] = e, excluded_ref in cider_common.h): the clip
// count is a maximum over the references, so the table keeps per union n-gram
// the reference that alone attains it (ng_arg, -1 when several do) and the
// largest count among the others (ng_cnt2): clip = ng_arg == e ? ng_cnt2 :
// ng_cnt; the closest-length reduction skips reference e.
__global__ __launch_bounds__(64 * SM_WAVES) void bleu4_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    int Nv, const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_len,
    const int32_t* __restrict__ vid_ng_off, const int64_t* __restrict__ ng_key,
    const int32_t* __restrict__ ng_cnt, const int32_t* __restrict__ ng_cnt2,
    const int32_t* __restrict__ ng_arg, int use_eos, const int64_t* __restrict__ exclude,
    float* __restrict__ out) {
  __shared__ int s_tok[SM_WAVES][SM_MAXT];
  __shared__ uint64_t s_key[SM_WAVES][4][SM_MAXT];
  __shared__ int s_tf[SM_WAVES][4][SM_MAXT];

  // (readfirstlane: the compiler then knows the wave index, and with it the video
  // and its table ranges, to be wave-uniform: scalar loads and loop counters)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x * SM_WAVES + w;
  if (hyp >= N) return;  // (whole wave; no block-level barrier below)

  const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, use_eos, s_tok[w]);
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
      if (!ok) key = 0;
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
  const bool vok = v64 >= 0 && v64 < Nv;  // (a video outside the tables scores 0)
  const int v = vok ? (int)v64 : 0;
  const int r0 = vid_ref_off[v], r1 = vok ? vid_ref_off[v + 1] : r0;
  // leave-one-out: the in-video index of the reference left out, -1 for none
  // (wave-uniform; only then are ng_cnt2 / ng_arg read)
  const int ex = excluded_ref(exclude, hyp, r0, r1);
  const int e = ex >= 0 ? ex - r0 : -1;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  const int g0 = vid_ng_off[v], g1 = vok ? vid_ng_off[v + 1] : g0;
  for (int g = g0 + lane; g < g1; g += 64) {
    const uint64_t key = (uint64_t)ng_key[g];
    int clip = ng_cnt[g];
    if (e >= 0 && ng_arg[g] == e) clip = ng_cnt2[g];  // (0: adds nothing)
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
  const int correct[4] = {wave_sum_i(c0), wave_sum_i(c1), wave_sum_i(c2), wave_sum_i(c3)};
  int best = 0x7fffffff;
  for (int r = r0 + lane; r < r1; r += 64) {
    const int lr = ref_len[r];
    if (r != ex) best = min(best, (abs(lr - W) << 8) | lr);
  }
  best = wave_min_i(best);
  if (lane == 0) {
    float res = 0.f;
    if (r1 > r0) {
      const double tiny = 1e-15, small = 1e-9;
      const int rlen = best & 0xff;
      double b = 1.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        b *= ((double)correct[k] + tiny) / ((double)max(0, W - k) + small);
      double s = pow(b, 0.25);
      const double ratio = ((double)W + tiny) / ((double)rlen + small);
      if (ratio < 1.0) s *= exp(1.0 - 1.0 / ratio);
      res = (float)s;
    }
    out[hyp] = res;
  }
}

// ROUGE-L.  Per wave: compaction, then lane j keeps hypothesis token j (-1 past
// the end: never equal to a reference token, which are >= 0).  The video's
// references are looped one at a time (a video may have more than 64); lane a
// loads token a of the reference (lengths <= 64), the next reference's load is
// issued before the current one is processed.  The LCS is the bit-parallel
// recurrence on one 64-bit word, bit j = hypothesis position j:
//   M = ballot(hyp_tok == ref_tok[a]);  U = V & M;  V = (V + U) | (V - U)
// starting from V = ~0; LCS = number of zero bits of V.  Everything in it is
// wave-uniform.  P = max_r lcs_r / len_h and R = max_r lcs_r / len_r are
// tracked separately as exact integer fractions (cross-multiplied compares;
// the correctly rounded quotient of the largest fraction is the largest of the
// rounded quotients) and divided once in double at the end.
// Leave-one-out: exclude[hyp] = e skips reference e of the video (excluded_ref).
__global__ __launch_bounds__(64 * SM_WAVES) void rouge_l_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    int Nv, const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_tok_off,
    const int32_t* __restrict__ ref_tok, int use_eos, const int64_t* __restrict__ exclude,
    float* __restrict__ out) {
  __shared__ int s_tok[SM_WAVES][SM_MAXT];

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x * SM_WAVES + w;
  if (hyp >= N) return;

  const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, use_eos, s_tok[w]);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int htok = lane < W ? s_tok[w][lane] : -1;

  const int64_t v64 = hyp_video[hyp];
  const bool vok = v64 >= 0 && v64 < Nv;  // (a video outside the tables scores 0)
  const int v = vok ? (int)v64 : 0;
  const int r0 = vid_ref_off[v], r1 = vok ? vid_ref_off[v + 1] : r0;
  int best_l = 0;             // max lcs (precision: the denominator len_h is shared)
  int rec_l = 0, rec_n = 1;   // max lcs / len_r as a fraction
  // leave-one-out: the loop walks the references other than `ex` (-1: all of
  // them); `r` is the reference being processed, `rn` the one after it, both
  // stepped over `ex`, so the prefetch never loads the excluded row
  const int ex = excluded_ref(exclude, hyp, r0, r1);
  int o0 = 0, o1 = 0, nxt = -2;
  int r = r0 == ex ? r0 + 1 : r0;
  if (r < r1) {
    o0 = ref_tok_off[r];
    o1 = ref_tok_off[r + 1];
    nxt = lane < min(o1 - o0, 64) ? ref_tok[o0 + lane] : -2;
  }
  while (r < r1) {
    const int n = min(o1 - o0, 64);
    const int rtok = nxt;
    const int rn = r + 1 == ex ? r + 2 : r + 1;
    if (rn < r1) {  // prefetch the next reference
      o0 = ref_tok_off[rn];
      o1 = ref_tok_off[rn + 1];
      nxt = lane < min(o1 - o0, 64) ? ref_tok[o0 + lane] : -2;
    }
    r = rn;
    uint64_t V = ~0ull;
    for (int a = 0; a < n; ++a) {
      const int c = __builtin_amdgcn_readlane(rtok, a);
      const uint64_t M = __ballot(htok == c);
      const uint64_t U = V & M;
      V = (V + U) | (V - U);
    }
    const int l = __popcll(~V);
    best_l = max(best_l, l);
    if (n > 0 && l * rec_n > rec_l * n) rec_l = l, rec_n = n;
  }
  if (lane == 0) {
    float res = 0.f;
    if (W > 0 && best_l > 0 && rec_l > 0) {
      const double beta = 1.2, b2 = beta * beta;
      const double p = (double)best_l / (double)W;
      const double rc = (double)rec_l / (double)rec_n;
      res = (float)(((1.0 + b2) * p * rc) / (rc + b2 * p));
    }
    out[hyp] = res;
  }
}

void launch_bleu4(const int64_t* hyps, int T, const int64_t* hyp_video, int N, int Nv,
                  const int32_t* vid_ref_off, const int32_t* ref_len, const int32_t* vid_ng_off,
                  const int64_t* ng_key, const int32_t* ng_cnt, const int32_t* ng_cnt2,
                  const int32_t* ng_arg, int use_eos, const int64_t* exclude, float* out,
                  hipStream_t stream) {
  if (!ng_cnt2 || !ng_arg) exclude = nullptr;  // (callers check: no tables, no exclusion)
  if (N <= 0) return;
  dim3 grid((N + SM_WAVES - 1) / SM_WAVES), block(64 * SM_WAVES);
  hipLaunchKernelGGL(bleu4_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, Nv, vid_ref_off,
                     ref_len, vid_ng_off, ng_key, ng_cnt, ng_cnt2, ng_arg, use_eos, exclude, out);
  post_launch("bleu4_kernel", stream);
}

void launch_rouge_l(const int64_t* hyps, int T, const int64_t* hyp_video, int N, int Nv,
                    const int32_t* vid_ref_off, const int32_t* ref_tok_off,
                    const int32_t* ref_tok, int use_eos, const int64_t* exclude, float* out,
                    hipStream_t stream) {
  if (N <= 0) return;
  dim3 grid((N + SM_WAVES - 1) / SM_WAVES), block(64 * SM_WAVES);
  hipLaunchKernelGGL(rouge_l_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, Nv, vid_ref_off,
                     ref_tok_off, ref_tok, use_eos, exclude, out);
  post_launch("rouge_l_kernel", stream);
}

}  // namespace cst
