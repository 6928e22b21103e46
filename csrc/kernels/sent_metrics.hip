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
//
// The bodies (keys, term frequencies, the reference loops and the final
// formulas) are functions of reward_bodies.h, which reward_mix_kernel
// (reward_mix.hip) calls too; the kernels here do the compaction and own the LDS.
#include "../common.h"
#include "../cider_common.h"
#include "reward_bodies.h"

namespace cst {

constexpr int SM_MAXT = 64;
constexpr int SM_WAVES = 4;  // hypotheses per block

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
  for (int n = 0; n < 4; ++n) s_key[w][n][lane] = ngram_key<true>(s_tok[w], W, n, lane);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int n = 0; n < 4; ++n) s_tf[w][n][lane] = first_tf(s_key[w][n], W - n, lane);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  const BleuTables tab = {Nv, vid_ref_off, ref_len, vid_ng_off, ng_key, ng_cnt, ng_cnt2, ng_arg};
  const float res = bleu4_refs(tab, s_key[w], s_tf[w], W, hyp, hyp_video, exclude, lane);
  if (lane == 0) out[hyp] = res;
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
  const RougeTables tab = {Nv, vid_ref_off, ref_tok_off, ref_tok};
  const float res = rouge_l_refs(tab, htok, W, hyp, hyp_video, exclude, lane);
  if (lane == 0) out[hyp] = res;
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
