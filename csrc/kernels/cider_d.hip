// K5: CIDEr-D of sampled captions, on the GPU.
//
// Replaces the per-iteration host round trip of the reference
// (/root/reference/train.py:185,198-199 -> utils.py:229-324 -> external
// pyciderevalcap CiderD on the CPU) with one launch.  Reference n-gram vectors
// (tf-idf values, per-order norms, bigram "lengths") are precomputed once per
// dataset by csrc/host/cider_host.cpp; this kernel only processes hypotheses.
//
// One 256-thread block per hypothesis:
//   1. token compaction with ballots, reproducing array_to_str
//      (utils.py:135-152): drop BOS (=1) anywhere, stop at the first EOS (=0)
//      and keep that "0" when use_eos;
//   2. packed n-gram keys (n<=4) in LDS; term frequencies by an in-wave
//      O(W) scan, counted once at the first occurrence (later duplicates get
//      value 0, which contributes exactly 0 to the clipped dot product);
//   3. idf from the df hash table in HBM, per-order norms by wave reduction;
//   4. the 4 waves split the video's references; for each one, lanes stride over its
//      unique n-grams, look each up among the hypothesis n-grams in LDS
//      (broadcast reads), accumulate min(vh, vr) * vr per order, normalise,
//      apply exp(-(lh - lr)^2 / (2 * 6^2));
//   5. score = 10 * sum_refs mean_n(val_n) / n_refs.
// Leave-one-out (GT consensus scores, ops/consensus.py): exclude[hyp] = e skips
// reference e of the hypothesis' video (excluded_ref, cider_common.h) and the
// mean divides by the references used.
// Deterministic: fixed-order wave/block reductions, no atomics.
// Steps 2-5 are functions of reward_bodies.h, which reward_mix_kernel
// (reward_mix.hip) calls too.
#include "../common.h"
#include "../cider_common.h"
#include "reward_bodies.h"

namespace cst {

constexpr int CIDER_MAXT = 64;

// One 256-thread block per hypothesis: wave 0 builds the hypothesis vector
// (steps 1-3) in LDS, then the 4 waves split the video's references.
// CLIPPED: CIDEr-D (min(vh, vr) * vr and the Gaussian length penalty).  false:
// coco CIDEr, the validation metric (vh * vr, penalty 1; csrc/kernels/
// corpus_metrics.hip describes the validation scorer).
template <bool CLIPPED>
__device__ __forceinline__ void cider_body(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    const int64_t* __restrict__ ht_keys, const float* __restrict__ ht_vals, uint32_t ht_cap,
    const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_ng_off,
    const float* __restrict__ ref_norm, const int32_t* __restrict__ ref_len,
    const int64_t* __restrict__ ng_key, const float* __restrict__ ng_val, float log_ref_len,
    int use_eos, const int64_t* __restrict__ exclude, float* __restrict__ out) {
  __shared__ int s_tok[CIDER_MAXT];
  __shared__ uint64_t s_key[4][CIDER_MAXT];
  __shared__ float s_val[4][CIDER_MAXT];
  __shared__ float s_norm[4];
  __shared__ float s_part[4];
  __shared__ int s_W;

  const int w = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x;
  const CiderTables tab = {ht_keys, ht_vals, ht_cap, vid_ref_off, ref_ng_off,
                           ref_norm, ref_len, ng_key,  ng_val,     log_ref_len};

  // -- 1. compaction (wave 0) ----------------------------------------------------
  if (w == 0) {
    const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, use_eos, s_tok);
    if (lane == 0) s_W = W;
  }
  __syncthreads();
  const int W = s_W;
  // -- 2. packed n-gram keys: wave n builds the order-(n+1) keys ------------------
  s_key[w][lane] = ngram_key<false>(s_tok, W, w, lane);
  __syncthreads();
  // -- 3. tf (first occurrence), idf, per-order norm: wave n handles order n+1 ----
  {
    const float v = cider_hyp_value(tab, s_key[w], W - w, lane);
    s_val[w][lane] = v;
    const float nrm = sqrtf(wave_sum(v * v));
    if (lane == 0) s_norm[w] = nrm;
  }
  __syncthreads();
  const float norm_h[4] = {s_norm[0], s_norm[1], s_norm[2], s_norm[3]};

  // -- 4. references, split over the 4 waves --------------------------------------
  const int v = (int)hyp_video[hyp];
  const int r0 = vid_ref_off[v], r1 = vid_ref_off[v + 1];
  const int ex = excluded_ref(exclude, hyp, r0, r1);  // (leave-one-out: -1 = none)
  const float total = cider_refs<CLIPPED>(tab, s_key, s_val, W, norm_h, r0, r1, ex, w, 4, lane);
  if (lane == 0) s_part[w] = total;
  __syncthreads();
  // (the mean divides by the references used)
  if (threadIdx.x == 0) out[hyp] = cider_final(s_part, r1 - r0 - (ex >= 0 ? 1 : 0));
}

__global__ __launch_bounds__(256) void cider_d_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    const int64_t* __restrict__ ht_keys, const float* __restrict__ ht_vals, uint32_t ht_cap,
    const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_ng_off,
    const float* __restrict__ ref_norm, const int32_t* __restrict__ ref_len,
    const int64_t* __restrict__ ng_key, const float* __restrict__ ng_val, float log_ref_len,
    int use_eos, const int64_t* __restrict__ exclude, float* __restrict__ out) {
  cider_body<true>(hyps, T, hyp_video, N, ht_keys, ht_vals, ht_cap, vid_ref_off, ref_ng_off,
                   ref_norm, ref_len, ng_key, ng_val, log_ref_len, use_eos, exclude, out);
}

__global__ __launch_bounds__(256) void cider_unclipped_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    const int64_t* __restrict__ ht_keys, const float* __restrict__ ht_vals, uint32_t ht_cap,
    const int32_t* __restrict__ vid_ref_off, const int32_t* __restrict__ ref_ng_off,
    const float* __restrict__ ref_norm, const int32_t* __restrict__ ref_len,
    const int64_t* __restrict__ ng_key, const float* __restrict__ ng_val, float log_ref_len,
    int use_eos, const int64_t* __restrict__ exclude, float* __restrict__ out) {
  cider_body<false>(hyps, T, hyp_video, N, ht_keys, ht_vals, ht_cap, vid_ref_off, ref_ng_off,
                    ref_norm, ref_len, ng_key, ng_val, log_ref_len, use_eos, exclude, out);
}

void launch_cider_d(const int64_t* hyps, int T, const int64_t* hyp_video, int N,
                    const int64_t* ht_keys, const float* ht_vals, uint32_t ht_cap,
                    const int32_t* vid_ref_off, const int32_t* ref_ng_off,
                    const float* ref_norm, const int32_t* ref_len, const int64_t* ng_key,
                    const float* ng_val, float log_ref_len, int use_eos,
                    const int64_t* exclude, float* out, hipStream_t stream) {
  if (N <= 0) return;
  dim3 grid(N), block(256);
  hipLaunchKernelGGL(cider_d_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, ht_keys,
                     ht_vals, ht_cap, vid_ref_off, ref_ng_off, ref_norm, ref_len, ng_key,
                     ng_val, log_ref_len, use_eos, exclude, out);
  post_launch("cider_d_kernel", stream);
}

// coco CIDEr (unclipped, no length penalty) on the same tables; T <= 64.
void launch_cider_unclipped(const int64_t* hyps, int T, const int64_t* hyp_video, int N,
                            const int64_t* ht_keys, const float* ht_vals, uint32_t ht_cap,
                            const int32_t* vid_ref_off, const int32_t* ref_ng_off,
                            const float* ref_norm, const int32_t* ref_len,
                            const int64_t* ng_key, const float* ng_val, float log_ref_len,
                            int use_eos, const int64_t* exclude, float* out,
                            hipStream_t stream) {
  if (N <= 0) return;
  dim3 grid(N), block(256);
  hipLaunchKernelGGL(cider_unclipped_kernel, grid, block, 0, stream, hyps, T, hyp_video, N,
                     ht_keys, ht_vals, ht_cap, vid_ref_off, ref_ng_off, ref_norm, ref_len, ng_key,
                     ng_val, log_ref_len, use_eos, exclude, out);
  post_launch("cider_unclipped_kernel", stream);
}

}  // namespace cst
