// Mixed-metric RL reward (--reward_mix): w_c * CIDEr-D + w_b * BLEU-4 +
// w_r * ROUGE-L of sampled captions in ONE launch, safe inside graph capture.
// Every term is what cider_d_kernel (x10 scale, the dataset's df table),
// bleu4_kernel and rouge_l_kernel return: the bodies are theirs
// (reward_bodies.h), run here on one 256-thread block per hypothesis:
//   1. wave 0 compacts the hypothesis once (compact_hypothesis);
//   2. wave n builds the order-(n+1) packed keys, with BLEU's rule (a token the
//      16-bit packing cannot hold gives key 0), and their first-occurrence term
//      frequencies: both are shared by CIDEr-D (tf * idf, per-order norms) and
//      BLEU (integer tf);
//   3. the waves split the metrics: BLEU-4 is the work of one wave (the last),
//      ROUGE-L of one wave (the one before it), the waves that are left (2 of
//      4 with all three metrics) split the video's references for CIDEr-D;
//   4. thread 0 adds the CIDEr-D partial sums, and blends in fp32:
//      out = ((w_c * c) + (w_b * b)) + (w_r * r), each product and sum rounded
//      once (no contraction); parts = (c, b, r).
// A metric of weight 0 is skipped wave-uniformly (its waves go to CIDEr-D), its
// column is exactly 0 and its table pointers may be null.  No leave-one-out.
// Deterministic: fixed-order wave / block reductions, no atomics.  The CIDEr-D
// partial sums are grouped by the waves that computed them, so that column may
// differ from cider_d_kernel's in the last bits; BLEU / ROUGE are integer
// statistics and the same fp64 formula: bit-equal to their kernels.
#include "../common.h"
#include "../cider_common.h"
#include "../launchers.h"
#include "reward_bodies.h"

namespace cst {

__global__ __launch_bounds__(256) void reward_mix_kernel(
    const int64_t* __restrict__ hyps, int T, const int64_t* __restrict__ hyp_video, int N,
    CiderTables ct, int cider_nv, BleuTables bt, RougeTables rt, int use_eos, float w_c,
    float w_b, float w_r, float* __restrict__ out, float* __restrict__ parts) {
  __shared__ int s_tok[RW_MAXT];
  __shared__ uint64_t s_key[4][RW_MAXT];
  __shared__ int s_tf[4][RW_MAXT];
  __shared__ float s_val[4][RW_MAXT];
  __shared__ float s_norm[4];
  __shared__ float s_part[4];
  __shared__ float s_br[2];
  __shared__ int s_W;

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int hyp = blockIdx.x;  // (grid = N)
  const bool has_c = w_c != 0.f, has_b = w_b != 0.f, has_r = w_r != 0.f;

  if (w == 0) {
    const int W = compact_hypothesis(hyps + (int64_t)hyp * T, T, lane, use_eos, s_tok);
    if (lane == 0) s_W = W;
  }
  __syncthreads();
  const int W = s_W;
  if (has_c || has_b) s_key[w][lane] = ngram_key<true>(s_tok, W, w, lane);
  __syncthreads();
  if (has_c || has_b) {
    const int tf = first_tf(s_key[w], W - w, lane);
    s_tf[w][lane] = tf;
    if (has_c) {  // (tf > 0: a first occurrence)
      const float v = tf > 0 ? cider_tfidf(ct, s_key[w][lane], tf) : 0.f;
      s_val[w][lane] = v;
      const float nrm = sqrtf(wave_sum(v * v));
      if (lane == 0) s_norm[w] = nrm;
    }
  }
  __syncthreads();

  // the waves' jobs (wave-uniform): BLEU wave 3, ROUGE the wave below it, CIDEr-D
  // the nc waves from 0
  const int wb = has_b ? 3 : -1;
  const int wr = has_r ? (has_b ? 2 : 3) : -1;
  const int nc = 4 - (has_b ? 1 : 0) - (has_r ? 1 : 0);
  int nref = 0;
  if (w == wb) {
    const float b = bleu4_refs(bt, s_key, s_tf, W, hyp, hyp_video, nullptr, lane);
    if (lane == 0) s_br[0] = b;
  } else if (w == wr) {
    const int htok = lane < W ? s_tok[lane] : -1;
    const float r = rouge_l_refs(rt, htok, W, hyp, hyp_video, nullptr, lane);
    if (lane == 0) s_br[1] = r;
  } else {
    float total = 0.f;
    if (has_c) {
      const int64_t v64 = hyp_video[hyp];
      const bool vok = v64 >= 0 && v64 < cider_nv;  // (a video outside the tables scores 0)
      const int v = vok ? (int)v64 : 0;
      const int r0 = ct.vid_ref_off[v], r1 = vok ? ct.vid_ref_off[v + 1] : r0;
      const float norm_h[4] = {s_norm[0], s_norm[1], s_norm[2], s_norm[3]};
      total = cider_refs<true>(ct, s_key, s_val, W, norm_h, r0, r1, -1, w, nc, lane);
      nref = r1 - r0;
    }
    if (lane == 0) s_part[w] = total;
  }
  if (w >= nc && lane == 0) s_part[w] = 0.f;  // (not a CIDEr-D wave: adds nothing)
  __syncthreads();
  if (threadIdx.x == 0) {  // (wave 0: always a CIDEr-D wave, nref is its own)
    const float c = has_c ? cider_final(s_part, nref) : 0.f;
    const float b = has_b ? s_br[0] : 0.f;
    const float r = has_r ? s_br[1] : 0.f;
    parts[(int64_t)hyp * 3 + 0] = c;
    parts[(int64_t)hyp * 3 + 1] = b;
    parts[(int64_t)hyp * 3 + 2] = r;
    out[hyp] = __fadd_rn(__fadd_rn(__fmul_rn(w_c, c), __fmul_rn(w_b, b)), __fmul_rn(w_r, r));
  }
}

void launch_reward_mix(const int64_t* hyps, int T, const int64_t* hyp_video, int N,
                       const MixCiderArgs& c, const MixSentArgs& s, int use_eos, float w_c,
                       float w_b, float w_r, float* out, float* parts, hipStream_t stream) {
  if (N <= 0) return;
  const CiderTables ct = {c.ht_keys, c.ht_vals, c.ht_cap, c.vid_ref_off, c.ref_ng_off,
                          c.ref_norm, c.ref_len, c.ng_key, c.ng_val,     c.log_ref_len};
  const BleuTables bt = {s.Nv,     s.vid_ref_off, s.ref_len, s.vid_ng_off,
                         s.ng_key, s.ng_cnt,      nullptr,   nullptr};
  const RougeTables rt = {s.Nv, s.vid_ref_off, s.ref_tok_off, s.ref_tok};
  dim3 grid(N), block(256);
  hipLaunchKernelGGL(reward_mix_kernel, grid, block, 0, stream, hyps, T, hyp_video, N, ct, c.Nv,
                     bt, rt, use_eos, w_c, w_b, w_r, out, parts);
  post_launch("reward_mix_kernel", stream);
}

}  // namespace cst
