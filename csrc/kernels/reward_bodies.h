// Device bodies of the sentence reward kernels: the pieces of cider_d_kernel
// (cider_d.hip), bleu4_kernel and rouge_l_kernel (sent_metrics.hip), as
// functions of the hypothesis index and the LDS they work on, so that
// reward_mix_kernel (reward_mix.hip) runs the same code on one block per
// hypothesis.  What each piece computes is described at the kernel that
// introduced it.
#pragma once
#include "../common.h"
#include "../cider_common.h"

namespace cst {

constexpr int RW_MAXT = 64;  // tokens of a hypothesis / reduced reference

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

// Packed key of the order-(n+1) n-gram that starts at position `lane` of the W
// compacted tokens (0 past the last one).  CHECKED (BLEU's rule): an n-gram
// with a token the 16-bit packing cannot hold gets key 0, which no table entry
// has; unchecked (cider_d_kernel) the caller guarantees ids <= 65,534.
template <bool CHECKED>
__device__ __forceinline__ uint64_t ngram_key(const int* s_tok, int W, int n, int lane) {
  uint64_t key = 0;
  if (lane < W - n) {
    if (CHECKED) {
      bool ok = true;
      for (int i = 0; i <= n; ++i) {
        const int t = s_tok[lane + i];
        ok = ok && t >= 0 && t < 65535;
        key |= (uint64_t)((t + 1) & 0xffff) << (16 * i);
      }
      if (!ok) key = 0;
    } else {
      for (int i = 0; i <= n; ++i) key |= (uint64_t)(s_tok[lane + i] + 1) << (16 * i);
    }
  }
  return key;
}

// Term frequency of `key` (this lane's, lane < cnt) among the cnt keys of its
// order, and whether this lane holds its first occurrence.
__device__ __forceinline__ int key_count(const uint64_t* s_key_n, int cnt, int lane, uint64_t key,
                                         bool* is_first) {
  int tf = 0;
  bool first = true;
  for (int j = 0; j < cnt; ++j) {
    const bool eq = s_key_n[j] == key;
    tf += eq;
    first = first && !(eq && j < lane);
  }
  *is_first = first;
  return tf;
}

// The same, kept at the first occurrence only: 0 for a later duplicate and for
// lane >= cnt.
__device__ __forceinline__ int first_tf(const uint64_t* s_key_n, int cnt, int lane) {
  int tf = 0;
  if (lane < cnt) {
    bool first;
    tf = key_count(s_key_n, cnt, lane, s_key_n[lane], &first);
    if (!first) tf = 0;
  }
  return tf;
}

// ---- CIDEr-D ------------------------------------------------------------------
struct CiderTables {
  const int64_t* ht_keys;
  const float* ht_vals;
  uint32_t ht_cap;
  const int32_t* vid_ref_off;
  const int32_t* ref_ng_off;
  const float* ref_norm;
  const int32_t* ref_len;
  const int64_t* ng_key;
  const float* ng_val;
  float log_ref_len;
};

// tf * idf of an n-gram (idf from the df hash table in HBM)
__device__ __forceinline__ float cider_tfidf(const CiderTables& t, uint64_t key, int tf) {
  const float df = df_lookup(t.ht_keys, t.ht_vals, t.ht_cap, key);
  return (float)tf * (t.log_ref_len - __logf(fmaxf(1.f, df)));
}

// tf-idf value of this lane's n-gram among the cnt of its order, kept at the
// first occurrence (a later duplicate gets 0, which adds exactly nothing).
__device__ __forceinline__ float cider_hyp_value(const CiderTables& t, const uint64_t* s_key_n,
                                                 int cnt, int lane) {
  float v = 0.f;
  if (lane < cnt) {
    const uint64_t key = s_key_n[lane];
    bool first;
    const int tf = key_count(s_key_n, cnt, lane, key, &first);
    if (first) v = cider_tfidf(t, key, tf);
  }
  return v;
}

// The references r0 + part, r0 + part + nparts, ... < r1 of the hypothesis'
// video (but `ex`), by one whole wave: the sum over them of sum_n val_n * pen.
template <bool CLIPPED>
__device__ __forceinline__ float cider_refs(const CiderTables& t,
                                            const uint64_t (*s_key)[RW_MAXT],
                                            const float (*s_val)[RW_MAXT], int W,
                                            const float* norm_h, int r0, int r1, int ex, int part,
                                            int nparts, int lane) {
  const float len_h = (float)max(W - 1, 0);
  float total = 0.f;
  for (int r = r0 + part; r < r1; r += nparts) {
    if (r == ex) continue;  // (wave-uniform)
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    const int g0 = t.ref_ng_off[r], g1 = t.ref_ng_off[r + 1];
    for (int g = g0 + lane; g < g1; g += 64) {
      const uint64_t key = (uint64_t)t.ng_key[g];
      const float vr = t.ng_val[g];
      const int n = ngram_order(key) - 1;
      const int cnt = W - n;
      float c = 0.f;
      for (int j = 0; j < cnt; ++j) {
        if (s_key[n][j] == key) c += (CLIPPED ? fminf(s_val[n][j], vr) : s_val[n][j]) * vr;
      }
      acc0 += n == 0 ? c : 0.f;
      acc1 += n == 1 ? c : 0.f;
      acc2 += n == 2 ? c : 0.f;
      acc3 += n == 3 ? c : 0.f;
    }
    const float acc[4] = {wave_sum(acc0), wave_sum(acc1), wave_sum(acc2), wave_sum(acc3)};
    float pen = 1.f;
    if (CLIPPED) {
      const float delta = len_h - (float)t.ref_len[r];
      pen = __expf(-(delta * delta) / 72.f);
    }
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float nr = t.ref_norm[r * 4 + n];
      float val = acc[n];
      if (norm_h[n] != 0.f && nr != 0.f) val /= (norm_h[n] * nr);
      s += val * pen;
    }
    total += s;
  }
  return total;
}

// score = 10 * (the four partial sums) / (4 * references used)
__device__ __forceinline__ float cider_final(const float* s_part, int nref) {
  const float t4 = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
  return nref > 0 ? 10.f * t4 / (4.f * (float)nref) : 0.f;
}

// ---- BLEU-4 -------------------------------------------------------------------
struct BleuTables {
  int Nv;
  const int32_t* vid_ref_off;
  const int32_t* ref_len;
  const int32_t* vid_ng_off;
  const int64_t* ng_key;
  const int32_t* ng_cnt;
  const int32_t* ng_cnt2;  // (leave-one-out only)
  const int32_t* ng_arg;   // (leave-one-out only)
};

// The closing formula of sentence BLEU-4 (eval/metrics.py::Bleu) in fp64, rounded
// once: the clipped matches per order, the hypothesis length and the closest
// reference length.  One copy for the table kernels and peer_mix_kernel, so equal
// integers give equal bits.
__device__ __forceinline__ float bleu4_close(const int* correct, int W, int rlen) {
  const double tiny = 1e-15, small = 1e-9;
  double b = 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    b *= ((double)correct[k] + tiny) / ((double)max(0, W - k) + small);
  double s = pow(b, 0.25);
  const double ratio = ((double)W + tiny) / ((double)rlen + small);
  if (ratio < 1.0) s *= exp(1.0 - 1.0 / ratio);
  return (float)s;
}

// Steps 3-5 of bleu4_kernel by one whole wave, from the hypothesis' checked keys
// and first-occurrence term frequencies in LDS.  The score, valid in lane 0.
__device__ __forceinline__ float bleu4_refs(const BleuTables& t, const uint64_t (*s_key)[RW_MAXT],
                                            const int (*s_tf)[RW_MAXT], int W, int hyp,
                                            const int64_t* __restrict__ hyp_video,
                                            const int64_t* __restrict__ exclude, int lane) {
  const int64_t v64 = hyp_video[hyp];
  const bool vok = v64 >= 0 && v64 < t.Nv;  // (a video outside the tables scores 0)
  const int v = vok ? (int)v64 : 0;
  const int r0 = t.vid_ref_off[v], r1 = vok ? t.vid_ref_off[v + 1] : r0;
  // leave-one-out: the in-video index of the reference left out, -1 for none
  // (wave-uniform; only then are ng_cnt2 / ng_arg read)
  const int ex = excluded_ref(exclude, hyp, r0, r1);
  const int e = ex >= 0 ? ex - r0 : -1;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  const int g0 = t.vid_ng_off[v], g1 = vok ? t.vid_ng_off[v + 1] : g0;
  for (int g = g0 + lane; g < g1; g += 64) {
    const uint64_t key = (uint64_t)t.ng_key[g];
    int clip = t.ng_cnt[g];
    if (e >= 0 && t.ng_arg[g] == e) clip = t.ng_cnt2[g];  // (0: adds nothing)
    const int n = ngram_order(key) - 1;
    const int cnt = W - n;
    int c = 0;
    for (int j = 0; j < cnt; ++j) {
      if (s_key[n][j] == key) c += min(s_tf[n][j], clip);
    }
    c0 += n == 0 ? c : 0;
    c1 += n == 1 ? c : 0;
    c2 += n == 2 ? c : 0;
    c3 += n == 3 ? c : 0;
  }
  const int correct[4] = {wave_sum_i(c0), wave_sum_i(c1), wave_sum_i(c2), wave_sum_i(c3)};
  int best = 0x7fffffff;
  for (int r = r0 + lane; r < r1; r += 64) {
    const int lr = t.ref_len[r];
    if (r != ex) best = min(best, (abs(lr - W) << 8) | lr);
  }
  best = wave_min_i(best);
  float res = 0.f;
  if (lane == 0 && r1 > r0) res = bleu4_close(correct, W, best & 0xff);
  return res;
}

// ---- ROUGE-L ------------------------------------------------------------------
struct RougeTables {
  int Nv;
  const int32_t* vid_ref_off;
  const int32_t* ref_tok_off;
  const int32_t* ref_tok;
};

// One reference of `n` tokens (lane a < n holds token a in rtok, other lanes a
// value no hypothesis token has) against the hypothesis (htok = token `lane`,
// -1 past its end): the LCS length by the bit-parallel recurrence on one 64-bit
// word, wave-uniform.
__device__ __forceinline__ int lcs_bits(int htok, int rtok, int n) {
  uint64_t V = ~0ull;
  for (int a = 0; a < n; ++a) {
    const int c = __builtin_amdgcn_readlane(rtok, a);
    const uint64_t M = __ballot(htok == c);
    const uint64_t U = V & M;
    V = (V + U) | (V - U);
  }
  return __popcll(~V);
}

// The closing formula of ROUGE-L (eval/metrics.py::Rouge, beta 1.2) in fp64,
// rounded once: best_l / W the largest LCS precision, rec_l / rec_n the largest
// LCS recall.  One copy for the table kernels and peer_mix_kernel.
__device__ __forceinline__ float rouge_l_close(int best_l, int W, int rec_l, int rec_n) {
  float res = 0.f;
  if (W > 0 && best_l > 0 && rec_l > 0) {
    const double beta = 1.2, b2 = beta * beta;
    const double p = (double)best_l / (double)W;
    const double rc = (double)rec_l / (double)rec_n;
    res = (float)(((1.0 + b2) * p * rc) / (rc + b2 * p));
  }
  return res;
}

// rouge_l_kernel after the compaction, by one whole wave: htok = hypothesis
// token `lane` (-1 past the end).  The score, valid in lane 0.
__device__ __forceinline__ float rouge_l_refs(const RougeTables& t, int htok, int W, int hyp,
                                              const int64_t* __restrict__ hyp_video,
                                              const int64_t* __restrict__ exclude, int lane) {
  const int64_t v64 = hyp_video[hyp];
  const bool vok = v64 >= 0 && v64 < t.Nv;  // (a video outside the tables scores 0)
  const int v = vok ? (int)v64 : 0;
  const int r0 = t.vid_ref_off[v], r1 = vok ? t.vid_ref_off[v + 1] : r0;
  int best_l = 0;             // max lcs (precision: the denominator len_h is shared)
  int rec_l = 0, rec_n = 1;   // max lcs / len_r as a fraction
  // leave-one-out: the loop walks the references other than `ex` (-1: all of
  // them); `r` is the reference being processed, `rn` the one after it, both
  // stepped over `ex`, so the prefetch never loads the excluded row
  const int ex = excluded_ref(exclude, hyp, r0, r1);
  int o0 = 0, o1 = 0, nxt = -2;
  int r = r0 == ex ? r0 + 1 : r0;
  if (r < r1) {
    o0 = t.ref_tok_off[r];
    o1 = t.ref_tok_off[r + 1];
    nxt = lane < min(o1 - o0, 64) ? t.ref_tok[o0 + lane] : -2;
  }
  while (r < r1) {
    const int n = min(o1 - o0, 64);
    const int rtok = nxt;
    const int rn = r + 1 == ex ? r + 2 : r + 1;
    if (rn < r1) {  // prefetch the next reference
      o0 = t.ref_tok_off[rn];
      o1 = t.ref_tok_off[rn + 1];
      nxt = lane < min(o1 - o0, 64) ? t.ref_tok[o0 + lane] : -2;
    }
    r = rn;
    const int l = lcs_bits(htok, rtok, n);
    best_l = max(best_l, l);
    if (n > 0 && l * rec_n > rec_l * n) rec_l = l, rec_n = n;
  }
  float res = 0.f;
  if (lane == 0) res = rouge_l_close(best_l, W, rec_l, rec_n);
  return res;
}

}  // namespace cst
