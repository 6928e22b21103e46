// Peer scores under a mixed utility (consensus / MBR decoding, --mbr_mix): every
// caption of a pool scored against the other captions of the same pool under
// w_c * CIDEr-D + w_b * BLEU-4 + w_r * ROUGE-L, in ONE launch.
//
// hyps (N = B * G, T): rows [k * G, (k + 1) * G) are the pool of video k; the
// references of row i are the G - 1 other rows of its pool.  parts[i] = (peer
// CIDEr-D as cider_pairwise_kernel defines it, sentence BLEU-4, ROUGE-L of
// eval/metrics.py against those references) -- what cider_d_kernel, bleu4_kernel
// and rouge_l_kernel give when the pool rows are the video's reference table and
// row i leaves itself out.  No reference table exists here: the references are
// built in LDS by the workgroup that scores against them.
//
// One 1024-thread workgroup (16 waves) per pool, or a few per pool when the batch
// has few pools (each builds all rows and scores its share), as
// cider_pairwise_kernel:
//   A. wave w builds rows w, w + 16, ... in LDS: the compacted tokens, the packed
//      keys of orders 1-4 with BLEU's rule (an n-gram with a token the 16-bit
//      packing cannot hold gets key 0 and matches nothing), the integer term
//      frequency at the first occurrence (0 at a later duplicate), the tf-idf
//      value, the per-order norms and the length of CIDEr-D (df probes only when
//      w_c > 0), W;
//   B. the (row, metric in use) pairs of the workgroup's rows are dealt to the
//      waves, one wave per pair:
//        CIDEr-D: as phase B of cider_pairwise_kernel;
//        BLEU-4:  a lane owns entry x of row i's n-grams; for a first occurrence
//                 it walks the peers and keeps the largest tf of that key in the
//                 peer's segment of the same order (the clip count); sum of
//                 min(tf, clip) per order by a wave reduction, closest peer
//                 length (ties to the shorter) by a wave min, bleu4_close;
//        ROUGE-L: lcs_bits of row i against every peer (the peer's tokens read
//                 once from LDS, then wave-uniform), largest LCS precision and
//                 recall, rouge_l_close;
//   C. one thread per row blends in fp32, each product and sum rounded once:
//      out = ((w_c * c) + (w_b * b)) + (w_r * r), as reward_mix_kernel.
// A metric of weight 0 is skipped wave-uniformly and its column is exactly 0.
// Deterministic: fixed-order reductions, no atomics; a (row, metric) pair is the
// work of one wave whatever the number of workgroups per pool.
//
// LDS per pool row (P = T + 1 slots per order): keys 4 * P * 8 B, tf-idf values
// and integer tf 4 * P * 4 B each, tokens P * 4 B (P rounded up to even, so rows
// stay 8-byte aligned), then {norm[4], len, W, pad} = 32 B: 68 * P + 32 B, at
// most 141,568 B within peer_cider_supported() -- one workgroup per CU.
#include <algorithm>

#include "../common.h"
#include "../cider_common.h"
#include "../launchers.h"
#include "peer_common.h"
#include "reward_bodies.h"

namespace cst {

static inline int peer_mix_row_bytes(int T) {
  const int P = T + 1;
  return 64 * P + 4 * ((P + 1) & ~1) + PEER_HDR_BYTES;
}
// G * P <= PEER_MAX_SLOTS; the token padding adds at most 4 B per row
constexpr int PEER_MIX_MAX_LDS = 68 * PEER_MAX_SLOTS + (4 + PEER_HDR_BYTES) * PEER_MAXG;

__global__ __launch_bounds__(PEER_WAVES * 64) void peer_mix_kernel(
    const int64_t* __restrict__ hyps, int T, int G, const int64_t* __restrict__ ht_keys,
    const float* __restrict__ ht_vals, uint32_t ht_cap, float log_ref_len, int use_eos,
    float w_c, float w_b, float w_r, float* __restrict__ out, float* __restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_pool[];
  __shared__ float s_res[PEER_MAXG * 3];

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int P = T + 1;
  const int row_bytes = 64 * P + 4 * ((P + 1) & ~1) + PEER_HDR_BYTES;
  const int64_t row0 = (int64_t)blockIdx.x * G;
  const bool has_c = w_c != 0.f, has_b = w_b != 0.f, has_r = w_r != 0.f;
  const bool has_keys = has_c || has_b;

  auto keys_of = [&](int r) { return reinterpret_cast<uint64_t*>(s_pool + (size_t)r * row_bytes); };
  auto vals_of = [&](int r) {
    return reinterpret_cast<float*>(s_pool + (size_t)r * row_bytes + 32 * P);
  };
  auto tf_of = [&](int r) {
    return reinterpret_cast<int*>(s_pool + (size_t)r * row_bytes + 48 * P);
  };
  auto tok_of = [&](int r) {
    return reinterpret_cast<int*>(s_pool + (size_t)r * row_bytes + 64 * P);
  };
  auto hdr_of = [&](int r) {
    return reinterpret_cast<float*>(s_pool + (size_t)r * row_bytes + row_bytes - PEER_HDR_BYTES);
  };
  auto len_of = [&](int r) { return reinterpret_cast<const int*>(hdr_of(r))[5]; };

  // -- A. the pool rows (all waves run every round: block barriers) -----------------
  for (int base = 0; base < G; base += PEER_WAVES) {
    const int r = base + w;
    const bool live = r < G;  // (wave-uniform)
    int W = 0;
    if (live) W = compact_hypothesis(hyps + (row0 + r) * T, T, lane, use_eos, tok_of(r));
    __syncthreads();
    const PeerSpan sp(W);
    if (live && has_keys) {
      uint64_t* k = keys_of(r);
      const int* tk = tok_of(r);
      for (int x = lane; x < sp.E; x += 64) {
        int pos;
        const int n = sp.order(x, pos);
        uint64_t key = 0;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i <= n) {
            const int t = tk[pos + i];
            ok = ok && t >= 0 && t < 65535;
            key |= (uint64_t)((t + 1) & 0xffff) << (16 * i);
          }
        k[n * P + pos] = ok ? key : 0;
      }
    }
    __syncthreads();
    if (live) {
      float sq0 = 0.f, sq1 = 0.f, sq2 = 0.f, sq3 = 0.f;
      if (has_keys) {
        const uint64_t* k = keys_of(r);
        float* v = vals_of(r);
        int* f = tf_of(r);
        for (int x = lane; x < sp.E; x += 64) {
          int pos;
          const int n = sp.order(x, pos);
          const uint64_t* seg = k + n * P;
          const int cnt = W - n;
          const uint64_t key = seg[pos];
          int tf = 0;
          bool first = true;
          for (int j = 0; j < cnt; ++j) {
            const bool eq = seg[j] == key;
            tf += eq;
            first = first && !(eq && j < pos);
          }
          if (!first || key == 0) tf = 0;  // (key 0: an n-gram the packing cannot hold)
          f[n * P + pos] = tf;
          if (has_c) {
            float val = 0.f;
            if (tf > 0) {
              const float df = df_lookup(ht_keys, ht_vals, ht_cap, key);
              val = (float)tf * (log_ref_len - __logf(fmaxf(1.f, df)));
            }
            v[n * P + pos] = val;
            const float sq = val * val;
            sq0 += n == 0 ? sq : 0.f;
            sq1 += n == 1 ? sq : 0.f;
            sq2 += n == 2 ? sq : 0.f;
            sq3 += n == 3 ? sq : 0.f;
          }
        }
        if (has_c)
          sq0 = wave_sum(sq0), sq1 = wave_sum(sq1), sq2 = wave_sum(sq2), sq3 = wave_sum(sq3);
      }
      if (lane == 0) {
        float* h = hdr_of(r);
        h[0] = sqrtf(sq0), h[1] = sqrtf(sq1), h[2] = sqrtf(sq2), h[3] = sqrtf(sq3);
        h[4] = (float)max(W - 1, 0);
        reinterpret_cast<int*>(h)[5] = W;
      }
    }
  }
  __syncthreads();

  // -- B. (row, metric) pairs of this workgroup's rows y, y + ny, ... ----------------
  const int nm = (int)has_c + (int)has_b + (int)has_r;
  const int ny = gridDim.y, y = blockIdx.y;
  const int nrows = y < G ? (G - y + ny - 1) / ny : 0;
  for (int t = w; t < nrows * nm; t += PEER_WAVES) {
    const int kk = t / nm, m = t - kk * nm;
    const int i = y + kk * ny;
    // the m-th metric in use: 0 CIDEr-D, 1 BLEU-4, 2 ROUGE-L (wave-uniform)
    int metric = 2;
    if (has_c && m == 0)
      metric = 0;
    else if (has_b && m == (int)has_c)
      metric = 1;
    const int Wi = __builtin_amdgcn_readfirstlane(len_of(i));
    float res = 0.f;  // (valid in lane 0)
    if (metric == 0) {
      const uint64_t* ki = keys_of(i);
      const float* vi = vals_of(i);
      const float* hi = hdr_of(i);
      const float ni0 = hi[0], ni1 = hi[1], ni2 = hi[2], ni3 = hi[3];
      const float len_i = hi[4];
      float total = 0.f;
      for (int j = 0; j < G; ++j) {
        if (j == i) continue;  // (wave-uniform)
        const uint64_t* kj = keys_of(j);
        const float* vj = vals_of(j);
        const float* hj = hdr_of(j);
        const PeerSpan sp(len_of(j));
        const float delta = len_i - hj[4];
        const float pen = __expf(-(delta * delta) / 72.f);
        const float nj0 = hj[0], nj1 = hj[1], nj2 = hj[2], nj3 = hj[3];
        const float s0 = (ni0 != 0.f && nj0 != 0.f) ? pen / (ni0 * nj0) : pen;
        const float s1 = (ni1 != 0.f && nj1 != 0.f) ? pen / (ni1 * nj1) : pen;
        const float s2 = (ni2 != 0.f && nj2 != 0.f) ? pen / (ni2 * nj2) : pen;
        const float s3 = (ni3 != 0.f && nj3 != 0.f) ? pen / (ni3 * nj3) : pen;
        for (int x = lane; x < sp.E; x += 64) {
          int pos;
          const int n = sp.order(x, pos);
          const float vr = vj[n * P + pos];
          if (vr != 0.f) {  // (0: a later duplicate, or idf 0 -- contributes 0)
            const uint64_t key = kj[n * P + pos];
            const uint64_t* seg = ki + n * P;
            const float* vseg = vi + n * P;
            const int cnt = Wi - n;
            float c = 0.f;
#pragma unroll 4
            for (int e = 0; e < cnt; ++e) {
              if (seg[e] == key) c += fminf(vseg[e], vr) * vr;
            }
            total += c * (n == 0 ? s0 : n == 1 ? s1 : n == 2 ? s2 : s3);
          }
        }
      }
      total = wave_sum(total);
      res = 10.f * total / (4.f * (float)(G - 1));
    } else if (metric == 1) {
      const uint64_t* ki = keys_of(i);
      const int* fi = tf_of(i);
      const PeerSpan sp(Wi);
      int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      for (int x = lane; x < sp.E; x += 64) {
        int pos;
        const int n = sp.order(x, pos);
        const int tfi = fi[n * P + pos];
        if (tfi > 0) {  // (a first occurrence of a key the packing holds)
          const uint64_t key = ki[n * P + pos];
          int clip = 0;  // the largest count of the key among the peers
          for (int j = 0; j < G && clip < tfi; ++j) {
            if (j == i) continue;
            const uint64_t* seg = keys_of(j) + n * P;
            const int* fseg = tf_of(j) + n * P;
            const int cnt = len_of(j) - n;
#pragma unroll 4
            for (int e = 0; e < cnt; ++e) {
              if (seg[e] == key) clip = max(clip, fseg[e]);
            }
          }
          const int c = min(tfi, clip);
          c0 += n == 0 ? c : 0;
          c1 += n == 1 ? c : 0;
          c2 += n == 2 ? c : 0;
          c3 += n == 3 ? c : 0;
        }
      }
      const int correct[4] = {wave_sum_i(c0), wave_sum_i(c1), wave_sum_i(c2), wave_sum_i(c3)};
      int best = 0x7fffffff;
      for (int j = lane; j < G; j += 64) {
        const int lr = len_of(j);
        if (j != i) best = min(best, (abs(lr - Wi) << 8) | lr);
      }
      best = wave_min_i(best);
      if (lane == 0) res = bleu4_close(correct, Wi, best & 0xff);
    } else {
      const int htok = lane < Wi ? tok_of(i)[lane] : -1;
      int best_l = 0;             // max lcs (precision: the denominator len_i is shared)
      int rec_l = 0, rec_n = 1;   // max lcs / len_j as a fraction
      for (int j = 0; j < G; ++j) {
        if (j == i) continue;  // (wave-uniform)
        const int n = __builtin_amdgcn_readfirstlane(len_of(j));
        const int rtok = lane < n ? tok_of(j)[lane] : -2;
        const int l = lcs_bits(htok, rtok, n);
        best_l = max(best_l, l);
        if (n > 0 && l * rec_n > rec_l * n) rec_l = l, rec_n = n;
      }
      if (lane == 0) res = rouge_l_close(best_l, Wi, rec_l, rec_n);
    }
    if (lane == 0) s_res[i * 3 + metric] = res;
  }
  __syncthreads();

  // -- C. blend ---------------------------------------------------------------------
  if ((int)threadIdx.x < nrows) {
    const int i = y + (int)threadIdx.x * ny;
    const float c = has_c ? s_res[i * 3 + 0] : 0.f;
    const float b = has_b ? s_res[i * 3 + 1] : 0.f;
    const float r = has_r ? s_res[i * 3 + 2] : 0.f;
    float* p = parts + (row0 + i) * 3;
    p[0] = c, p[1] = b, p[2] = r;
    out[row0 + i] = __fadd_rn(__fadd_rn(__fmul_rn(w_c, c), __fmul_rn(w_b, b)), __fmul_rn(w_r, r));
  }
}

// The caller checks peer_cider_supported(G, T) and the weights first
// (train_ops.cpp peer_mix_score).
void launch_peer_mix(const int64_t* hyps, int T, int G, int B, const int64_t* ht_keys,
                     const float* ht_vals, uint32_t ht_cap, float log_ref_len, int use_eos,
                     float w_c, float w_b, float w_r, float* out, float* parts,
                     hipStream_t stream) {
  if (B <= 0) return;
  if (!peer_cider_supported(G, T))
    throw std::runtime_error("peer_mix: pool outside the supported (G, T)");
  const int nm = (w_c != 0.f) + (w_b != 0.f) + (w_r != 0.f);
  if (nm == 0 || (w_c != 0.f && (!ht_keys || !ht_vals || ht_cap == 0)))
    throw std::runtime_error("peer_mix: no metric in use, or CIDEr-D without a df table");
  const int lds = G * peer_mix_row_bytes(T);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)peer_mix_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, PEER_MIX_MAX_LDS);
    attr = true;
  }
  // few pools: up to 4 workgroups share one (each with pairs to score), towards
  // one workgroup per CU
  const int rounds = (G * nm + PEER_WAVES - 1) / PEER_WAVES;
  const int split = std::max(1, std::min({4, rounds, 256 / B}));
  hipLaunchKernelGGL(peer_mix_kernel, dim3(B, split), dim3(PEER_WAVES * 64), lds, stream, hyps, T,
                     G, ht_keys, ht_vals, ht_cap, log_ref_len, use_eos, w_c, w_b, w_r, out, parts);
  post_launch("peer_mix_kernel", stream);
}

}  // namespace cst
