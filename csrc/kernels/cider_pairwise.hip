// Peer CIDEr-D (consensus / MBR decoding): every caption of a pool scored against
// the other captions of the same pool, on the GPU.
//
// hyps (N = B * G, T): rows [k * G, (k + 1) * G) are the pool of video k.  out[i]
// is 10 x the mean over the G - 1 other rows j of i's pool of the CIDEr-D
// similarity with i as the hypothesis and j as the reference -- what
// cider_d_kernel (cider_d.hip) gives when the pool rows are the video's reference
// table and row i leaves itself out.  No reference table exists here: the
// "references" are built in LDS by the same workgroup that scores against them.
//
// One 1024-thread workgroup (16 waves) per pool, or a few per pool when the batch
// has fewer pools than the chip has CUs (each builds all vectors and scores its
// share of the rows).  The kernel is latency-bound (short dependent LDS and HBM
// reads), so it runs four waves per SIMD and spreads the four n-gram orders of a
// row over the lanes instead of walking them one after the other:
//   A. the waves build the vectors of rows w, w + 16, ... in LDS, as steps 1-3 of
//      cider_body<true>: compact_hypothesis, packed n-gram keys (n <= 4), tf
//      counted at the first occurrence (later duplicates hold 0), idf from the df
//      hash table in HBM (once per row per workgroup, not once per pair),
//      per-order L2 norms,
//      length max(W - 1, 0).  A lane owns entry x of the row's 4W - 6 n-grams,
//      all orders in one pass for W <= 17;
//   B. wave w takes hypotheses i = w, w + 16, ...; for every peer j, lanes stride
//      over j's entries of all orders and search i's entries of the same order in
//      LDS: min(v_i, v_j) * v_j, scaled by exp(-(len_i - len_j)^2 / 72) /
//      (norm_i * norm_j).  A later duplicate of j holds 0 and contributes exactly
//      0, so only unique n-grams of j count, as in a reference table.  Each lane
//      adds its scaled terms in the fixed order (j, entry); one wave_sum per
//      hypothesis.
// Deterministic: fixed-order reductions, no atomics; the result of a row does not
// depend on how many workgroups share its pool.
//
// LDS per pool row (P = T + 1 slots per order): keys 4 * P * 8 B, values
// 4 * P * 4 B, then {norm[4], len, W, pad} = 32 B.  peer_cider_supported()
// bounds G and G * P so that a pool fits one CU's LDS beside the static scratch:
// at most 64 rows of 31 tokens or 32 rows of 63 (98 KB).
#include <algorithm>

#include "../common.h"
#include "../cider_common.h"
#include "peer_common.h"

namespace cst {

constexpr int PEER_MAX_LDS = 48 * PEER_MAX_SLOTS + PEER_HDR_BYTES * PEER_MAXG;  // 100,352 B

static inline int peer_row_bytes(int T) { return 48 * (T + 1) + PEER_HDR_BYTES; }

bool peer_cider_supported(int64_t G, int64_t T) {
  return G >= 2 && G <= PEER_MAXG && T >= 1 && T <= PEER_MAXT && G * (T + 1) <= PEER_MAX_SLOTS;
}

__global__ __launch_bounds__(PEER_WAVES * 64) void cider_pairwise_kernel(
    const int64_t* __restrict__ hyps, int T, int G, const int64_t* __restrict__ ht_keys,
    const float* __restrict__ ht_vals, uint32_t ht_cap, float log_ref_len, int use_eos,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_pool[];
  __shared__ int s_tok[PEER_WAVES][64];

  const int w = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int P = T + 1;
  const int row_bytes = 48 * P + PEER_HDR_BYTES;
  const int64_t row0 = (int64_t)blockIdx.x * G;

  auto keys_of = [&](int r) { return reinterpret_cast<uint64_t*>(s_pool + (size_t)r * row_bytes); };
  auto vals_of = [&](int r) {
    return reinterpret_cast<float*>(s_pool + (size_t)r * row_bytes + 32 * P);
  };
  auto hdr_of = [&](int r) {
    return reinterpret_cast<float*>(s_pool + (size_t)r * row_bytes + 48 * P);
  };

  // -- A. vectors of the pool rows (all waves run every round: block barriers) -----
  for (int base = 0; base < G; base += PEER_WAVES) {
    const int r = base + w;
    const bool live = r < G;  // (wave-uniform)
    int W = 0;
    if (live) W = compact_hypothesis(hyps + (row0 + r) * T, T, lane, use_eos, s_tok[w]);
    __syncthreads();
    const PeerSpan sp(W);
    if (live) {
      uint64_t* k = keys_of(r);
      for (int x = lane; x < sp.E; x += 64) {
        int pos;
        const int n = sp.order(x, pos);
        uint64_t key = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i <= n) key |= (uint64_t)(s_tok[w][pos + i] + 1) << (16 * i);
        k[n * P + pos] = key;
      }
    }
    __syncthreads();
    if (live) {
      const uint64_t* k = keys_of(r);
      float* v = vals_of(r);
      float* h = hdr_of(r);
      float sq0 = 0.f, sq1 = 0.f, sq2 = 0.f, sq3 = 0.f;
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
        float val = 0.f;
        if (first) {
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
      sq0 = wave_sum(sq0), sq1 = wave_sum(sq1), sq2 = wave_sum(sq2), sq3 = wave_sum(sq3);
      if (lane == 0) {
        h[0] = sqrtf(sq0), h[1] = sqrtf(sq1), h[2] = sqrtf(sq2), h[3] = sqrtf(sq3);
        h[4] = (float)max(W - 1, 0);
        reinterpret_cast<int*>(h)[5] = W;
      }
    }
  }
  __syncthreads();

  // -- B. every hypothesis against its peers ---------------------------------------
  for (int i = blockIdx.y * PEER_WAVES + w; i < G; i += PEER_WAVES * gridDim.y) {
    const uint64_t* ki = keys_of(i);
    const float* vi = vals_of(i);
    const float* hi = hdr_of(i);
    const float ni0 = hi[0], ni1 = hi[1], ni2 = hi[2], ni3 = hi[3];
    const float len_i = hi[4];
    const int Wi = reinterpret_cast<const int*>(hi)[5];
    float total = 0.f;
    for (int j = 0; j < G; ++j) {
      if (j == i) continue;  // (wave-uniform)
      const uint64_t* kj = keys_of(j);
      const float* vj = vals_of(j);
      const float* hj = hdr_of(j);
      const PeerSpan sp(reinterpret_cast<const int*>(hj)[5]);
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
    if (lane == 0) out[row0 + i] = 10.f * total / (4.f * (float)(G - 1));
  }
}

// The caller checks peer_cider_supported(G, T) first (train_ops.cpp cider_score).
void launch_cider_pairwise(const int64_t* hyps, int T, int G, int B, const int64_t* ht_keys,
                           const float* ht_vals, uint32_t ht_cap, float log_ref_len,
                           int use_eos, float* out, hipStream_t stream) {
  if (B <= 0) return;
  if (!peer_cider_supported(G, T))
    throw std::runtime_error("cider_pairwise: pool outside the supported (G, T)");
  const int lds = G * peer_row_bytes(T);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)cider_pairwise_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, PEER_MAX_LDS);
    attr = true;
  }
  // few pools: up to 4 workgroups share one (each with rows to score), towards
  // one workgroup per CU
  const int rounds = (G + PEER_WAVES - 1) / PEER_WAVES;
  const int split = std::max(1, std::min({4, rounds, 256 / B}));
  hipLaunchKernelGGL(cider_pairwise_kernel, dim3(B, split), dim3(PEER_WAVES * 64), lds, stream,
                     hyps, T, G, ht_keys, ht_vals, ht_cap, log_ref_len, use_eos, out);
  post_launch("cider_pairwise_kernel", stream);
}

}  // namespace cst
