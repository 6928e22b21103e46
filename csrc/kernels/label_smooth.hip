// K7, label smoothing (--label_smoothing eps): the uniform part of the
// smoothed XE target on the exp-store vocab head, without a dense pass.
//
// The smoothed log-prob of row (t, r) with target y is
//     g = (1 - eps) lp[y] + eps mean_v lp[v],
//     mean_v lp[v] = Hd . wbar + bbar - lse
// (wbar = the column mean of the logit weights, bbar = the mean bias, Hd the
// saved vocab input), and with the incoming gradient dg of g the vocab head's
// dS (vocab_grad.hip) becomes
//     dS_rv = (1 - eps) dg [v = y] + eps dg / V - dg p_rv.
// row_weights (vocab_grad.hip) scales the one-hot weight by 1 - eps and keeps
// alpha = -(a + dg) s; the uniform term is rank-1 wherever it appears:
//     dHd_r += eps dg_r wbar       (ls_shift: X_r += (eps dg_r / alpha_r) wbar,
//                                   the reverse loop forms alpha_r X_r + ...)
//     dW_v  += (1 / V) sum_r eps dg_r Hd_r     (ls_rowsum + ls_add)
//     db_v  += (1 / V) sum_r eps dg_r
// Every sum is two-stage in a fixed order (per-row-block partials, then one
// reduce): no float atomics, runs are bit-equal.  None of these kernels is
// launched with eps = 0.
#include "../common.h"
#include "../launchers.h"

namespace cst {

constexpr int LS_THREADS = 256, LS_UNROLL = 4, LS_MAXH = 2048;

// Weighted column sums of bf16 rows (n, H), stage 1: block b owns rows
// [b rb, b rb + rb); thread (g, c) keeps the 8 sums of chunk c over the rows
// g, g + G, ... (G = 256 / (H / 8) row groups, LS_UNROLL row loads in flight),
// the groups are summed through LDS in group order.  part (blocks, ldp): the
// H column sums, then at [H] the sum of the rows' extra term.
//   w.dg == nullptr: weight 1, extra bias[row]   (column mean of W, mean bias)
//   else: weight = extra = eps dg[r, t] of row t R + r   (the rank-1 sums)
__global__ __launch_bounds__(LS_THREADS) void ls_rowsum_part_kernel(
    const uint16_t* __restrict__ rows, int64_t n, int H, LsRowW w, int rb,
    float* __restrict__ part, int ldp) {
  __shared__ float s_acc[LS_THREADS * 8 + LS_THREADS];
  const int nch = H / 8, G = LS_THREADS / nch;
  const int c = threadIdx.x % nch, g = threadIdx.x / nch;
  float acc[8], ex = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * rb, r1 = min(r0 + rb, n);
  if (g < G) {
    for (int64_t rr = r0 + g; rr < r1; rr += (int64_t)LS_UNROLL * G) {
      uint4 x[LS_UNROLL];
      float wt[LS_UNROLL], e[LS_UNROLL];
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) {
        const int64_t r = rr + (int64_t)u * G;
        const bool in = r < r1;
        const int64_t rc = in ? r : r1 - 1;  // (a row of the block: loaded, weight 0)
        if (w.dg != nullptr) {
          wt[u] = in ? w.eps * w.dg[(rc % w.R) * w.rs + rc / w.R] : 0.f;
          e[u] = wt[u];
        } else {
          wt[u] = in ? 1.f : 0.f;
          e[u] = in ? w.bias[rc] : 0.f;
        }
        x[u] = *reinterpret_cast<const uint4*>(rows + rc * H + 8 * c);
      }
#pragma unroll
      for (int u = 0; u < LS_UNROLL; ++u) {
        const uint32_t q[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[2 * k] = fmaf(wt[u], bf2f(q[k] & 0xffff), acc[2 * k]);
          acc[2 * k + 1] = fmaf(wt[u], bf2f(q[k] >> 16), acc[2 * k + 1]);
        }
        ex += e[u];
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_acc[g * H + 8 * c + k] = acc[k];
    if (c == 0) s_acc[LS_THREADS * 8 + g] = ex;
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * ldp;
  for (int h = threadIdx.x; h < H; h += LS_THREADS) {
    float s = 0.f;
    for (int k = 0; k < G; ++k) s += s_acc[k * H + h];
    out[h] = s;
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < G; ++k) s += s_acc[LS_THREADS * 8 + k];
    out[H] = s;
  }
}

// stage 2: out[h] = scale sum_b part[b, h], h < n (the H columns and the extra
// term).  64 columns per block, 4 groups of 64 threads splitting the partial
// rows (8 loads in flight each), summed through LDS (as vgrad_colsum_reduce)
__global__ __launch_bounds__(256) void ls_rowsum_reduce_kernel(const float* __restrict__ part,
                                                               int nb, int ldp, int n, float scale,
                                                               float* __restrict__ out) {
  __shared__ float s_p[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int v = blockIdx.x * 64 + c;
  float s = 0.f;
  if (v < n) {
    int b = g;
    for (; b + 28 < nb; b += 32) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = part[(int64_t)(b + 4 * u) * ldp + v];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += x[u];
    }
    for (; b < nb; b += 4) s += part[(int64_t)b * ldp + v];
  }
  s_p[g][c] = s;
  __syncthreads();
  if (g == 0 && v < n) out[v] = (s_p[0][c] + s_p[1][c] + s_p[2][c] + s_p[3][c]) * scale;
}

int ls_rowsum_blocks(int64_t n, int rb) { return (int)((n + rb - 1) / rb); }

void launch_ls_rowsum(const uint16_t* rows, int64_t n, int H, const LsRowW& w, int rb, float scale,
                      float* part, float* out, hipStream_t stream) {
  if (H % 8 != 0 || H < 8 || H > LS_MAXH)
    throw std::runtime_error("label smoothing: H must be a multiple of 8 and <= 2048");
  if (n <= 0 || rb <= 0) throw std::runtime_error("label smoothing: empty row sum");
  const int nb = ls_rowsum_blocks(n, rb), ldp = H + 8;
  hipLaunchKernelGGL(ls_rowsum_part_kernel, dim3(nb), dim3(LS_THREADS), 0, stream, rows, n, H, w,
                     rb, part, ldp);
  post_launch("ls_rowsum_part_kernel", stream);
  hipLaunchKernelGGL(ls_rowsum_reduce_kernel, dim3((H + 1 + 63) / 64), dim3(256), 0, stream, part,
                     nb, ldp, H + 1, scale, out);
  post_launch("ls_rowsum_reduce_kernel", stream);
}

// One wavefront per row (t, r): mean_v lp[v] = Hd . wbar + bbar - lse (fp32 dot
// of the bf16 row, 8-column chunks per lane), blended into the target
// log-prob the combine wrote: g = (1 - eps) g + eps mean_v lp[v]
__global__ __launch_bounds__(LS_THREADS) void ls_blend_kernel(
    const uint16_t* __restrict__ hd, const float* __restrict__ wbar, const float* __restrict__ lse,
    int64_t NR, int R, int H, float eps, float* __restrict__ g_xe, int64_t g_rs) {
  const int64_t row = (int64_t)blockIdx.x * (LS_THREADS / WAVE) + (threadIdx.x >> 6);
  if (row >= NR) return;
  const int lane = threadIdx.x & 63;
  float d = 0.f;
  for (int c = lane; 8 * c < H; c += WAVE) {
    const uint4 h = *reinterpret_cast<const uint4*>(hd + row * H + 8 * c);
    const float4 w0 = *reinterpret_cast<const float4*>(wbar + 8 * c);
    const float4 w1 = *reinterpret_cast<const float4*>(wbar + 8 * c + 4);
    d = fmaf(bf2f(h.x & 0xffff), w0.x, d), d = fmaf(bf2f(h.x >> 16), w0.y, d);
    d = fmaf(bf2f(h.y & 0xffff), w0.z, d), d = fmaf(bf2f(h.y >> 16), w0.w, d);
    d = fmaf(bf2f(h.z & 0xffff), w1.x, d), d = fmaf(bf2f(h.z >> 16), w1.y, d);
    d = fmaf(bf2f(h.w & 0xffff), w1.z, d), d = fmaf(bf2f(h.w >> 16), w1.w, d);
  }
  d = wave_sum(d);
  if (lane == 0) {
    float* gp = g_xe + (row % R) * g_rs + row / R;
    *gp = (1.f - eps) * *gp + eps * (d + wbar[H] - lse[row]);
  }
}

void launch_ls_blend(const uint16_t* hd, const float* wbar, const float* lse, int64_t NR, int R,
                     int H, float eps, float* g_xe, int64_t g_rs, hipStream_t stream) {
  if (H % 8 != 0) throw std::runtime_error("label smoothing: H must be a multiple of 8");
  const int rows = LS_THREADS / WAVE;
  hipLaunchKernelGGL(ls_blend_kernel, dim3((unsigned)((NR + rows - 1) / rows)), dim3(LS_THREADS), 0,
                     stream, hd, wbar, lse, NR, R, H, eps, g_xe, g_rs);
  post_launch("ls_blend_kernel", stream);
}

// One wavefront per row of [row0, row0 + nrows): X_r += (eps dg_r / alpha_r)
// wbar, after X and alpha are final (vgrad_onehot / vgrad_fix) and before the
// reverse loop reads alpha_r X_r.  Rows without a target gradient (masked:
// dg = 0) or without any gradient (alpha = 0) are not touched.
__global__ __launch_bounds__(LS_THREADS) void ls_shift_kernel(
    float* __restrict__ X, const float* __restrict__ alpha, const float* __restrict__ wbar,
    LsRowW w, int64_t row0, int64_t nrows, int H) {
  const int64_t i = (int64_t)blockIdx.x * (LS_THREADS / WAVE) + (threadIdx.x >> 6);
  if (i >= nrows) return;
  const int64_t row = row0 + i;
  const float u = w.eps * w.dg[(row % w.R) * w.rs + row / w.R], al = alpha[row];
  if (u == 0.f || al == 0.f) return;
  const float k = u / al;
  const int lane = threadIdx.x & 63;
  for (int c = lane; 4 * c < H; c += WAVE) {
    float4* xp = reinterpret_cast<float4*>(X + row * H + 4 * c);
    const float4 wv = *reinterpret_cast<const float4*>(wbar + 4 * c);
    float4 x = *xp;
    x.x = fmaf(k, wv.x, x.x), x.y = fmaf(k, wv.y, x.y);
    x.z = fmaf(k, wv.z, x.z), x.w = fmaf(k, wv.w, x.w);
    *xp = x;
  }
}

void launch_ls_shift(float* X, const float* alpha, const float* wbar, const LsRowW& w,
                     int64_t row0, int64_t nrows, int H, hipStream_t stream) {
  if (H % 4 != 0) throw std::runtime_error("label smoothing: H must be a multiple of 4");
  if (nrows <= 0) return;
  const int rows = LS_THREADS / WAVE;
  hipLaunchKernelGGL(ls_shift_kernel, dim3((unsigned)((nrows + rows - 1) / rows)),
                     dim3(LS_THREADS), 0, stream, X, alpha, wbar, w, row0, nrows, H);
  post_launch("ls_shift_kernel", stream);
}

// dW (V, H) += gs[0 .. H) on every vocabulary row, db (V) += gs[H]: one float4
// per thread
__global__ __launch_bounds__(256) void ls_add_kernel(float* __restrict__ dW,
                                                     float* __restrict__ db,
                                                     const float* __restrict__ gs, int V, int H) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int h4 = H / 4;
  if (i < (int64_t)V * h4) {
    float4* p = reinterpret_cast<float4*>(dW) + i;
    const float4 s = *reinterpret_cast<const float4*>(gs + 4 * (i % h4));
    float4 x = *p;
    x.x += s.x, x.y += s.y, x.z += s.z, x.w += s.w;
    *p = x;
  }
  if (i < V) db[i] += gs[H];
}

void launch_ls_add(float* dW, float* db, const float* gs, int V, int H, hipStream_t stream) {
  if (H % 4 != 0) throw std::runtime_error("label smoothing: H must be a multiple of 4");
  const int64_t n = (int64_t)V * (H / 4);
  hipLaunchKernelGGL(ls_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dW, db,
                     gs, V, H);
  post_launch("ls_add_kernel", stream);
}

}  // namespace cst
