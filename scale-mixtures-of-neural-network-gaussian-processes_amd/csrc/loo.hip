// loo.hip — leave-one-out cross-validation of the exact GP / Student-t process (Rasmussen & Williams 5.4.2), for C target
// columns that share one kernel matrix (SPR: C = 1, MultiSPR).  Leaving out point i leaves out all C outputs of that point.
//
// With K~ = K + eps I, P = K~^-1, A = P Y [n,C], p_i = P_ii, Q = sum_ic Y_ic A_ic, e_i = sum_c A_ic^2 / p_i:
//   mean      mu_ic = Y_ic - A_ic / p_i
//   Gaussian  (df <= 0): variance 1 / p_i,   log p_i = -(C/2) log 2 pi + (C/2) log p_i - e_i / 2
//   Student-t (nu = df, s = scale; vec(Y) ~ MVT_NC(nu, 0, s (I_C x K~))): a C-variate t with nu + (N-1) C degrees of freedom,
//             shape sigma_i^2 I_C, sigma_i^2 = t_i / (nu + (N-1) C) * s / p_i, t_i = nu + (Q - e_i) / s, t_Q = nu + Q / s,
//             log p_i = lgamma(m2) - lgamma(m1) - (C/2) log pi - (C/2) log s + (C/2) log p_i + m1 log t_i - m2 log t_Q,
//             m1 = (nu + (N-1) C) / 2, m2 = (nu + N C) / 2
//   Lambda = sum_i log p_i, and its seed G (d Lambda = sum_ij G_ij dK~_ij over all i, j):
//     le_i = -1/2 | -m1 / (s t_i),   lQ = 0 | sum_i m1 / (s t_i) - N m2 / (s t_Q),   a_ic = 2 le_i A_ic / p_i,
//     d_i = C / (2 p_i) - le_i e_i / p_i,   U = P a,   W = U / 2 + lQ A / 2,
//     G = -P diag(d) P - (W A^T + A W^T)
// so the existing tangent passes (grad.hip, cnn_grad.hip), fed G in place of -K~^-1 with coef = 0 and a zero alpha, return
// d Lambda / d(w_std, b_std, last_w_std, eps).
//
// Device work of the head, in launch order (everything per point and every sum over points in fp64, per-block partials in a
// fixed tree plus a one-block second stage: no floating-point atomics, two calls give the same bits):
//   loo_diag_kernel    p_i, e_i, partial sums of Q                                   n threads
//   loo_sum_kernel     Q
//   loo_point_kernel   mean, scale2, a [n,C], d [n], partials of Lambda, lQ, d/d df, d/d scale
//   loo_sum_kernel     those four sums (and lQ's closed-form tail)
//   -- only with a seed (g_d != NULL) --
//   loo_pack_kernel    N = -P mirrored from the LOWER triangle of the input into a full, zero-padded [n_pad, n_pad] copy, and
//                      S = N diag(d) beside it (d_i has either sign under the Student-t head: no square-root trick)
//   loo_u_kernel       W = -(N a) / 2 + lQ A / 2, one wave per row, fp64 sums (N^2 C)
//   loo_pdp_kernel     -N diag(d) N = -(rows of N) x (rows of S)^T on the 128 x 128 MFMA tile engine, lower tiles only: the one
//                      N^3 launch (N^3 flops for the triangle), the flop count and tile shape of syrk_rows_kernel (cholesky.hip)
//   loo_rank_kernel    the rank-2C terms, one pass behind it: G_ij -= sum_c W_ic A_jc + A_ic W_jc, summed in fp64
// Workspace: 2 n_pad^2 elements of the storage type (the two padded operands; n_pad = n rounded up to 128) and
// (4 n + 2 n C) doubles.  g_d may be the input matrix itself (the pack has read it before the product writes): the fused
// entries keep no second n^2 matrix for the seed.
#include <climits>
#include <cmath>
#include <vector>

#include "gemm_nt.hpp"
#include "internal.hpp"

namespace {

struct LooHead {
  double df, scale;   // df <= 0: Gaussian
  int64_t n;
  int c;
};

// fixed-order sum of 256 values (the tree of diag_trace_kernel)
__device__ __forceinline__ double loo_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// (hi, lo) += a * b with the product's and the sum's rounding errors kept in lo (Dekker / Knuth): the C-term sums of a point
// come out to about one rounding of their value.  The Student-t head needs it: t_i = nu + (Q - e_i) / s is a difference of two
// such sums that cancel completely at n = 1 and largely at small n, and le_i, a, d and the seed all hang on it.
__device__ __forceinline__ void loo_dd_fma(double a, double b, double& hi, double& lo) {
#pragma clang fp contract(off)   // the error terms are exact only for the rounded product and the rounded sum themselves
  const double pr = a * b, pe = fma(a, b, -pr);
  const double sm = hi + pr, bb = sm - hi;
  lo += ((hi - (sm - bb)) + (pr - bb)) + pe;
  hi = sm;
}

template <typename T>
__global__ void __launch_bounds__(256) loo_diag_kernel(const T* __restrict__ nkinv, int64_t ldk, const T* __restrict__ alpha,
                                                       const T* __restrict__ y, int64_t n, int c, double* __restrict__ p,
                                                       double* __restrict__ e, double* __restrict__ elo,
                                                       double* __restrict__ partq) {
  __shared__ double red[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double q = 0.0, ql = 0.0;
  if (i < n) {
    const double pi = -(double)nkinv[i * ldk + i];
    double s2 = 0.0, s2l = 0.0;
    for (int k = 0; k < c; ++k) {
      const double a = (double)alpha[i * c + k];
      loo_dd_fma(a, a, s2, s2l);
      loo_dd_fma((double)y[i * c + k], a, q, ql);
    }
    const double eh = s2 / pi;
    p[i] = pi;
    e[i] = eh;
    elo[i] = (fma(-eh, pi, s2) + s2l) / pi;   // e_i = eh + elo: the quotient's remainder and the sum's low part
  }
  const double s = loo_block_sum(q, red), sl = loo_block_sum(ql, red);   // partq [blocks][2]: high and low parts of Q
  if (threadIdx.x == 0) {
    partq[2 * blockIdx.x] = s;
    partq[2 * blockIdx.x + 1] = sl;
  }
}

// out[q] = sum over parts of part[t * nq + q], q < nq <= 4, in a fixed order.  head != 0: out = {Lambda, lQ, d/d df, d/d scale}
// of loo_point_kernel's partials, and lQ gets its closed-form tail -N m2 / (s t_Q) (0 for the Gaussian head).
__global__ void __launch_bounds__(256) loo_sum_kernel(const double* __restrict__ part, int64_t nparts, int nq, double* __restrict__ out,
                                                      int head, LooHead h, const double* __restrict__ qp) {
  __shared__ double red[256];
  for (int q = 0; q < nq; ++q) {
    double v = 0.0;
    for (int64_t t = threadIdx.x; t < nparts; t += 256) v += part[t * nq + q];
    const double s = loo_block_sum(v, red);
    if (threadIdx.x == 0) out[q] = s;
  }
  if (head && threadIdx.x == 0) {
    double lq = 0.0;
    if (h.df > 0.0) {
      const double m2 = 0.5 * (h.df + (double)h.n * h.c), tq = h.df + (qp[0] + qp[1]) / h.scale;
      lq = out[1] - (double)h.n * m2 / (h.scale * tq);
    }
    out[1] = lq;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) loo_point_kernel(const T* __restrict__ alpha, const T* __restrict__ y, LooHead h,
                                                        const double* __restrict__ p, const double* __restrict__ e,
                                                        const double* __restrict__ elo, const double* __restrict__ qp,
                                                        T* __restrict__ mean,
                                                        T* __restrict__ scale2, double* __restrict__ acoef,
                                                        double* __restrict__ dvec, double* __restrict__ part) {
  __shared__ double red[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double Q = qp[0] + qp[1], C = (double)h.c;   // qp = {high, low} part of Q
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < h.n) {
    const double pi = p[i], ei = e[i];
    double le, s2;
    if (!(h.df > 0.0)) {
      le = -0.5;
      s2 = 1.0 / pi;
      v[0] = 0.5 * C * log(pi) - 0.5 * ei;
    } else {
      const double s = h.scale, dfc = h.df + (double)(h.n - 1) * C;
      const double m1 = 0.5 * dfc, m2 = 0.5 * (h.df + (double)h.n * C);
      const double qme = (qp[0] - ei) + (qp[1] - elo[i]);   // Q - e_i from the two-part sums: no cancellation error
      const double ti = h.df + qme / s, tq = h.df + Q / s;
      le = -m1 / (s * ti);
      s2 = ti / dfc * s / pi;
      v[0] = 0.5 * C * log(pi) + m1 * log(ti) - m2 * log(tq);
      v[1] = m1 / (s * ti);
      v[2] = 0.5 * log(ti) + m1 / ti - 0.5 * log(tq) - m2 / tq;
      v[3] = -0.5 * C / s - m1 * qme / (s * s * ti) + m2 * Q / (s * s * tq);
    }
    dvec[i] = 0.5 * C / pi - le * ei / pi;
    if (scale2) scale2[i] = (T)s2;
    for (int k = 0; k < h.c; ++k) {
      const double a = (double)alpha[i * h.c + k];
      if (mean) mean[i * h.c + k] = (T)((double)y[i * h.c + k] - a / pi);
      acoef[i * h.c + k] = 2.0 * le * a / pi;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double s = loo_block_sum(v[q], red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 4 + q] = s;
  }
}

// 32 x 32 tiles of the lower triangle of nk (= -P): the tile and, through LDS, its mirror image go into the full zero-padded
// copy np [npad, npad] and, scaled column-wise by d, into sp.
template <typename T>
__global__ void __launch_bounds__(256) loo_pack_kernel(const T* __restrict__ nk, int64_t ldk, int64_t n, const double* __restrict__ dvec,
                                                       T* __restrict__ np, T* __restrict__ sp, int64_t ld) {
  __shared__ T tile[32][33];
  const int tr = blockIdx.y, tc = blockIdx.x;
  if (tc > tr) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t j = (int64_t)tc * 32 + tx;
  const double dj = j < n ? dvec[j] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = (int64_t)tr * 32 + ty + 8 * r;
    T v = T(0);
    if (i < n && j < n) {
      const int64_t hi = i > j ? i : j, lo = i > j ? j : i;   // (a diagonal tile reads its upper half from the lower one)
      v = nk[hi * ldk + lo];
    }
    np[i * ld + j] = v;
    sp[i * ld + j] = (T)((double)v * dj);
    tile[ty + 8 * r][tx] = v;
  }
  if (tc == tr) return;
  __syncthreads();
  const int64_t j2 = (int64_t)tr * 32 + tx;
  const double dj2 = j2 < n ? dvec[j2] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i2 = (int64_t)tc * 32 + ty + 8 * r;
    const T v = tile[tx][ty + 8 * r];
    np[i2 * ld + j2] = v;
    sp[i2 * ld + j2] = (T)((double)v * dj2);
  }
}

// w[i, k] = -(sum_j np[i, j] acoef[j, k]) / 2 + lQ alpha[i, k] / 2: one wave per row, the row read once per group of CB columns
// (rows_dot_multi_kernel's shape, cholesky.hip); fp64 sums in a fixed order.
template <typename T, int CB>
__global__ void __launch_bounds__(256) loo_u_kernel(const T* __restrict__ np, int64_t ld, const double* __restrict__ acoef,
                                                    const T* __restrict__ alpha, int64_t n, int c, const double* __restrict__ lqp,
                                                    double* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const double lq = *lqp;
  for (int c0 = 0; c0 < c; c0 += CB) {
    double s[CB];
#pragma unroll
    for (int e = 0; e < CB; ++e) s[e] = 0.0;
    for (int64_t k = lane; k < n; k += 64) {
      const double xv = (double)np[row * ld + k];
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        const int ce = c0 + e < c ? c0 + e : c - 1;
        s[e] += xv * acoef[k * c + ce];
      }
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) {
      double v = s[e];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (lane == 0 && c0 + e < c) w[row * c + c0 + e] = -0.5 * v + 0.5 * lq * (double)alpha[row * c + c0 + e];
    }
  }
}

// g[i, j] = -sum_k np[i, k] sp[j, k] for j <= i < n: one workgroup per lower 128 x 128 tile, K = ld (= n_pad) -- the launch
// shape of syrk_rows_kernel (cholesky.hip) with a second operand.
template <typename T>
__global__ void __launch_bounds__(256, 2) loo_pdp_kernel(const T* __restrict__ np, const T* __restrict__ sp, int64_t ld,
                                                        T* __restrict__ g, int64_t ldg, int64_t n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Tile = MainTile<T>;
  using M = typename Tile::M;
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  const int64_t row0 = (int64_t)tr * kTile, col0 = (int64_t)tc * kTile;
  Tile t;
  t.zero();
  t.mainloop(np + row0 * ld, ld, sp + col0 * ld, ld, (int)ld, smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int m = 0; m < Tile::MT; ++m)
#pragma unroll
    for (int nn = 0; nn < Tile::NT; ++nn)
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        const int64_t gr = row0 + wr * Tile::WM + m * M::TM + M::acc_row(lane, i);
        const int64_t gc = col0 + wc * Tile::WN + nn * M::TN + M::acc_col(lane);
        if (gr < n && gc <= gr) g[gr * ldg + gc] = -t.acc[m][nn][i];
      }
}

// g[i, j] -= sum_k w[i, k] alpha[j, k] + alpha[i, k] w[j, k] for j <= i < n: 64 x 64 tiles of the lower triangle, a thread owns
// one column and 16 rows (the row side is wave-uniform); the 2 C terms of an entry are summed in fp64 and rounded once.
// Diagonal tiles are mirrored: nothing else is written above the diagonal.
template <typename T>
__global__ void __launch_bounds__(256) loo_rank_kernel(T* __restrict__ g, int64_t ldg, const T* __restrict__ alpha,
                                                       const double* __restrict__ w, int64_t n, int c) {
  constexpr int GT = 64, NR = GT / 4;
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  const int64_t row0 = (int64_t)tr * GT, col0 = (int64_t)tc * GT;
  const int lc = threadIdx.x % GT;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / GT);
  const int64_t j = col0 + lc, jc = j < n ? j : n - 1;
  double acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.0;
  for (int k = 0; k < c; ++k) {
    const double aj = (double)alpha[jc * c + k], wj = w[jc * c + k];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = row0 + wv + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
      acc[r] = fma(w[ic * c + k], aj, fma((double)alpha[ic * c + k], wj, acc[r]));
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t i = row0 + wv + 4 * r;
    if (i < n && j <= i) {
      const T v = (T)((double)g[i * ldg + j] - acc[r]);
      g[i * ldg + j] = v;
      // the tangent passes walk 64 x 64 tiles and multiply what lies above the diagonal inside a diagonal tile by zero: it has
      // to be finite there, so a diagonal tile is left whole (symmetric)
      if (tr == tc && j < i) g[j * ldg + i] = v;
    }
  }
}

template <typename T>
__global__ void loo_fill_nan_kernel(T* __restrict__ a, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) a[i] = (T)__builtin_nan("");
}

template <typename T>
int loo_fill_nan(smn_ctx* ctx, void* a, int64_t count) {
  if (!a || count <= 0) return SMN_OK;
  hipLaunchKernelGGL(loo_fill_nan_kernel<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<T*>(a), count);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

int loo_fill_nan(smn_ctx* ctx, int dtype, void* a, int64_t count) {
  return by_dtype(dtype, [&](auto e) { return loo_fill_nan<decltype(e)>(ctx, a, count); });
}

double loo_digamma(double x) {   // x > 0: recurrence up to 16, then the asymptotic series (first term left out: 0.021 / x^12 < 1e-16)
  double r = 0.0;
  while (x < 16.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  return r + std::log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
}

// doubles of workspace slot 13 in front of the zero vector the fused entries hand to the tangent pass
size_t loo_small_doubles(int64_t n, int64_t c) {
  const size_t nb = (size_t)((n + 255) / 256);
  return 4 * (size_t)n + 2 * (size_t)n * (size_t)c + 6 * nb + 8;
}

template <typename T>
int loo_head_t(smn_ctx* ctx, const void* nkinv, int64_t ldk, const void* alpha, const void* y, int64_t n, int64_t c, double df,
               double scale, double* lam_h, void* mean, void* scale2, double* dhead_h, void* g, int64_t ldg) {
  const int64_t nb = (n + 255) / 256;
  void* sv = nullptr;
  SMN_TRY(smn_workspace(ctx, 13, sizeof(double) * (loo_small_doubles(n, c) + (size_t)n), &sv));
  double* p = static_cast<double*>(sv);
  double* e = p + n;
  double* elo = e + n;
  double* dvec = elo + n;
  double* acoef = dvec + n;
  double* w = acoef + n * c;
  double* partq = w + n * c;
  double* part = partq + 2 * nb;
  double* out = part + 4 * nb;   // out[0..3] = Lambda, lQ, d/d df, d/d scale; out[4..5] = Q (high, low part)
  const T* nk = static_cast<const T*>(nkinv);
  const T* al = static_cast<const T*>(alpha);
  const T* yy = static_cast<const T*>(y);
  const LooHead h{df, scale, n, (int)c};
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(loo_diag_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, nk, ldk, al, yy, n, (int)c, p, e, elo, partq);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(256), 0, st, partq, nb, 2, out + 4, 0, h, out + 4);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(loo_point_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, al, yy, h, p, e, elo, out + 4, static_cast<T*>(mean),
                     static_cast<T*>(scale2), acoef, dvec, part);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(256), 0, st, part, nb, 4, out, 1, h, out + 4);
  SMN_CHECK_LAUNCH(ctx);
  if (g) {
    const int64_t n_pad = round_up(n, kTile);
    void* bv = nullptr;
    SMN_TRY(smn_workspace(ctx, 12, sizeof(T) * 2 * (size_t)n_pad * (size_t)n_pad, &bv));
    T* np = static_cast<T*>(bv);
    T* sp = np + (size_t)n_pad * (size_t)n_pad;
    {
      const unsigned tp = (unsigned)(n_pad / 32);
      hipLaunchKernelGGL(loo_pack_kernel<T>, dim3(tp, tp), dim3(256), 0, st, nk, ldk, n, dvec, np, sp, n_pad);
      SMN_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL((loo_u_kernel<T, 8>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, np, n_pad, acoef, al, n, (int)c, out + 1, w);
    SMN_CHECK_LAUNCH(ctx);
    {
      const int64_t t = n_pad / kTile, ntiles = t * (t + 1) / 2;
      SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(loo_pdp_kernel<T>), MainTile<T>::LDS_BYTES));
      ProfScope ps(ctx, PROF_MISC, st);
      hipLaunchKernelGGL(loo_pdp_kernel<T>, dim3((unsigned)ntiles), dim3(256), MainTile<T>::LDS_BYTES, st, np, sp, n_pad,
                         static_cast<T*>(g), ldg, n);
      SMN_CHECK_LAUNCH(ctx);
    }
    {
      const int64_t t = (n + 63) / 64, ntiles = t * (t + 1) / 2;
      hipLaunchKernelGGL(loo_rank_kernel<T>, dim3((unsigned)ntiles), dim3(256), 0, st, static_cast<T*>(g), ldg, al, w, n, (int)c);
      SMN_CHECK_LAUNCH(ctx);
    }
  }
  double r[4];
  SMN_HIP(ctx, hipMemcpyAsync(r, out, sizeof r, hipMemcpyDeviceToHost, st));
  SMN_HIP(ctx, hipStreamSynchronize(st));
  const double N = (double)n, C = (double)c;
  double lam = r[0], ddf = 0.0, dsc = 0.0;
  if (!(df > 0.0)) {
    lam += N * (-0.5 * C * std::log(2.0 * M_PI));
  } else {
    const double m1 = 0.5 * (df + (N - 1.0) * C), m2 = 0.5 * (df + N * C);
    lam += N * (std::lgamma(m2) - std::lgamma(m1) - 0.5 * C * std::log(M_PI) - 0.5 * C * std::log(scale));
    ddf = r[2] + N * 0.5 * (loo_digamma(m2) - loo_digamma(m1));
    dsc = r[3];
  }
  if (lam_h) *lam_h = lam;
  if (dhead_h) {
    dhead_h[0] = ddf;
    dhead_h[1] = dsc;
  }
  return SMN_OK;
}

int loo_head(smn_ctx* ctx, int dtype, const void* nkinv, int64_t ldk, const void* alpha, const void* y, int64_t n, int64_t c,
             double df, double scale, double* lam_h, void* mean, void* scale2, double* dhead_h, void* g, int64_t ldg) {
  return by_dtype(dtype, [&](auto e) {
    return loo_head_t<decltype(e)>(ctx, nkinv, ldk, alpha, y, n, c, df, scale, lam_h, mean, scale2, dhead_h, g, ldg);
  });
}

// not positive definite: NaN in every output
int loo_all_nan(smn_ctx* ctx, int dtype, int64_t n, int64_t c, double* lam_h, void* mean, void* scale2, double* dhead_h,
                double* terms_h, void* g, int64_t ldg) {
  const double nan = std::nan("");
  if (lam_h) *lam_h = nan;
  if (dhead_h) dhead_h[0] = dhead_h[1] = nan;
  for (int i = 0; i < 4 && terms_h; ++i) terms_h[i] = nan;
  SMN_TRY(loo_fill_nan(ctx, dtype, mean, n * c));
  SMN_TRY(loo_fill_nan(ctx, dtype, scale2, n));
  if (g) SMN_TRY(loo_fill_nan(ctx, dtype, g, (n - 1) * ldg + n));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}

int loo_check(smn_ctx* ctx, const char* who, int dtype, int64_t n, int64_t c, double df, double scale) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (n <= 0 || c < 1) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes", who);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  if (df > 0.0 && !(scale > 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: scale must be > 0", who);
  return SMN_OK;
}

// the n zeros (of the storage type) behind the head's doubles in slot 13: the alpha of a tangent pass that is fed a seed
int loo_zero_alpha(smn_ctx* ctx, int dtype, int64_t n, int64_t c, void** zeros) {
  void* sv = nullptr;
  SMN_TRY(smn_workspace(ctx, 13, sizeof(double) * (loo_small_doubles(n, c) + (size_t)n), &sv));
  *zeros = static_cast<double*>(sv) + loo_small_doubles(n, c);
  SMN_HIP(ctx, hipMemsetAsync(*zeros, 0, dtype_size(dtype) * (size_t)n, ctx->stream));
  return SMN_OK;
}

// What the two gradient entries do between the factored posterior and their tangent pass: info out; NaN in every output when K~
// did not factor (*zeros stays null: no tangent pass); else the head with its seed written over -K~^-1, and the zero alpha
int loo_seed(smn_ctx* ctx, int dtype, const Posterior& p, const void* y_d, int64_t n, int64_t c, double df, double scale,
             double* lam_h, double* dhead_h, int* info_h, double* terms_h, void* mean, void* scale2, void** zeros) {
  *zeros = nullptr;
  if (info_h) *info_h = p.info;
  if (p.info != 0) return loo_all_nan(ctx, dtype, n, c, lam_h, mean, scale2, dhead_h, terms_h, nullptr, 0);
  SMN_TRY(loo_head(ctx, dtype, p.ninv, p.ldinv, p.alpha, y_d, n, c, df, scale, lam_h, mean, scale2, dhead_h, p.ninv, p.ldinv));
  return loo_zero_alpha(ctx, dtype, n, c, zeros);
}

}  // namespace

extern "C" int smn_loo_head(smn_ctx* ctx, int dtype, const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, const void* y_d,
                            int64_t n, int64_t c, double df, double scale, double* loo_logpdf_h, void* loo_mean_d,
                            void* loo_scale2_d, double dhead_h[2], void* g_d, int64_t ldg) {
  if (!ctx || !neg_kinv_d || !alpha_d || !y_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(loo_check(ctx, "smn_loo_head", dtype, n, c, df, scale));
  SMN_CHECK_LD(ctx, "smn_loo_head", ldkinv, n);
  if (g_d) SMN_CHECK_LD(ctx, "smn_loo_head", ldg, n);
  return loo_head(ctx, dtype, neg_kinv_d, ldkinv, alpha_d, y_d, n, c, df, scale, loo_logpdf_h, loo_mean_d, loo_scale2_d, dhead_h,
                  g_d, ldg);
}

extern "C" int smn_loo_multi(smn_ctx* ctx, int dtype, void* k_d, int64_t n, int64_t ldk, const void* y_d, int64_t c, double eps_abs,
                             double df, double scale, double* loo_logpdf_h, void* loo_mean_d, void* loo_scale2_d,
                             double dhead_h[2], double* logdet_h, int* info_h, void* g_d, int64_t ldg) {
  if (!ctx || !k_d || !y_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(loo_check(ctx, "smn_loo_multi", dtype, n, c, df, scale));
  SMN_CHECK_LD(ctx, "smn_loo_multi", ldk, n);
  if (g_d) SMN_CHECK_LD(ctx, "smn_loo_multi", ldg, n);
  const KernelInto build = [&](void* w_d, int64_t ldw) { return copy_matrix(ctx, dtype, w_d, ldw, k_d, ldk, n, n, 1); };
  Posterior p;
  SMN_TRY(posterior_from_build(ctx, dtype, n, build, y_d, c, eps_abs, &p));
  if (logdet_h) *logdet_h = p.logdet;
  if (info_h) *info_h = p.info;
  if (p.info != 0) return loo_all_nan(ctx, dtype, n, c, loo_logpdf_h, loo_mean_d, loo_scale2_d, dhead_h, nullptr, g_d, ldg);
  return loo_head(ctx, dtype, p.ninv, p.ldinv, p.alpha, y_d, n, c, df, scale, loo_logpdf_h, loo_mean_d, loo_scale2_d, dhead_h, g_d,
                  ldg);
}

// Everything from x and Y [n,c] for the MLP / dense-ResNet kernels: Gram matrix, factorisation with identity (heads.hip: both
// routes), the head with its seed written over -K~^-1, then the tangent pass of grad.hip over that seed.
extern "C" int smn_spr_loo_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                                double eps_abs, double df, double scale, double* loo_logpdf_h, double dhead_h[2], int* info_h,
                                double terms_h[4], void* loo_mean_d, void* loo_scale2_d) {
  if (!ctx || !x_d || !y_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(loo_check(ctx, "smn_spr_loo_grad", dtype, n, c, df, scale));
  if (d <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_spr_loo_grad: bad sizes");
  SMN_CHECK_LD(ctx, "smn_spr_loo_grad", ldx, d);
  const BuildSpec spec{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};
  Posterior p;
  SMN_TRY(posterior_from_x(ctx, spec, x_d, n, ldx, d, y_d, c, eps_abs, &p));
  void* zeros = nullptr;
  SMN_TRY(loo_seed(ctx, dtype, p, y_d, n, c, df, scale, loo_logpdf_h, dhead_h, info_h, terms_h, loo_mean_d, loo_scale2_d, &zeros));
  if (!zeros) return SMN_OK;
  return smn_lml_grad_terms(ctx, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, p.k0, n, p.ld0, p.q, p.ninv, p.ldinv,
                            zeros, 0.0, terms_h);
}

// The same for get_cnn_kernel: the conv build of the lower triangle straight into the factorisation workspace, and the
// tangent pass of cnn_grad.hip over the seed (H * W <= SMN_CNN_GRAD_MAX_PIXELS).
extern "C" int smn_spr_cnn_loo_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                    double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                    const void* y_d, int64_t c, double eps_abs, double df, double scale, double* loo_logpdf_h,
                                    double dhead_h[2], int* info_h, double terms_h[4], void* loo_mean_d, void* loo_scale2_d) {
  if (!ctx || !x_d || !y_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(loo_check(ctx, "smn_spr_cnn_loo_grad", dtype, n, c, df, scale));
  if (H <= 0 || W <= 0 || C <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_spr_cnn_loo_grad: bad sizes");
  if (H * W > SMN_CNN_GRAD_MAX_PIXELS)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_spr_cnn_loo_grad: images of more than %d pixels", SMN_CNN_GRAD_MAX_PIXELS);
  if (!(last_w_std != 0.0)) return smn_fail(ctx, SMN_EINVAL, "smn_spr_cnn_loo_grad: bad hyper-parameters");
  const BuildSpec spec{dtype, SMN_NET_MLP, act, num_hiddens, w_std, b_std, last_w_std};   // (net: not read by the conv build)
  Posterior p;
  SMN_TRY(posterior_from_images(ctx, spec, x_d, n, H, W, C, y_d, c, eps_abs, &p));
  void* zeros = nullptr;
  SMN_TRY(loo_seed(ctx, dtype, p, y_d, n, c, df, scale, loo_logpdf_h, dhead_h, info_h, terms_h, loo_mean_d, loo_scale2_d, &zeros));
  if (!zeros) return SMN_OK;
  return smn_kernel_cnn_grad_terms(ctx, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, p.ninv, p.ldinv, zeros,
                                   0.0, terms_h);
}

// -K~^-1 and A = K~^-1 Y exactly as the gradient entries form them (Gram matrix, layer recursion, factorisation with identity:
// the joint route below n_pad = 8192, the rectangle route from there on), left where the caller can read them: what
// smn_loo_head is fed inside smn_spr_loo_grad.  neg_kinv_d [n,n] (ld = ldkinv, a multiple of 16 bytes): the lower triangle is
// valid on both routes.
extern "C" int smn_spr_kinv(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                            double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                            double eps_abs, void* neg_kinv_d, int64_t ldkinv, void* alpha_d, double* logdet_h, int* info_h) {
  if (!ctx || !x_d || !y_d || !neg_kinv_d || !alpha_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(loo_check(ctx, "smn_spr_kinv", dtype, n, c, 0.0, 1.0));
  const size_t es = dtype_size(dtype);
  if (d <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_spr_kinv: bad sizes");
  SMN_CHECK_LD(ctx, "smn_spr_kinv", ldx, d);
  SMN_CHECK_LD(ctx, "smn_spr_kinv", ldkinv, n);
  if (ldkinv % (16 / (int64_t)es))
    return smn_fail(ctx, SMN_EINVAL, "smn_spr_kinv: ldkinv = %lld is not a multiple of 16 bytes", (long long)ldkinv);
  const BuildSpec spec{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};
  Posterior p;
  SMN_TRY(posterior_from_x(ctx, spec, x_d, n, ldx, d, y_d, c, eps_abs, &p, neg_kinv_d, ldkinv, alpha_d));
  if (logdet_h) *logdet_h = p.logdet;
  if (info_h) *info_h = p.info;
  return SMN_OK;
}
