// pcg.hip — smn_pcg_solve: preconditioned conjugate gradients on (K + lambda I) X = B with K applied by smn_kernel_mlp_matmul.
//
// c independent CG recurrences that share one K-apply per iteration: every column has its own alpha and beta, its own stopping
// test, and leaves the shared product when it has stopped.  X, R, Z, P and K~P are fp64 [n, c]; only the operand of the K-apply
// is cast to `dtype`.  The preconditioner is M = L L^T + lambda I, applied by the Woodbury identity
//     M^-1 r = (r - L (lambda I + L^T L)^-1 L^T r) / lambda
// with the m x m matrix formed once (smn_lowrank_gram), factored once (smn_cholesky, fp64) and applied by two smn_trsm.
//
// Every inner product is summed in a fixed order: rows in chunks of kDotRows, a chunk by a fixed tree of 256 partial sums, the
// chunks ascending; L^T R by splits of kDotRows rows ascending.  No floating-point atomics: two calls give the same bits.  The
// CG scalars are formed on the host from those sums (two small copies and synchronisations per iteration beside one K-apply).
#include <cmath>
#include <vector>

#include "internal.hpp"

int matmul_check(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, const void* x1_d, int64_t n1, int64_t ldx1,
                 const void* x2_d, int64_t n2, int64_t ldx2, int64_t d, BuildSpec* spec, bool* ntk);   // kernel_matmul.hip

namespace {

constexpr int kMaxCols = 48;
constexpr int kDotRows = 1024;   // rows per chunk of an inner product / per split of L^T R
constexpr int kLtrChunk = 8;     // columns of R one pass of the L^T R kernel keeps in registers

struct ColList { int n; int idx[kMaxCols]; };
struct ColScal { double v[kMaxCols]; };

// part[chunk, k] = sum over the chunk's rows of a[i, col_k] b[i, col_k] for the listed columns
__global__ void __launch_bounds__(256) pcg_dot_kernel(const double* __restrict__ a, int64_t lda, const double* __restrict__ b, int64_t ldb,
                                                      int64_t n, ColList cols, double* __restrict__ part) {
  __shared__ double sh[256];
  const int col = cols.idx[blockIdx.y];
  const int64_t r0 = (int64_t)blockIdx.x * kDotRows;
  const int64_t r1 = r0 + kDotRows < n ? r0 + kDotRows : n;
  double s = 0.0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) s = fma(a[i * lda + col], b[i * ldb + col], s);
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(int64_t)blockIdx.x * cols.n + blockIdx.y] = sh[0];
}

// out[e] = sum over the chunks, ascending
__global__ void pcg_sum_kernel(const double* __restrict__ part, int64_t chunks, int64_t count, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
  for (int64_t q = 0; q < chunks; ++q) s += part[q * count + e];
  out[e] = s;
}

// dst[i, a] = (T) src[i, idx[a]]: the operand of the K-apply
template <typename T>
__global__ void pcg_pack_kernel(const double* __restrict__ src, int64_t lds, int64_t n, ColList cols, T* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  const int64_t i = e / cols.n;
  const int a = (int)(e % cols.n);
  dst[e] = (T)src[i * lds + cols.idx[a]];
}

// w[i, idx[a]] = kp[i, a] + lambda p[i, idx[a]]
__global__ void pcg_shift_kernel(const double* __restrict__ kp, const double* __restrict__ p, int64_t n, int c, ColList cols, double lambda,
                                 double* __restrict__ w) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  const int64_t i = e / cols.n;
  const int a = (int)(e % cols.n);
  const int64_t o = i * c + cols.idx[a];
  w[o] = fma(lambda, p[o], kp[e]);
}

// r[i, idx[a]] = b[i, idx[a]] - (kx[i, a] + lambda x[i, idx[a]])
__global__ void pcg_residual_kernel(const double* __restrict__ b, int64_t ldb, const double* __restrict__ kx, const double* __restrict__ x,
                                    int64_t ldx, int64_t n, int c, ColList cols, double lambda, double* __restrict__ r) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  const int64_t i = e / cols.n;
  const int a = (int)(e % cols.n);
  const int col = cols.idx[a];
  r[i * c + col] = b[i * ldb + col] - fma(lambda, x[i * ldx + col], kx[e]);
}

// x += alpha p, r -= alpha w on the listed columns
__global__ void pcg_update_kernel(double* __restrict__ x, int64_t ldx, double* __restrict__ r, const double* __restrict__ p,
                                  const double* __restrict__ w, int64_t n, int c, ColList cols, ColScal alpha) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  const int64_t i = e / cols.n;
  const int col = cols.idx[(int)(e % cols.n)];
  const double al = alpha.v[col];
  x[i * ldx + col] = fma(al, p[i * c + col], x[i * ldx + col]);
  r[i * c + col] = fma(-al, w[i * c + col], r[i * c + col]);
}

// p = z + beta p on the listed columns
__global__ void pcg_direction_kernel(double* __restrict__ p, const double* __restrict__ z, int64_t n, int c, ColList cols, ColScal beta) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  const int64_t i = e / cols.n;
  const int col = cols.idx[(int)(e % cols.n)];
  p[i * c + col] = fma(beta.v[col], p[i * c + col], z[i * c + col]);
}

// dst[i, k] = value for every k < c (value NaN: a breakdown's outputs; 0: the start)
__global__ void pcg_fill_kernel(double* __restrict__ dst, int64_t ld, int64_t n, int c, double value) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * c) return;
  dst[(e / c) * ld + e % c] = value;
}

// dst[i, idx[a]] = 0
__global__ void pcg_zero_cols_kernel(double* __restrict__ dst, int64_t ld, int64_t n, ColList cols) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cols.n) return;
  dst[(e / cols.n) * ld + cols.idx[(int)(e % cols.n)]] = 0.0;
}

// dst[i, k] = src[i, k] (k < c; leading dimensions may differ)
__global__ void pcg_copy_kernel(double* __restrict__ dst, int64_t ldd, const double* __restrict__ src, int64_t lds, int64_t n, int c) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * c) return;
  dst[(e / c) * ldd + e % c] = src[(e / c) * lds + e % c];
}

// One split of U = L^T R in fp64, rows ascending: thread = column a of L.  part[(split, a, k)]
template <typename T>
__global__ void __launch_bounds__(256) pcg_ltr_kernel(const T* __restrict__ L, int64_t n, int m, int64_t ldl, const double* __restrict__ r,
                                                      int c, double* __restrict__ part) {
  const int64_t s = blockIdx.x;
  const int64_t r0 = s * kDotRows;
  const int64_t r1 = r0 + kDotRows < n ? r0 + kDotRows : n;
  const int a = blockIdx.y * 256 + threadIdx.x;
  if (a >= m) return;
  for (int k0 = 0; k0 < c; k0 += kLtrChunk) {
    double acc[kLtrChunk];
#pragma unroll
    for (int q = 0; q < kLtrChunk; ++q) acc[q] = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      const double l = (double)L[i * ldl + a];
#pragma unroll
      for (int q = 0; q < kLtrChunk; ++q)
        if (k0 + q < c) acc[q] = fma(l, r[i * c + k0 + q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < kLtrChunk; ++q)
      if (k0 + q < c) part[(s * m + a) * c + k0 + q] = acc[q];
  }
}

// z[i, k] = (r[i, k] - sum_a L[i, a] s[a, k]) / lambda, a ascending (m == 0: z = r / lambda)
template <typename T>
__global__ void pcg_apply_kernel(const T* __restrict__ L, int64_t n, int m, int64_t ldl, const double* __restrict__ s,
                                 const double* __restrict__ r, int c, double lambda, double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * c) return;
  const int64_t i = e / c;
  const int k = (int)(e % c);
  double acc = 0.0;
  for (int a = 0; a < m; ++a) acc = fma((double)L[i * ldl + a], s[(int64_t)a * c + k], acc);
  z[e] = (r[e] - acc) / lambda;
}

inline unsigned blocks_for(int64_t count) { return (unsigned)((count + 255) / 256); }

struct Pcg {
  smn_ctx* ctx; int dtype; int64_t n; int c; double lambda;
  const void* L; int64_t m, ldl;
  double *R, *Z, *P, *W, *KP, *U, *part, *dots, *G;
  void* Pc;

  // out_h[k] = a[:, idx[k]] . b[:, idx[k]] for the listed columns (entries of the others are left alone).  Synchronises.
  int dot(const double* a, int64_t lda, const double* b, int64_t ldb, const ColList& cols, double* out_h) {
    if (cols.n == 0) return SMN_OK;
    const int64_t chunks = (n + kDotRows - 1) / kDotRows;
    hipLaunchKernelGGL(pcg_dot_kernel, dim3((unsigned)chunks, (unsigned)cols.n), dim3(256), 0, ctx->stream, a, lda, b, ldb, n, cols, part);
    SMN_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(pcg_sum_kernel, dim3(1), dim3(64), 0, ctx->stream, part, chunks, (int64_t)cols.n, dots);
    SMN_CHECK_LAUNCH(ctx);
    double tmp[kMaxCols];
    SMN_HIP(ctx, hipMemcpyAsync(tmp, dots, sizeof(double) * (size_t)cols.n, hipMemcpyDeviceToHost, ctx->stream));
    SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int a2 = 0; a2 < cols.n; ++a2) out_h[cols.idx[a2]] = tmp[a2];
    return SMN_OK;
  }

  // Z = M^-1 R (every column: the m x m side does not notice the idle ones)
  int precondition() {
    return by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      const T* Lt = static_cast<const T*>(L);
      if (m > 0) {
        const int64_t splits = (n + kDotRows - 1) / kDotRows;
        hipLaunchKernelGGL(pcg_ltr_kernel<T>, dim3((unsigned)splits, (unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, Lt, n, (int)m,
                           ldl, R, c, part);
        SMN_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(pcg_sum_kernel, dim3(blocks_for(m * c)), dim3(256), 0, ctx->stream, part, splits, m * c, U);
        SMN_CHECK_LAUNCH(ctx);
        SMN_TRY(smn_trsm(ctx, SMN_F64, G, m, m, U, c, c, 0));
        SMN_TRY(smn_trsm(ctx, SMN_F64, G, m, m, U, c, c, 1));
      }
      hipLaunchKernelGGL(pcg_apply_kernel<T>, dim3(blocks_for(n * c)), dim3(256), 0, ctx->stream, Lt, n, (int)m, ldl, U, R, c, lambda, Z);
      SMN_CHECK_LAUNCH(ctx);
      return (int)SMN_OK;
    });
  }

  int pack(const double* src, int64_t lds, const ColList& cols) {
    return by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      hipLaunchKernelGGL(pcg_pack_kernel<T>, dim3(blocks_for(n * cols.n)), dim3(256), 0, ctx->stream, src, lds, n, cols, static_cast<T*>(Pc));
      SMN_CHECK_LAUNCH(ctx);
      return (int)SMN_OK;
    });
  }
};

}  // namespace

extern "C" int smn_pcg_solve(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                             const void* x_d, int64_t n, int64_t ldx, int64_t d, double lambda, const void* L_d, int64_t m, int64_t ldl,
                             const double* b_d, int64_t c, int64_t ldb, double tol, int max_iter, int warm, double* sol_d, int64_t lds,
                             int* iters_h, int* col_iters_h, double* resid_h, double* hist_h, int* info_h) {
  if (!ctx) return SMN_EINVAL;
  const char* who = "smn_pcg_solve";
  BuildSpec spec{};
  bool ntk = false;
  SMN_TRY(matmul_check(ctx, who, dtype, net, act, num_hiddens, x_d, n, ldx, nullptr, 0, 0, d, &spec, &ntk));
  if (!(lambda > 0.0) || !std::isfinite(lambda)) return smn_fail(ctx, SMN_EINVAL, "%s: lambda = %g is not a positive number", who, lambda);
  if (!(tol > 0.0 && tol < 1.0)) return smn_fail(ctx, SMN_EINVAL, "%s: tol = %g is not in (0, 1)", who, tol);
  if (max_iter < 1) return smn_fail(ctx, SMN_EINVAL, "%s: max_iter = %d", who, max_iter);
  if (m < 0 || m > n) return smn_fail(ctx, SMN_EINVAL, "%s: m = %lld outside [0, n = %lld]", who, (long long)m, (long long)n);
  if (!L_d) m = 0;
  if (m > SMN_LOWRANK_MAX_RANK)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: m = %lld is above SMN_LOWRANK_MAX_RANK = %d", who, (long long)m, SMN_LOWRANK_MAX_RANK);
  if (m > 0) SMN_CHECK_LD(ctx, who, ldl, m);
  if (c < 1 || c > kMaxCols) return smn_fail(ctx, c > kMaxCols ? SMN_ENOTSUP : SMN_EINVAL, "%s: c = %lld outside [1, %d]", who, (long long)c, kMaxCols);
  if (!b_d || !sol_d || !iters_h || !resid_h || !info_h) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  SMN_CHECK_LD(ctx, who, ldb, c);
  SMN_CHECK_LD(ctx, who, lds, c);
  SMN_ENTER(ctx);

  const int C = (int)c;
  const size_t es = dtype_size(dtype);
  const size_t vec = al256(sizeof(double) * (size_t)n * (size_t)c);
  const int64_t chunks = (n + kDotRows - 1) / kDotRows;
  const size_t part_bytes = al256(sizeof(double) * (size_t)chunks * (size_t)c * (size_t)(m > 0 ? m : 1));
  const size_t u_bytes = al256(sizeof(double) * (size_t)(m > 0 ? m : 1) * (size_t)c);
  void *base = nullptr, *gv = nullptr;
  SMN_TRY(smn_workspace(ctx, 17, 5 * vec + al256(es * (size_t)n * (size_t)c) + part_bytes + u_bytes + 512, &base));
  SMN_TRY(smn_workspace(ctx, 18, sizeof(double) * (size_t)(m > 0 ? m * m : 1), &gv));
  Pcg s{};
  s.ctx = ctx; s.dtype = dtype; s.n = n; s.c = C; s.lambda = lambda; s.L = L_d; s.m = m; s.ldl = ldl;
  char* p = static_cast<char*>(base);
  s.R = reinterpret_cast<double*>(p); p += vec;
  s.Z = reinterpret_cast<double*>(p); p += vec;
  s.P = reinterpret_cast<double*>(p); p += vec;
  s.W = reinterpret_cast<double*>(p); p += vec;
  s.KP = reinterpret_cast<double*>(p); p += vec;
  s.Pc = p; p += al256(es * (size_t)n * (size_t)c);
  s.part = reinterpret_cast<double*>(p); p += part_bytes;
  s.U = reinterpret_cast<double*>(p); p += u_bytes;
  s.dots = reinterpret_cast<double*>(p);
  s.G = static_cast<double*>(gv);
  hipStream_t st = ctx->stream;
  const double nan = std::nan("");

  auto apply_k = [&](const double* src, int64_t ld_src, const ColList& cols) -> int {   // KP[:, a] = K cast(src[:, idx[a]])
    SMN_TRY(s.pack(src, ld_src, cols));
    return smn_kernel_mlp_matmul(ctx, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, nullptr, 0, 0, d, 0.0, s.Pc,
                                 cols.n, cols.n, s.KP, cols.n);
  };
  auto breakdown = [&]() -> int {
    hipLaunchKernelGGL(pcg_fill_kernel, dim3(blocks_for(n * c)), dim3(256), 0, st, sol_d, lds, n, C, nan);
    SMN_CHECK_LAUNCH(ctx);
    for (int k = 0; k < C; ++k) {
      resid_h[k] = nan;
      if (col_iters_h) col_iters_h[k] = -1;
    }
    *info_h = 2;
    return SMN_OK;
  };

  // the preconditioner's m x m side, once per call: G = lambda I + L^T L = C C^T in fp64
  if (m > 0) {
    SMN_TRY(smn_lowrank_gram(ctx, dtype, L_d, n, m, ldl, nullptr, nullptr, 0, 0, s.G, m, nullptr, nullptr));
    int ginfo = 0;
    SMN_TRY(smn_cholesky(ctx, SMN_F64, s.G, m, m, m, m, lambda, 0.0, &ginfo, nullptr));
    if (ginfo != 0) {
      *iters_h = 0;
      return breakdown();
    }
  }

  ColList all{};
  all.n = C;
  for (int k = 0; k < C; ++k) all.idx[k] = k;
  double bb[kMaxCols], rr[kMaxCols], rz[kMaxCols], pw[kMaxCols], bnorm[kMaxCols];
  SMN_TRY(s.dot(b_d, ldb, b_d, ldb, all, bb));
  ColList nz{};   // columns with a non-zero right-hand side
  for (int k = 0; k < C; ++k) {
    bnorm[k] = std::sqrt(bb[k]);
    if (bb[k] > 0.0 && std::isfinite(bb[k])) nz.idx[nz.n++] = k;
    else if (!(bb[k] == 0.0)) { *iters_h = 0; return breakdown(); }   // a non-finite right-hand side
  }
  if (!warm) {
    hipLaunchKernelGGL(pcg_fill_kernel, dim3(blocks_for(n * c)), dim3(256), 0, st, sol_d, lds, n, C, 0.0);
    SMN_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(pcg_copy_kernel, dim3(blocks_for(n * c)), dim3(256), 0, st, s.R, c, b_d, ldb, n, C);
    SMN_CHECK_LAUNCH(ctx);
  } else {
    hipLaunchKernelGGL(pcg_fill_kernel, dim3(blocks_for(n * c)), dim3(256), 0, st, s.R, c, n, C, 0.0);
    SMN_CHECK_LAUNCH(ctx);
    if (nz.n > 0) {
      SMN_TRY(apply_k(sol_d, lds, nz));
      hipLaunchKernelGGL(pcg_residual_kernel, dim3(blocks_for(n * nz.n)), dim3(256), 0, st, b_d, ldb, s.KP, sol_d, lds, n, C, nz, lambda, s.R);
      SMN_CHECK_LAUNCH(ctx);
    }
    if (nz.n < C) {   // a zero right-hand side has the solution zero, whatever the start
      ColList zc{};
      for (int k = 0; k < C; ++k)
        if (!(bb[k] > 0.0)) zc.idx[zc.n++] = k;
      hipLaunchKernelGGL(pcg_zero_cols_kernel, dim3(blocks_for(n * zc.n)), dim3(256), 0, st, sol_d, lds, n, zc);
      SMN_CHECK_LAUNCH(ctx);
    }
  }
  std::vector<int> col_it((size_t)C, 0);
  for (int k = 0; k < C; ++k) rr[k] = 0.0;
  SMN_TRY(s.dot(s.R, c, s.R, c, nz, rr));
  ColList act_cols{};
  for (int k = 0; k < C; ++k) {
    const double rel = bb[k] > 0.0 ? std::sqrt(rr[k]) / bnorm[k] : 0.0;
    if (hist_h) hist_h[k] = rel;
    if (bb[k] > 0.0 && !std::isfinite(rel)) { *iters_h = 0; return breakdown(); }
    if (bb[k] > 0.0 && !(std::sqrt(rr[k]) <= tol * bnorm[k])) act_cols.idx[act_cols.n++] = k;
  }
  int it = 0;
  if (act_cols.n > 0) {
    SMN_TRY(s.precondition());
    hipLaunchKernelGGL(pcg_copy_kernel, dim3(blocks_for(n * c)), dim3(256), 0, st, s.P, c, s.Z, c, n, C);
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(s.dot(s.R, c, s.Z, c, act_cols, rz));
  }
  while (act_cols.n > 0 && it < max_iter) {
    ++it;
    SMN_TRY(apply_k(s.P, c, act_cols));
    hipLaunchKernelGGL(pcg_shift_kernel, dim3(blocks_for(n * act_cols.n)), dim3(256), 0, st, s.KP, s.P, n, C, act_cols, lambda, s.W);
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(s.dot(s.P, c, s.W, c, act_cols, pw));
    ColScal alpha{};
    for (int a = 0; a < act_cols.n; ++a) {
      const int k = act_cols.idx[a];
      alpha.v[k] = rz[k] / pw[k];
      if (!(pw[k] > 0.0) || !std::isfinite(alpha.v[k])) { *iters_h = it; return breakdown(); }
    }
    hipLaunchKernelGGL(pcg_update_kernel, dim3(blocks_for(n * act_cols.n)), dim3(256), 0, st, sol_d, lds, s.R, s.P, s.W, n, C, act_cols, alpha);
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(s.dot(s.R, c, s.R, c, act_cols, rr));
    ColList next{};
    for (int k = 0; k < C; ++k)
      if (hist_h) hist_h[(size_t)it * (size_t)C + (size_t)k] = bb[k] > 0.0 ? std::sqrt(rr[k]) / bnorm[k] : 0.0;
    for (int a = 0; a < act_cols.n; ++a) {
      const int k = act_cols.idx[a];
      if (!std::isfinite(rr[k])) { *iters_h = it; return breakdown(); }
      if (std::sqrt(rr[k]) <= tol * bnorm[k]) col_it[(size_t)k] = it;
      else next.idx[next.n++] = k;
    }
    act_cols = next;
    if (act_cols.n == 0 || it == max_iter) break;
    SMN_TRY(s.precondition());
    double rz_new[kMaxCols];
    SMN_TRY(s.dot(s.R, c, s.Z, c, act_cols, rz_new));
    ColScal beta{};
    for (int a = 0; a < act_cols.n; ++a) {
      const int k = act_cols.idx[a];
      beta.v[k] = rz_new[k] / rz[k];
      if (!std::isfinite(beta.v[k])) { *iters_h = it; return breakdown(); }
      rz[k] = rz_new[k];
    }
    hipLaunchKernelGGL(pcg_direction_kernel, dim3(blocks_for(n * act_cols.n)), dim3(256), 0, st, s.P, s.Z, n, C, act_cols, beta);
    SMN_CHECK_LAUNCH(ctx);
  }
  for (int a = 0; a < act_cols.n; ++a) col_it[(size_t)act_cols.idx[a]] = it;   // still running at max_iter
  if (hist_h)
    for (int j = it + 1; j <= max_iter; ++j)
      for (int k = 0; k < C; ++k) hist_h[(size_t)j * (size_t)C + (size_t)k] = nan;   // iterations that were not run

  // the true residual of the returned solution: one further K-apply
  for (int k = 0; k < C; ++k) resid_h[k] = 0.0;
  if (nz.n > 0) {
    SMN_TRY(apply_k(sol_d, lds, nz));
    hipLaunchKernelGGL(pcg_residual_kernel, dim3(blocks_for(n * nz.n)), dim3(256), 0, st, b_d, ldb, s.KP, sol_d, lds, n, C, nz, lambda, s.W);
    SMN_CHECK_LAUNCH(ctx);
    double tt[kMaxCols];
    SMN_TRY(s.dot(s.W, c, s.W, c, nz, tt));
    for (int a = 0; a < nz.n; ++a) resid_h[nz.idx[a]] = std::sqrt(tt[nz.idx[a]]) / bnorm[nz.idx[a]];
  }
  *iters_h = it;
  for (int k = 0; k < C && col_iters_h; ++k) col_iters_h[k] = col_it[(size_t)k];
  *info_h = act_cols.n > 0 ? 1 : 0;
  return SMN_OK;
}
