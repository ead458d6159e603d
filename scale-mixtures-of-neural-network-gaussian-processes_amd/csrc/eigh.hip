// eigh.hip — symmetric positive definite eigendecomposition on the device (smn_eigh_pd) and the finite-time
// gradient-descent predictions built on it (smn_predict_gd).
//
// smn_eigh_pd:  A = L L^T by the project's factorisation (cholesky.hip, untouched), then one-sided (Hestenes) Jacobi on the
// rows of M = L^T: rotations J from the left make the rows of J^T M mutually orthogonal, and with A = M^T M = (J^T M)^T (J^T M)
// the eigenvectors are the normalised rows and the eigenvalues their squared norms -- no separate accumulation of V.
// Working on the factor instead of A keeps the small eigenvalues to the accuracy of the factorisation (Veselic & Hari).
//   - M is kept in fp64 for both dtypes (the fp32 factor converts exactly), so the only fp32 rounding of the fp32 solver
//     is the factorisation's and the final store;
//   - pairs follow the round-robin ("tournament") order: the pairs of one round are disjoint, one workgroup per pair, one
//     launch per round, n - 1 (n even) or n (n odd) rounds per sweep; a round is bandwidth-bound (it streams M once);
//   - every sum runs in a fixed order (strided partial sums per thread, a fixed butterfly per wave, the four waves added
//     in order): two calls on the same input give the same bits;
//   - a pair is converged when |g_i . g_j| <= n u ||g_i|| ||g_j|| (u of the caller's dtype); pairs above fp64 round-off are
//     still rotated, so the sweep that reports convergence has left the rows orthogonal far below the test's level.  The
//     device sets one word per sweep, the HOST reads it once per sweep and decides; no workgroup waits on another and
//     every loop has a fixed bound;
//   - ascending order at the end: the host sorts the n squared norms, one kernel permutes, scales and stores.
// This is the UNBLOCKED form: 3 n^3 flops per sweep on the vector ALU against ~6 n^3 on MFMA for the blocked form with
// Gram blocks ("Symmetric eigensolver"); its cost is the (n - 1) passes over M per sweep.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <numeric>

#include "internal.hpp"

namespace {

constexpr int kEighSlot = 14, kGdSlot = 15;
constexpr int kMaxSweepsCap = 1000;

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// fixed-order sum over the 256 threads of a workgroup; every thread returns the total
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// M[k, i] = L[i, k] for i >= k, 0 below: the rows of M are the columns of the factor (fp64 copy)
template <typename T>
__global__ void factor_rows_kernel(double* __restrict__ m, int64_t n, const T* __restrict__ l, int64_t ldl) {
  __shared__ double tile[32][33];
  const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;   // block of L: rows r0.., columns c0..
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t r = r0 + i, c = c0 + threadIdx.x;
    tile[i][threadIdx.x] = (r < n && c < n && c <= r) ? (double)l[r * ldl + c] : 0.0;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t c = c0 + i, r = r0 + threadIdx.x;
    if (c < n && r < n) m[c * n + r] = tile[threadIdx.x][i];
  }
}

// One round of the tournament: workgroup k owns the pair (p, q) of round `round` among m = n rounded up to even players.
__global__ __launch_bounds__(256) void jacobi_round_kernel(double* __restrict__ m_d, int64_t n, int m, int round, double tol,
                                                           int* __restrict__ flag) {
  __shared__ double red[4];
  const int k = blockIdx.x;
  int p, q;
  if (k == 0) {
    p = m - 1;
    q = round;
  } else {
    p = (round + k) % (m - 1);
    q = (round - k + (m - 1)) % (m - 1);
  }
  if (p >= n || q >= n) return;   // the bye of an odd n (uniform over the workgroup)
  if (p > q) { const int s = p; p = q; q = s; }
  double* __restrict__ a = m_d + (int64_t)p * n;
  double* __restrict__ b = m_d + (int64_t)q * n;
  double saa = 0.0, sbb = 0.0, sab = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double x = a[i], y = b[i];
    saa = fma(x, x, saa);
    sbb = fma(y, y, sbb);
    sab = fma(x, y, sab);
  }
  saa = block_sum(saa, red);
  sbb = block_sum(sbb, red);
  sab = block_sum(sab, red);
  const double g = fabs(sab), lim = sqrt(saa) * sqrt(sbb);
  if (!(g <= tol * lim) && threadIdx.x == 0) *flag = 1;   // (a NaN counts as not converged)
  if (!(g > DBL_EPSILON * lim)) return;
  const double zeta = (sbb - saa) / (2.0 * sab);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  // Rutishauser's form of the update, x - s (y + tau x) and y + s (x - tau y) with tau = s / (1 + c) (= c x - s y and s x + c y):
  // the rounding of s and tau enters scaled by |s|, where a rounded c would rescale the whole row by 1 + O(u) at EVERY
  // rotation, however small its angle -- a coherent error that lands in the eigenvalues (fp64 r_l 1.1-1.5 with the c, s form: profiles/r15_gd_predict.txt)
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t, tau = s / (1.0 + c);
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double x = a[i], y = b[i];
    a[i] = x - s * (y + tau * x);
    b[i] = y + s * (x - tau * y);
  }
}

__global__ __launch_bounds__(256) void row_norms_kernel(const double* __restrict__ m_d, int64_t n, double* __restrict__ nrm2) {
  __shared__ double red[4];
  const double* a = m_d + (int64_t)blockIdx.x * n;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s = fma(a[i], a[i], s);
  s = block_sum(s, red);
  if (threadIdx.x == 0) nrm2[blockIdx.x] = s;
}

// w[k] = ||row perm[k]||^2, vt[k, :] = row perm[k] / its norm  (vt rows are the eigenvectors, ld = n)
template <typename T>
__global__ __launch_bounds__(256) void eig_store_kernel(const double* __restrict__ m_d, int64_t n, const double* __restrict__ nrm2,
                                                        const int* __restrict__ perm, T* __restrict__ w, T* __restrict__ vt) {
  const int64_t k = blockIdx.x;
  const int src = perm[k];
  const double lam = nrm2[src], inv = 1.0 / sqrt(lam);
  const double* a = m_d + (int64_t)src * n;
  for (int64_t i = threadIdx.x; i < n; i += 256) vt[k * n + i] = (T)(a[i] * inv);
  if (threadIdx.x == 0) w[k] = (T)lam;
}

template <typename T>
__global__ void fill_kernel(T* __restrict__ dst, int64_t ld, int64_t rows, int64_t cols, T value) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) dst[r * ld + c] = value;
}

int fill_matrix(smn_ctx* ctx, int dtype, void* dst, int64_t ld, int64_t rows, int64_t cols, double value) {
  if (rows <= 0 || cols <= 0) return SMN_OK;
  dim3 g((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768));
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(fill_kernel<T>, g, dim3(256), 0, ctx->stream, static_cast<T*>(dst), ld, rows, cols, (T)value);
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

// The solver proper.  a [n, n] (lower triangle read, ld = lda) + (jitter_abs + ridge_rel tr(a) / n) I, the shift applied by
// the factorisation exactly as smn_cholesky applies it.  w_d [n]; vt_d [n, n] (ld = n, ROWS are eigenvectors) and / or
// v_d (ld = ldv, COLUMNS are eigenvectors); either may be null.  info != 0 from the factorisation: outputs NaN.
int eigh_core(smn_ctx* ctx, int dtype, const void* a_d, int64_t n, int64_t lda, double jitter_abs, double ridge_rel, void* w_d,
              void* vt_d, void* v_d, int64_t ldv, int max_sweeps, int* info_h, int* sweeps_h) {
  const size_t es = dtype_size(dtype);
  if (max_sweeps <= 0) max_sweeps = 30;
  if (max_sweeps > kMaxSweepsCap) return smn_fail(ctx, SMN_EINVAL, "smn_eigh_pd: max_sweeps = %d is above %d", max_sweeps, kMaxSweepsCap);
  if (n > (int64_t)1 << 30) return smn_fail(ctx, SMN_ENOTSUP, "smn_eigh_pd: n = %lld is too large", (long long)n);
  const int64_t np = round_up(n, kTile);
  const size_t b_l = align256(es * (size_t)np * (size_t)np), b_m = align256(sizeof(double) * (size_t)n * (size_t)n),
               b_nrm = align256(sizeof(double) * (size_t)n), b_perm = align256(sizeof(int) * (size_t)n),
               b_flag = align256(sizeof(int) * (size_t)max_sweeps), b_vt = align256(es * (size_t)n * (size_t)n);
  void* ws = nullptr;
  SMN_TRY(smn_workspace(ctx, kEighSlot, b_l + b_m + b_nrm + b_perm + b_flag + b_vt, &ws));
  char* base = static_cast<char*>(ws);
  void* lw = base;
  double* m_d = reinterpret_cast<double*>(base + b_l);
  double* nrm_d = reinterpret_cast<double*>(base + b_l + b_m);
  int* perm_d = reinterpret_cast<int*>(base + b_l + b_m + b_nrm);
  int* flag_d = reinterpret_cast<int*>(base + b_l + b_m + b_nrm + b_perm);
  void* vt_own = base + b_l + b_m + b_nrm + b_perm + b_flag;
  if (!vt_d) vt_d = vt_own;

  // the factorisation, on a padded copy (A is not modified): the route smn_cholesky takes for unaligned operands
  SMN_HIP(ctx, hipMemsetAsync(lw, 0, es * (size_t)np * (size_t)np, ctx->stream));
  SMN_TRY(copy_matrix(ctx, dtype, lw, np, a_d, lda, n, n, 1));
  SMN_TRY(fill_identity_pad(ctx, dtype, lw, np, np, n));
  SMN_TRY(cholesky_padded(ctx, FactorCall{dtype, lw, np, np, np, n, jitter_abs, ridge_rel, true}));
  HeadScalars head;
  SMN_TRY(fetch_results(ctx, nullptr, 0, &head));
  const int info = head.info;
  if (sweeps_h) *sweeps_h = 0;
  if (info != 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (w_d) SMN_TRY(fill_matrix(ctx, dtype, w_d, n, 1, n, nan));
    if (vt_d != vt_own) SMN_TRY(fill_matrix(ctx, dtype, vt_d, n, n, n, nan));
    if (v_d) SMN_TRY(fill_matrix(ctx, dtype, v_d, ldv, n, n, nan));
    if (info_h) *info_h = info;
    return SMN_OK;
  }

  {
    dim3 g((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), b(32, 8);
    by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      hipLaunchKernelGGL(factor_rows_kernel<T>, g, b, 0, ctx->stream, m_d, n, static_cast<const T*>(lw), np);
    });
    SMN_CHECK_LAUNCH(ctx);
  }
  const double u = dtype == SMN_F64 ? DBL_EPSILON : (double)FLT_EPSILON;
  const double tol = (double)n * u;
  const int m = (int)((n + 1) / 2 * 2);
  int sweeps = 0;
  bool converged = n == 1;
  if (n > 1) {
    SMN_HIP(ctx, hipMemsetAsync(flag_d, 0, sizeof(int) * (size_t)max_sweeps, ctx->stream));
    for (int s = 0; s < max_sweeps && !converged; ++s) {
      for (int r = 0; r < m - 1; ++r) {
        hipLaunchKernelGGL(jacobi_round_kernel, dim3((unsigned)(m / 2)), dim3(256), 0, ctx->stream, m_d, n, m, r, tol, flag_d + s);
      }
      SMN_CHECK_LAUNCH(ctx);
      int f = 1;
      SMN_HIP(ctx, hipMemcpyAsync(&f, flag_d + s, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
      ++sweeps;
      converged = f == 0;
    }
  }
  hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, m_d, n, nrm_d);
  SMN_CHECK_LAUNCH(ctx);
  std::vector<double> nrm((size_t)n);
  SMN_HIP(ctx, hipMemcpyAsync(nrm.data(), nrm_d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return nrm[(size_t)x] < nrm[(size_t)y]; });
  SMN_HIP(ctx, hipMemcpyAsync(perm_d, perm.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  void* w_out = w_d ? w_d : static_cast<void*>(nrm_d);   // (never the case for the public entry)
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(eig_store_kernel<T>, dim3((unsigned)n), dim3(256), 0, ctx->stream, m_d, n, nrm_d, perm_d,
                       static_cast<T*>(w_out), static_cast<T*>(vt_d));
  });
  SMN_CHECK_LAUNCH(ctx);
  if (v_d) SMN_TRY(transpose_matrix(ctx, dtype, v_d, ldv, vt_d, n, n, n));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));   // perm is host memory of this frame
  if (sweeps_h) *sweeps_h = sweeps;
  if (info_h) *info_h = converged ? 0 : -1;
  return SMN_OK;
}

// ---------------------------------------------------------------------------------------------- smn_predict_gd
enum { SCALE_NONE = 0, SCALE_D = 1, SCALE_E = 2 };

// dst[r, k] = src[r, k] * f(lambda_k) * mult;  f = 1, d(lambda) = -expm1(-lambda s) / lambda or e(lambda) = -expm1(-2 lambda s) / lambda
// (s = +inf: 1 / lambda for both); eigenvalues clamped at 0, where the limits s and 2 s stand in.
template <typename T>
__global__ void scale_cols_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds, int64_t rows, int64_t cols,
                                  const T* __restrict__ lam, int mode, double s, double mult) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cols) return;
  double f = mult;
  if (mode != SCALE_NONE) {
    const double l = fmax((double)lam[k], 0.0), ss = mode == SCALE_E ? 2.0 * s : s;
    f *= l > 0.0 ? (isinf(ss) ? 1.0 / l : -expm1(-l * ss) / l) : ss;
  }
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) dst[r * ldd + k] = (T)((double)src[r * lds + k] * f);
}

// dst[i, j] = src[max(i, j), min(i, j)]: a full symmetric copy from the lower triangle
template <typename T>
__global__ void sym_copy_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) dst[i * ldd + j] = i >= j ? src[i * lds + j] : src[j * lds + i];
}

// cov[i, j] = K**[hi, lo] + s1[hi, lo] * sg1 - (s2[i, j] + s2[j, i])   (s2 null: nngp mode, sg1 = -1); symmetric to the bit
template <typename T>
__global__ void gd_cov_kernel(T* __restrict__ cov, int64_t ldc, const T* __restrict__ kss, int64_t ldk, const T* __restrict__ s1,
                              const T* __restrict__ s2, int64_t t, double sg1) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t) return;
  for (int64_t i = blockIdx.y; i < t; i += gridDim.y) {
    const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    double v = (double)kss[hi * ldk + lo] + sg1 * (double)s1[hi * t + lo];
    if (s2) v -= (double)s2[i * t + j] + (double)s2[j * t + i];
    cov[i * ldc + j] = (T)v;
  }
}

struct Gd {
  smn_ctx* ctx; int dtype; size_t es; void* scratch;
  // out [ra, rb] (ld = ldo) = (A [ra, k] with column j scaled by f(lambda_j)) B [rb, k]^T through the NT product of smn_gram
  // (which divides by k: the scaled copy of A carries the factor k)
  int nt(const void* a, int64_t ra, int64_t lda, const void* b, int64_t rb, int64_t ldb, int64_t k, void* out, int64_t ldo,
         int mode = SCALE_NONE, const void* lam = nullptr, double s = 0.0) const {
    dim3 g((unsigned)((k + 255) / 256), (unsigned)(ra < 32768 ? ra : 32768));
    by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      hipLaunchKernelGGL(scale_cols_kernel<T>, g, dim3(256), 0, ctx->stream, static_cast<T*>(scratch), k,
                         static_cast<const T*>(a), lda, ra, k, static_cast<const T*>(lam), mode, s, (double)k);
    });
    SMN_CHECK_LAUNCH(ctx);
    return smn_gram(ctx, dtype, scratch, ra, k, b, rb, ldb, k, out, ldo, nullptr, nullptr);
  }
};

}  // namespace

extern "C" int smn_eigh_pd(smn_ctx* ctx, int dtype, const void* a_d, int64_t n, int64_t lda, void* w_d, void* v_d, int64_t ldv,
                           int max_sweeps, int* info_h, int* sweeps_h) {
  if (!ctx || !a_d || !w_d || !v_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (n <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_eigh_pd: empty");
  SMN_CHECK_LD(ctx, "smn_eigh_pd", lda, n);
  SMN_CHECK_LD(ctx, "smn_eigh_pd", ldv, n);
  return eigh_core(ctx, dtype, a_d, n, lda, 0.0, 0.0, w_d, nullptr, v_d, ldv, max_sweeps, info_h, sweeps_h);
}

extern "C" int smn_predict_gd(smn_ctx* ctx, int dtype, const void* k_joint_d, const void* theta_joint_d, int64_t n, int64_t t,
                              int64_t ld, const void* y_d, int64_t c, double diag_rel, double diag_abs, const double* times_h,
                              int64_t nt, double learning_rate, void* mean_d, void* cov_d, int64_t ldc, void* evals_d,
                              int* info_h) {
  if (!ctx || !k_joint_d || !y_d || !times_h || !mean_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (n <= 0 || t <= 0 || c <= 0 || nt <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_predict_gd: empty");
  SMN_CHECK_LD(ctx, "smn_predict_gd", ld, n + t);
  if (cov_d) SMN_CHECK_LD(ctx, "smn_predict_gd", ldc, t);
  if (!(learning_rate >= 0.0) || std::isinf(learning_rate)) return smn_fail(ctx, SMN_EINVAL, "smn_predict_gd: bad learning_rate");
  for (int64_t j = 0; j < nt; ++j)
    if (!(times_h[j] >= 0.0)) return smn_fail(ctx, SMN_EINVAL, "smn_predict_gd: times_h[%lld] is negative or NaN", (long long)j);
  const size_t es = dtype_size(dtype);
  const bool ntk = theta_joint_d != nullptr;
  const char* kj = static_cast<const char*>(k_joint_d);
  const char* gj = ntk ? static_cast<const char*>(theta_joint_d) : kj;
  auto at = [&](const char* p, int64_t r, int64_t col) { return static_cast<const void*>(p + es * (size_t)(r * ld + col)); };

  // workspace: V^T, lambda, the scaled left operand, P, y^T, z^T, one [t, t] product; NTK: K_dd (full), V^T K_dd, K^, Q^T, R, a second [t, t]
  const int64_t rmax = std::max(std::max(n, t), c);
  const size_t b_nn = align256(es * (size_t)n * (size_t)n), b_tn = align256(es * (size_t)t * (size_t)n),
               b_cn = align256(es * (size_t)c * (size_t)n), b_tt = align256(es * (size_t)t * (size_t)t),
               b_n = align256(es * (size_t)n), b_scr = align256(es * (size_t)rmax * (size_t)n);
  size_t total = b_nn + b_n + b_scr + b_tn + 2 * b_cn + b_tt;
  if (ntk) total += 3 * b_nn + 2 * b_tn + b_tt;
  void* ws = nullptr;
  SMN_TRY(smn_workspace(ctx, kGdSlot, total, &ws));
  char* p = static_cast<char*>(ws);
  auto take = [&](size_t b) { char* r = p; p += b; return static_cast<void*>(r); };
  void* vt = take(b_nn); void* lam = take(b_n); void* scratch = take(b_scr);
  void* pm = take(b_tn); void* yt = take(b_cn); void* zt = take(b_cn); void* s1 = take(b_tt);
  void *kdd = nullptr, *u = nullptr, *khat = nullptr, *qt = nullptr, *r = nullptr, *s2 = nullptr;
  if (ntk) { kdd = take(b_nn); u = take(b_nn); khat = take(b_nn); qt = take(b_tn); r = take(b_tn); s2 = take(b_tt); }

  int info = 0;
  SMN_TRY(eigh_core(ctx, dtype, gj, n, ld, diag_abs, diag_rel, lam, vt, nullptr, n, 0, &info, nullptr));
  if (info_h) *info_h = info;
  if (evals_d) SMN_TRY(copy_matrix(ctx, dtype, evals_d, n, lam, n, 1, n, 0));
  if (info != 0) {   // not positive definite, or not converged: NaN, like the other predictive entries
    const double nan = std::numeric_limits<double>::quiet_NaN();
    SMN_TRY(fill_matrix(ctx, dtype, mean_d, c, nt * t, c, nan));
    if (cov_d) SMN_TRY(fill_matrix(ctx, dtype, cov_d, ldc, nt * t, t, nan));
    return SMN_OK;
  }
  const Gd gd{ctx, dtype, es, scratch};
  // once: P = G_*d V, z^T = y^T V; NTK: K^ = V^T K_dd V, Q^T = K_*d V
  SMN_TRY(gd.nt(at(gj, n, 0), t, ld, vt, n, n, n, pm, n));
  SMN_TRY(transpose_matrix(ctx, dtype, yt, n, y_d, c, n, c));
  SMN_TRY(gd.nt(yt, c, n, vt, n, n, n, zt, n));
  if (ntk && cov_d) {
    dim3 g((unsigned)((n + 255) / 256), (unsigned)(n < 32768 ? n : 32768));
    by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      hipLaunchKernelGGL(sym_copy_kernel<T>, g, dim3(256), 0, ctx->stream, static_cast<T*>(kdd), n, static_cast<const T*>(k_joint_d), ld, n);
    });
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(gd.nt(vt, n, n, kdd, n, n, n, u, n));
    SMN_TRY(gd.nt(u, n, n, vt, n, n, n, khat, n));
    SMN_TRY(gd.nt(at(kj, n, 0), t, ld, vt, n, n, n, qt, n));
  }
  for (int64_t j = 0; j < nt; ++j) {
    const double s = learning_rate * times_h[j] / ((double)n * (double)c);
    char* mean_j = static_cast<char*>(mean_d) + es * (size_t)(j * t * c);
    SMN_TRY(gd.nt(pm, t, n, zt, c, n, n, mean_j, c, SCALE_D, lam, s));
    if (!cov_d) continue;
    char* cov_j = static_cast<char*>(cov_d) + es * (size_t)(j * t * ldc);
    double sg1 = -1.0;
    if (!ntk) {
      SMN_TRY(gd.nt(pm, t, n, pm, t, n, n, s1, t, SCALE_E, lam, s));          // (P . e) P^T
    } else {
      SMN_TRY(gd.nt(pm, t, n, khat, n, n, n, r, n, SCALE_D, lam, s));         // R = (P . d) K^
      SMN_TRY(gd.nt(pm, t, n, qt, t, n, n, s2, t, SCALE_D, lam, s));          // (P . d) Q = A_t K_d*
      SMN_TRY(gd.nt(r, t, n, pm, t, n, n, s1, t, SCALE_D, lam, s));           // R (P . d)^T = (R . d) P^T
      sg1 = 1.0;
    }
    dim3 g((unsigned)((t + 255) / 256), (unsigned)(t < 32768 ? t : 32768));
    by_dtype(dtype, [&](auto e) {
      using T = decltype(e);
      hipLaunchKernelGGL(gd_cov_kernel<T>, g, dim3(256), 0, ctx->stream, reinterpret_cast<T*>(cov_j), ldc,
                         static_cast<const T*>(at(kj, n, n)), ld, static_cast<const T*>(s1), static_cast<const T*>(s2), t, sg1);
    });
    SMN_CHECK_LAUNCH(ctx);
  }
  return SMN_OK;
}
