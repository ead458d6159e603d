// svsp_train.hip — the training half of the sparse variational scale-mixture classifier: the negative ELBO of SVSP.loss
// (spax/models.py:30-56, spax/priors.py:21-26,36-42,52-58,70-82, spax/utils.py:53-58 of the reference) and its analytic
// gradient with respect to everything but the inducing images:
//   smn_rng_variates_ddf   the Student-t variates of smn_rng_variates together with their derivative in df (Bailey's polar
//                          method is differentiable in df at fixed (u, v); acceptance does not depend on df)
//   smn_svsp_head_grad     the correlated Monte-Carlo softmax head, forward and backward: L_c = chol(scale cov[c]),
//                          f = mean + L xi, ll = mean log-softmax at the label; gmean, gcov (through the reverse-mode
//                          Cholesky), gscale and the pathwise df term
//   smn_svsp_elbo_grad     -ll and kl/N from K([Z; x], [Z; x]), q_mu, q_var, and the reverse pass through the sparse-posterior
//                          algebra: g q_mu, g q_var, g eps, g s, and Gbar = d loss / d K over the union of inducing and batch images
// Everything but the variates and the exponentials of the head is fp64 (the reason smn_svsp_moments gives: a 1e-6 jitter is
// not numerically positive definite in fp32).  Every sum has a fixed order -- no floating-point atomics -- so two calls give
// the same bits.  The factorisations are cholesky_padded (cholesky.hip) one problem after the other: its batched form does
// not keep the factors, which the head samples with.  The I x I inverses are two smn_trsm sweeps over an identity.
// Sizes are those of a mini-batch (I ~ 200, B <= 256, C <= 128): the dense products below are a plain LDS-tiled fp64 kernel
// with grid.z = the class; nothing here is large enough for the 128 x 128 tile engine of the kernel build to fill a tile.
#include <climits>
#include <cmath>
#include <limits>
#include <vector>

#include "internal.hpp"

namespace {

#include "svsp_rng.hpp"

constexpr int kMaxC = SMN_SVSP_MAX_CLASSES;
constexpr int kMaxB = SMN_SVSP_MAX_BATCH;
static_assert(kMaxB == 256, "chol_reverse_kernel: one thread per column of a class's [B,B] matrices");

// ---------------------------------------------------------------- variates
// out[p * sp + c * sc + s] = variate of (point0 + p, class c, draw s), computed in T, stored as O; dout = d/d df (df > 0 only)
template <typename T, typename O>
__global__ void __launch_bounds__(256) variates_kernel(uint32_t k0, uint32_t k1, T df, uint32_t point0, int C, int64_t S,
                                                       int64_t sp, int64_t sc, O* __restrict__ out, O* __restrict__ dout) {
  const int64_t p = blockIdx.x;
  const int g = blockIdx.y;
  // with the derivative wanted, student_t_ddf gives the variate too (the expression of student_t: the same bits, which the
  // tests compare with smn_rng_variates), so that no variate is generated twice
  const bool both = dout && df > T(0);
  for (int64_t s = threadIdx.x; s < S; s += 256) {
    T z[4] = {T(0), T(0), T(0), T(0)};
    if (!both) draw4<T>(k0, k1, (uint32_t)s, point0 + (uint32_t)p, g, C, df, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * g + k;
      if (c < C) {
        T dt = T(0);
        if (both) z[k] = student_t_ddf<T>(k0, k1, (uint32_t)s, point0 + (uint32_t)p, (uint32_t)c, df, dt);
        out[p * sp + c * sc + s] = (O)z[k];
        if (dout) dout[p * sp + c * sc + s] = (O)dt;
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) widen_kernel(const T* __restrict__ in, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// ---------------------------------------------------------------- small dense helpers (all fp64)
// dst [batch][np][np] <- scale * lower(src [batch][n][n], ld = lds, batch stride sbs); identity on the padded diagonal, zero
// elsewhere: the padded operand of cholesky_padded
__global__ void __launch_bounds__(256) pack_lower_kernel(const double* __restrict__ src, int64_t lds, int64_t sbs, int64_t n,
                                                         int64_t np, double scale, double* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  if (j >= np) return;
  double v = 0.0;
  if (i < n && j <= i) v = scale * src[b * sbs + i * lds + j];
  else if (i >= n && j == i) v = 1.0;
  dst[(b * np + i) * np + j] = v;
}

// After one cholesky_padded: *info_out = 0, or the 1-based index of the first pivot that is non-positive (the factorisation's
// own report) or below n u max_j K_jj (the rank tolerance smn_svsp_moments applies); *logdet_out = 2 sum log L_jj.
__global__ void __launch_bounds__(256) collect_kernel(const double* __restrict__ scal, const int* __restrict__ info_dev,
                                                      const double* __restrict__ l, int64_t ldl, int64_t n, double* logdet_out,
                                                      int* info_out) {
  __shared__ double s_max[256];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = INT_MAX;
  double m = 0.0;   // max_j K_jj = max_j sum_k L_jk^2 >= max_j L_jj^2: the diagonal of L L^T, rebuilt from the factor's rows
  for (int64_t j = tid; j < n; j += 256) {
    double r = 0.0;
    for (int64_t k = 0; k <= j; ++k) r = fma(l[j * ldl + k], l[j * ldl + k], r);
    m = fmax(m, r);
  }
  s_max[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = fmax(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  const double tol = (double)n * 0x1p-52 * s_max[0];
  for (int64_t j = tid; j < n; j += 256) {
    const double d = l[j * ldl + j];
    if (!(d * d > tol)) atomicMin(&s_bad, (int)(j + 1));
  }
  __syncthreads();
  if (tid == 0) {
    const int dev = info_dev[0];
    *info_out = (dev != INT_MAX && dev != 0) ? dev : (s_bad == INT_MAX ? 0 : s_bad);
    if (logdet_out) *logdet_out = scal[0];
  }
}

__global__ void __launch_bounds__(256) identity_kernel(double* __restrict__ a, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j < n) a[i * n + j] = i == j ? 1.0 : 0.0;
}

// C[z] = alpha op(A[z]) op(B[z]) + beta C[z];  op(A) is M x K, op(B) is K x N; row-major; ta / tb: the operand is stored
// transposed.  16 x 16 outputs per workgroup, K in steps of 16 through LDS; each output is one thread's sum in k order.
struct Gemm {
  int ta, tb;
  int64_t M, N, K;
  double alpha, beta;
  const double* A; int64_t lda, sa;
  const double* B; int64_t ldb, sb;
  double* C; int64_t ldc, sc;
};
__global__ void __launch_bounds__(256) gemm_kernel(Gemm g) {
  __shared__ double sA[16][17], sB[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t z = blockIdx.z;
  const double* A = g.A + z * g.sa;
  const double* B = g.B + z * g.sb;
  const int64_t m0 = (int64_t)blockIdx.y * 16, n0 = (int64_t)blockIdx.x * 16;
  double acc = 0.0;
  for (int64_t k0 = 0; k0 < g.K; k0 += 16) {
    {
      // sA[r][c] = op(A)(m0 + r, k0 + c); the thread index runs along the operand's contiguous dimension
      const int r = g.ta ? tx : ty, c = g.ta ? ty : tx;
      const int64_t m = m0 + r, k = k0 + c;
      sA[r][c] = (m < g.M && k < g.K) ? (g.ta ? A[k * g.lda + m] : A[m * g.lda + k]) : 0.0;
    }
    {
      // sB[r][c] = op(B)(k0 + r, n0 + c)
      const int r = g.tb ? tx : ty, c = g.tb ? ty : tx;
      const int64_t k = k0 + r, n = n0 + c;
      sB[r][c] = (k < g.K && n < g.N) ? (g.tb ? B[n * g.ldb + k] : B[k * g.ldb + n]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fma(sA[ty][k], sB[k][tx], acc);
    __syncthreads();
  }
  const int64_t m = m0 + ty, n = n0 + tx;
  if (m < g.M && n < g.N) {
    double* c = g.C + z * g.sc + m * g.ldc + n;
    *c = g.beta == 0.0 ? g.alpha * acc : fma(g.alpha, acc, g.beta * *c);
  }
}

int gemm(smn_ctx* ctx, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, int64_t sa,
         const double* B, int64_t ldb, int64_t sb, double beta, double* C, int64_t ldc, int64_t sc, int64_t batch = 1) {
  Gemm g{ta, tb, M, N, K, alpha, beta, A, lda, sa, B, ldb, sb, C, ldc, sc};
  hipLaunchKernelGGL(gemm_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)((M + 15) / 16), (unsigned)batch), dim3(256), 0,
                     ctx->stream, g);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

// out[0] = scale * sum_i in[i * stride], one workgroup, fixed order: thread t adds elements t, t + 256, ...; then an LDS tree
__global__ void __launch_bounds__(256) sum_kernel(const double* __restrict__ in, int64_t n, int64_t stride, double scale,
                                                  double* __restrict__ out) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t i = tid; i < n; i += 256) a += in[i * stride];
  s[tid] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = scale * s[0];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// out[r] = sum_s in[r * S + s]: one wave per row, lanes stride over s, butterfly at the end (the same order in every call)
__global__ void __launch_bounds__(64) row_sum_kernel(const double* __restrict__ in, int64_t S, double* __restrict__ out) {
  const int64_t r = blockIdx.x;
  double a = 0.0;
  for (int64_t s = threadIdx.x; s < S; s += 64) a += in[r * S + s];
  a = wave_sum(a);
  if (threadIdx.x == 0) out[r] = a;
}

// ---------------------------------------------------------------- the head: sample, softmax, reverse-mode Cholesky
// f[c,b,s] = mean[c,b] + sum_{k <= b} L_c[b,k] xi[c,k,s] (and h = sum L d xi / d df); lanes over the draws.  Both k-sums
// are reductions over the fp64 factor: they run and stay in fp64 (the variates in them are T values, widened)
__global__ void __launch_bounds__(256) sample_kernel(const double* __restrict__ mean, const double* __restrict__ lp, int64_t bp,
                                                     const double* __restrict__ xi, const double* __restrict__ dxi, int64_t B,
                                                     int64_t S, double* __restrict__ f, double* __restrict__ h) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, c = blockIdx.z;
  if (s >= S) return;
  const double* l = lp + (c * bp + b) * bp;
  const double* x = xi + c * B * S + s;
  double acc = mean[c * B + b];
  for (int64_t k = 0; k <= b; ++k) acc = fma(l[k], x[k * S], acc);
  f[(c * B + b) * S + s] = acc;
  if (dxi) {
    const double* dx = dxi + c * B * S + s;
    double hh = 0.0;
    for (int64_t k = 0; k <= b; ++k) hh = fma(l[k], dx[k * S], hh);
    h[(c * B + b) * S + s] = hh;
  }
}

// per (b, s): softmax over the classes; f is overwritten by gf = (softmax - onehot) / (B S);
// llpart[b,s] = log-softmax at the label, dfpart[b,s] = sum_c gf h.
// The exponentials and the logarithm are T: x_c = f_c - max f is formed in fp64 (exact shift, so the result does not depend
// on the level of f), rounded to T once, and e_c = exp(x_c) in T.  Their sum over the classes, the quotient e_c / sum and
// gf are fp64, as every reduction and gradient is.  Rounding x costs |x| 2^-24 relative on e_c, and |x| e^x <= 1 / e: every
// softmax entry is within a few 2^-24 ABSOLUTE of the exact one, whatever the magnitude of f.  (fm + log(sum) and f - lse
// in T would each add |f| 2^-24 to every class of the draw at once, which sums over draws of either sign do not forgive.)
template <typename T>
__global__ void __launch_bounds__(256) softmax_kernel(double* __restrict__ f, const double* __restrict__ h,
                                                      const int* __restrict__ labels, int C, int64_t B, int64_t S,
                                                      double* __restrict__ llpart, double* __restrict__ dfpart) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (s >= S) return;
  const int64_t cs = B * S, at = b * S + s;
  const int y = labels[b];
  double fm = f[at];
  for (int c = 1; c < C; ++c) fm = fmax(fm, f[c * cs + at]);
  double se = 0.0;
  for (int c = 0; c < C; ++c) se += (double)Real<T>::exp_((T)(f[c * cs + at] - fm));
  const double lse = (double)Real<T>::log_((T)se);
  const double inv = 1.0 / ((double)B * (double)S);
  double dfp = 0.0, lly = 0.0;
  for (int c = 0; c < C; ++c) {
    const double x = f[c * cs + at] - fm;
    if (c == y) lly = x - lse;
    const double g = ((double)Real<T>::exp_((T)x) / se - (c == y ? 1.0 : 0.0)) * inv;
    f[c * cs + at] = g;
    if (h) dfp = fma(g, h[c * cs + at], dfp);
  }
  llpart[at] = lly;
  if (dfpart) dfpart[at] = dfp;
}

// Reverse-mode Cholesky (Murray, arXiv:1602.07527, the unblocked symbolic form): from gL = d loss / d L (lower triangle read)
//   Phi = tril(L^T gL), diagonal halved;   Y = L^-T Phi;   W^T = Y L^-1 (as L^T W = Y^T);   gS = (W + W^T) / 2
//   gcov = scale gS;   gscale_part[c] = <gS, cov[c]>
// One workgroup per class; thread j owns column j of Phi, Y and W, so each of the three sweeps runs without a barrier
// inside it: the back substitution of a column reads only entries its own thread wrote.  The factor is read B^2 / 2 times
// per thread: it is kept in LDS, packed lower, when that fits (B <= 199 at 160 KB), and read through L2 otherwise.
__global__ void __launch_bounds__(256) chol_reverse_kernel(const double* __restrict__ lp, int64_t bp, const double* __restrict__ gl,
                                                           const double* __restrict__ cov, int64_t B, double scale, int in_lds,
                                                           double* __restrict__ ybuf, double* __restrict__ wbuf,
                                                           double* __restrict__ gcov, double* __restrict__ gscale_part) {
  extern __shared__ double s_l[];
  __shared__ double s_red[256];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const double* lg = lp + c * bp * bp;
  const double* g = gl + c * B * B;
  double* y = ybuf + c * B * B;
  double* w = wbuf + c * B * B;
  if (in_lds) {
    for (int64_t i = 0; i < B; ++i)
      for (int64_t k = tid; k <= i; k += 256) s_l[i * (i + 1) / 2 + k] = lg[i * bp + k];
    __syncthreads();
  }
  auto L = [&](int64_t m, int64_t i) -> double { return in_lds ? s_l[m * (m + 1) / 2 + i] : lg[m * bp + i]; };
  const int64_t j = tid;
  if (j < B) {
    // Phi[i,j], i >= j
    for (int64_t i = 0; i < j; ++i) y[i * B + j] = 0.0;
    for (int64_t i = j; i < B; ++i) {
      double acc = 0.0;
      for (int64_t m = i; m < B; ++m) acc = fma(L(m, i), g[m * B + j], acc);
      y[i * B + j] = i == j ? 0.5 * acc : acc;
    }
    // L^T Y = Phi, column j, in place
    for (int64_t i = B - 1; i >= 0; --i) {
      double acc = y[i * B + j];
      for (int64_t m = i + 1; m < B; ++m) acc = fma(-L(m, i), y[m * B + j], acc);
      y[i * B + j] = acc / L(i, i);
    }
  }
  __threadfence_block();
  __syncthreads();
  if (j < B) {
    // L^T W = Y^T, column j: the right-hand side is row j of Y
    for (int64_t i = B - 1; i >= 0; --i) {
      double acc = y[j * B + i];
      for (int64_t m = i + 1; m < B; ++m) acc = fma(-L(m, i), w[m * B + j], acc);
      w[i * B + j] = acc / L(i, i);
    }
  }
  __threadfence_block();
  __syncthreads();
  double part = 0.0;
  if (j < B) {
    const double* cv = cov + c * B * B;
    double* go = gcov + c * B * B;
    for (int64_t i = 0; i < B; ++i) {
      const double gs = 0.5 * (w[i * B + j] + w[j * B + i]);
      go[i * B + j] = scale * gs;
      part = fma(gs, cv[i * B + j], part);
    }
  }
  s_red[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  if (tid == 0) gscale_part[c] = s_red[0];
}

// info[C] (per class) -> info[C] = the first non-zero one
__global__ void first_info_kernel(int* info, int C) {
  int v = 0;
  for (int c = 0; c < C && v == 0; ++c) v = info[c];
  info[C] = v;
}

struct HeadOut {
  double* scal;   // device: [0] ll, [1] gscale, [2] dfterm
  int* info;      // device: one int, 0 or the first bad pivot of the first class that is not positive definite
};

bool rng_range_ok(int64_t point0, int64_t npoints, int64_t S) {
  return point0 >= 0 && npoints > 0 && npoints <= 0x7fffffff && point0 + npoints <= ((int64_t)1 << 32) && S > 0 &&
         S <= ((int64_t)1 << 32);
}

int factor_one(smn_ctx* ctx, double* lp, int64_t np, int64_t n, double jitter_abs, double ridge_rel, double* logdet_out,
               int* info_out) {
  SMN_TRY(cholesky_padded(ctx, FactorCall{SMN_F64, lp, np, np, np, n, jitter_abs, ridge_rel, true}));
  hipLaunchKernelGGL(collect_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->d_scal, ctx->d_info, lp, np, n, logdet_out, info_out);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

// The head on the context's stream, no synchronisation: mean [C,B], cov [C,B,B], gmean [C,B], gcov [C,B,B] fp64 device.
template <typename T>
int head_run(smn_ctx* ctx, const double* mean, const double* cov, const int* labels_h, int64_t B, int C, int64_t S, double df,
             double scale, uint64_t seed, int64_t point0, const void* noise, const void* dnoise, double* gmean, double* gcov,
             HeadOut* out) {
  const bool student = df > 0.0;
  const int64_t bp = round_up(B, kTile);
  const size_t ncbs = (size_t)C * (size_t)B * (size_t)S, ncbb = (size_t)C * (size_t)B * (size_t)B;
  const size_t nd = ncbs * (student ? 4 : 2) + (size_t)C * (size_t)bp * (size_t)bp + 3 * ncbb + 2 * (size_t)B * (size_t)S +
                    (size_t)C + 8;
  void* wv = nullptr;
  SMN_TRY(smn_workspace(ctx, 11, sizeof(double) * nd + sizeof(int) * ((size_t)B + (size_t)C + 2), &wv));
  double* xi = static_cast<double*>(wv);
  double* f = xi + ncbs;
  double* dxi = student ? f + ncbs : nullptr;
  double* h = student ? dxi + ncbs : nullptr;
  double* lp = f + ncbs * (student ? 3 : 1);
  double* gl = lp + (size_t)C * (size_t)bp * (size_t)bp;
  double* ybuf = gl + ncbb;
  double* wbuf = ybuf + ncbb;
  double* llpart = wbuf + ncbb;
  double* dfpart = llpart + (size_t)B * (size_t)S;
  double* gsp = dfpart + (size_t)B * (size_t)S;
  double* scal = gsp + C;
  int* labels = reinterpret_cast<int*>(scal + 8);
  int* info = labels + B;
  hipStream_t st = ctx->stream;
  SMN_HIP(ctx, hipMemcpyAsync(labels, labels_h, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, st));
  SMN_HIP(ctx, hipMemsetAsync(scal, 0, sizeof(double) * 8, st));
  // variates [C,B,S]: the generator's (point, class, draw) order written class-major, or the caller's arrays widened
  if (noise) {
    const unsigned gb = (unsigned)((ncbs + 255) / 256);
    hipLaunchKernelGGL(widen_kernel<T>, dim3(gb), dim3(256), 0, st, static_cast<const T*>(noise), (int64_t)ncbs, xi);
    if (student) {
      if (dnoise) hipLaunchKernelGGL(widen_kernel<T>, dim3(gb), dim3(256), 0, st, static_cast<const T*>(dnoise), (int64_t)ncbs, dxi);
      else SMN_HIP(ctx, hipMemsetAsync(dxi, 0, sizeof(double) * ncbs, st));
    }
  } else {
    hipLaunchKernelGGL((variates_kernel<T, double>), dim3((unsigned)B, (unsigned)((C + 3) / 4)), dim3(256), 0, st, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (T)(student ? df : 0.0), (uint32_t)point0, C, S, S, B * S, xi, dxi);
  }
  SMN_CHECK_LAUNCH(ctx);
  // L_c = chol(scale cov[c])
  hipLaunchKernelGGL(pack_lower_kernel, dim3((unsigned)((bp + 255) / 256), (unsigned)bp, (unsigned)C), dim3(256), 0, st, cov, B,
                     B * B, B, bp, scale, lp);
  SMN_CHECK_LAUNCH(ctx);
  for (int c = 0; c < C; ++c) SMN_TRY(factor_one(ctx, lp + (size_t)c * bp * bp, bp, B, 0.0, 0.0, nullptr, info + c));
  hipLaunchKernelGGL(first_info_kernel, dim3(1), dim3(1), 0, st, info, C);
  SMN_CHECK_LAUNCH(ctx);
  // forward
  const unsigned gs = (unsigned)((S + 255) / 256);
  hipLaunchKernelGGL(sample_kernel, dim3(gs, (unsigned)B, (unsigned)C), dim3(256), 0, st, mean, lp, bp, xi, dxi, B, S, f, h);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(softmax_kernel<T>, dim3(gs, (unsigned)B), dim3(256), 0, st, f, h, labels, C, B, S, llpart,
                     student ? dfpart : nullptr);
  SMN_CHECK_LAUNCH(ctx);
  const int64_t bs = B * S;
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, llpart, bs, (int64_t)1, 1.0 / ((double)B * (double)S), scal + 0);
  if (student) hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, dfpart, bs, (int64_t)1, 1.0, scal + 2);
  SMN_CHECK_LAUNCH(ctx);
  // backward: gmean = sum_s gf, gL = gf xi^T, then through the factorisation
  hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)(C * B)), dim3(64), 0, st, f, S, gmean);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 0, 1, B, B, S, 1.0, f, S, bs, xi, S, bs, 0.0, gl, B, B * B, C));
  const size_t lds_l = sizeof(double) * (size_t)(B * (B + 1) / 2);
  const int in_lds = lds_l <= 160 * 1024 - 4096 ? 1 : 0;
  if (in_lds) SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(chol_reverse_kernel), lds_l));
  hipLaunchKernelGGL(chol_reverse_kernel, dim3((unsigned)C), dim3(256), in_lds ? lds_l : 0, st, lp, bp, gl, cov, B, scale, in_lds,
                     ybuf, wbuf, gcov, gsp);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, gsp, (int64_t)C, (int64_t)1, 1.0, scal + 1);
  SMN_CHECK_LAUNCH(ctx);
  out->scal = scal;
  out->info = info + C;
  return SMN_OK;
}

int head_check(smn_ctx* ctx, const char* who, int dtype, const int* labels_h, int64_t B, int64_t C, int64_t S, double df,
               double scale, int64_t point0) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (C <= 0 || C > kMaxC) return smn_fail(ctx, SMN_EINVAL, "%s: 1 <= C <= %d classes", who, kMaxC);
  if (!rng_range_ok(point0, B, S)) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes (point indices and draws are 32-bit counter words)", who);
  if (df != df || !(scale > 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: df is NaN or scale is not > 0", who);
  if (B > kMaxB) return smn_fail(ctx, SMN_ENOTSUP, "%s: batch of %lld > %d (SMN_SVSP_MAX_BATCH)", who, (long long)B, kMaxB);
  for (int64_t i = 0; i < B; ++i)
    if (labels_h[i] < 0 || labels_h[i] >= C)
      return smn_fail(ctx, SMN_EINVAL, "%s: label %d of point %lld is outside [0, %lld)", who, labels_h[i], (long long)i, (long long)C);
  return SMN_OK;
}

// ---------------------------------------------------------------- the reverse pass through the sparse-posterior algebra
// aq[c,b,i] = A[b,i] q_var[c,i]
__global__ void __launch_bounds__(256) scale_cols_kernel(const double* __restrict__ a, const double* __restrict__ q_var, int64_t B,
                                                         int64_t I, double* __restrict__ aq) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, c = blockIdx.z;
  if (i < I) aq[(c * B + b) * I + i] = a[b * I + i] * q_var[c * I + i];
}

// dst[z][r, :cols] = src[r, :cols] for every z < gridDim.z (the B_B term of every class's covariance)
__global__ void __launch_bounds__(256) bcast_kernel(const double* __restrict__ src, int64_t lds, int64_t rows, int64_t cols,
                                                    double* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, z = blockIdx.z;
  if (j < cols) dst[(z * rows + i) * cols + j] = src[i * lds + j];
}

// One thread per inducing point i (sums over classes and batch points in index order):
//   g_q_var[c,i] = sum_b A[b,i] T1[c,b,i] + (Kinv_ii - 1 / q_var[c,i]) / (2N)        (T1[c] = gcov[c] A)
//   g_q_mu[c,i]  = gm_a[c,i] + s kq[c,i] / N                                        (gm_a = gmean A, kq = q_mu Kinv)
//   gA[b,i]      = gA0[b,i] + 2 sum_c T1[c,b,i] q_var[c,i]                          (gA0 = gmean^T q_mu, updated in place)
//   parts[i]     = (sum_c log q_var, sum_c Kinv_ii q_var, sum_c q_mu kq, K_ZZ[i,i])
__global__ void __launch_bounds__(256) per_inducing_kernel(const double* __restrict__ a, const double* __restrict__ t1,
                                                           const double* __restrict__ kinv, const double* __restrict__ q_mu,
                                                           const double* __restrict__ q_var, const double* __restrict__ kq,
                                                           const double* __restrict__ k, int64_t ldk, int64_t I, int64_t B, int C,
                                                           double s, double n_train, double* __restrict__ g_q_mu,
                                                           double* __restrict__ g_q_var, double* __restrict__ ga,
                                                           double* __restrict__ parts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= I) return;
  const double kd = kinv[i * I + i];
  double slog = 0.0, strq = 0.0, squad = 0.0;
  for (int c = 0; c < C; ++c) {
    const double qv = q_var[c * I + i];
    double d = 0.0;
    for (int64_t b = 0; b < B; ++b) d = fma(a[b * I + i], t1[(c * B + b) * I + i], d);
    g_q_var[c * I + i] = d + (kd - 1.0 / qv) / (2.0 * n_train);
    g_q_mu[c * I + i] += s * kq[c * I + i] / n_train;
    slog += log(qv);
    strq = fma(kd, qv, strq);
    squad = fma(q_mu[c * I + i], kq[c * I + i], squad);
  }
  for (int64_t b = 0; b < B; ++b) {
    double d = 0.0;
    for (int c = 0; c < C; ++c) d = fma(t1[(c * B + b) * I + i], q_var[c * I + i], d);
    ga[b * I + i] = fma(2.0, d, ga[b * I + i]);
  }
  parts[i] = slog;
  parts[I + i] = strq;
  parts[2 * I + i] = squad;
  parts[3 * I + i] = k[i * ldk + i];
}

// gbb[i,j] = sum_c gcov[c][i,j]
__global__ void __launch_bounds__(256) class_sum_kernel(const double* __restrict__ gcov, int64_t n, int C, double* __restrict__ gbb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double d = 0.0;
  for (int c = 0; c < C; ++c) d += gcov[c * n + i];
  gbb[i] = d;
}

// gKinv = sym(m) + (diag(sum_c q_var) + s qq) / (2N), in place in m (m = K_Zx gA, qq = q_mu^T q_mu); one thread per pair i >= j
__global__ void __launch_bounds__(256) gkinv_kernel(double* __restrict__ m, const double* __restrict__ qq,
                                                    const double* __restrict__ q_var, int64_t I, int C, double s, double n_train) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j > i || j >= I) return;
  double v = 0.5 * (m[i * I + j] + m[j * I + i]) + s * qq[i * I + j] / (2.0 * n_train);
  if (i == j) {
    double d = 0.0;
    for (int c = 0; c < C; ++c) d += q_var[c * I + i];
    v += d / (2.0 * n_train);
  }
  m[i * I + j] = v;
  m[j * I + i] = v;
}

// Gbar [U,U], symmetric, both triangles:
//   ZZ: sym(gK_abs + gK_rel) + (eps / I) tr(gK_rel) I + C K_ZZ^-1 / (2N)      xx: sym(gBB)
//   xZ and its mirror: (gA Kinv - 2 gBB P^T) / 2 each  (gxz [B,I] = the total derivative with respect to the K_xZ block)
// tr[0] = tr(gK_abs), tr[1] = tr(gK_rel)
__global__ void __launch_bounds__(256) gbar_kernel(const double* __restrict__ gk_abs, const double* __restrict__ gk_rel,
                                                   const double* __restrict__ kzz_inv, const double* __restrict__ gbb,
                                                   const double* __restrict__ gxz, const double* __restrict__ tr, int64_t I,
                                                   int64_t B, int C, double eps, double n_train, double* __restrict__ gbar,
                                                   int64_t ldg) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j > i) return;
  double v;
  if (i < I) {
    v = 0.5 * ((gk_abs[i * I + j] + gk_abs[j * I + i]) + (gk_rel[i * I + j] + gk_rel[j * I + i])) +
        (double)C * 0.5 * (kzz_inv[i * I + j] + kzz_inv[j * I + i]) / (2.0 * n_train);
    if (i == j) v += eps / (double)I * tr[1];
  } else if (j < I) {
    v = 0.5 * gxz[(i - I) * I + j];
  } else {
    v = 0.5 * (gbb[(i - I) * B + (j - I)] + gbb[(j - I) * B + (i - I)]);
  }
  gbar[i * ldg + j] = v;
  gbar[j * ldg + i] = v;
}

// res[0] = -ll, [1] = kl / N (without the prior's closed-form terms), [2] = g eps, [3] = gscale, [4] = g s, [5] = dfterm,
// [6] = info (as a double)
__global__ void elbo_scalars_kernel(const double* __restrict__ head, const int* __restrict__ head_info,
                                    const double* __restrict__ sums, const double* __restrict__ tr,
                                    const double* __restrict__ logdet0, const int* __restrict__ infos, int64_t I, int C, double s,
                                    double n_train, double* __restrict__ res) {
  // sums: [0] sum log q_var, [1] sum Kinv_ii q_var, [2] quad, [3] tr K_ZZ
  const double kl = 0.5 * ((double)C * logdet0[0] - sums[0] - (double)I * (double)C + sums[1] + s * sums[2]);
  res[0] = -head[0];
  res[1] = kl / n_train;
  res[2] = tr[0] + sums[3] / (double)I * tr[1];
  res[3] = head[1];
  res[4] = 0.5 * sums[2] / n_train;
  res[5] = head[2];
  int info = 0;
  for (int k = 0; k < 3 && info == 0; ++k) info = infos[k];
  if (info == 0) info = head_info[0];
  res[6] = (double)info;
}

// inv [n,n] <- (L L^T)^-1 from the padded factor lp (ld = np): two triangular sweeps over an identity
int inverse_from_factor(smn_ctx* ctx, const double* lp, int64_t np, int64_t n, double* inv) {
  hipLaunchKernelGGL(identity_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, ctx->stream, inv, n);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_trsm(ctx, SMN_F64, lp, n, np, inv, n, n, 0));
  return smn_trsm(ctx, SMN_F64, lp, n, np, inv, n, n, 1);
}

template <typename T>
int elbo_t(smn_ctx* ctx, const double* k, int64_t ldk, int64_t I, int64_t B, int C, const double* q_mu, const double* q_var,
           double eps, double s, double n_train, const int* labels_h, int64_t S, double df, double scale, uint64_t seed,
           int64_t point0, const void* noise, const void* dnoise, double* g_q_mu, double* g_q_var, double* gbar, int64_t ldg,
           double res_h[7]) {
  const int64_t ip = round_up(I, kTile);
  const size_t nii = (size_t)I * I, nib = (size_t)I * B, nbb = (size_t)B * B, nci = (size_t)C * I;
  const size_t nd = (size_t)ip * ip + 6 * nii + 5 * nib + 2 * nbb + 2 * (size_t)C * nib + 2 * (size_t)C * nbb + (size_t)C * B * 2 +
                    2 * nci + 4 * (size_t)I + 32;
  void* wv = nullptr;
  SMN_TRY(smn_workspace(ctx, 10, sizeof(double) * nd + sizeof(int) * 8, &wv));
  double* p = static_cast<double*>(wv);
  auto take = [&](size_t n) { double* r = p; p += n; return r; };
  double* lp = take((size_t)ip * ip);     // the padded factor, reused by the three factorisations
  double* kzz_inv = take(nii);            // K_ZZ^-1 (no jitter)
  double* kinv = take(nii);               // K_abs^-1
  double* krel_inv = take(nii);           // K_rel^-1
  double* m1 = take(nii);                 // K_Zx gA -> gKinv
  double* m2 = take(nii);                 // q_mu^T q_mu -> Kinv gKinv -> P gBB P^T
  double* gk_abs = take(nii);
  double* a = take(nib);                  // A [B,I]
  double* pm = take(nib);                 // P [I,B]
  double* ga = take(nib);                 // gA [B,I]
  double* t2 = take(nib);                 // P gBB [I,B]
  double* gxz = take(nib);                // [B,I]
  double* bb = take(nbb);
  double* gbb = take(nbb);
  double* aq = take((size_t)C * nib);     // A diag(q_var[c]) [C,B,I]
  double* t1 = take((size_t)C * nib);     // gcov[c] A [C,B,I]
  double* cov = take((size_t)C * nbb);
  double* gcov = take((size_t)C * nbb);
  double* mean = take((size_t)C * B);
  double* gmean = take((size_t)C * B);
  double* kq = take(nci);                 // q_mu Kinv [C,I]
  double* parts = take(4 * (size_t)I);
  double* sums = take(4);
  double* tr = take(2);
  double* logdets = take(3);
  double* res = take(8);
  int* infos = reinterpret_cast<int*>(take(4));
  hipStream_t st = ctx->stream;
  const double* kzx = k + I;              // K_Zx [I,B], ld = ldk
  const double* kxx = k + I * ldk + I;    // K_xx [B,B], ld = ldk
  const dim3 gpack((unsigned)((ip + 255) / 256), (unsigned)ip, 1);
  // K_ZZ without jitter (its log-determinant, priors.py:37), K_abs = K_ZZ + eps I, K_rel = K_ZZ + eps tr(K_ZZ) / I I
  const double jit[3] = {0.0, eps, 0.0}, rel[3] = {0.0, 0.0, eps};
  double* inv_of[3] = {kzz_inv, kinv, krel_inv};
  for (int t = 0; t < 3; ++t) {
    hipLaunchKernelGGL(pack_lower_kernel, gpack, dim3(256), 0, st, k, ldk, (int64_t)0, I, ip, 1.0, lp);
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(factor_one(ctx, lp, ip, I, jit[t], rel[t], logdets + t, infos + t));
    SMN_TRY(inverse_from_factor(ctx, lp, ip, I, inv_of[t]));
  }
  // forward: A = K_xZ Kinv, P = K_rel^-1 K_Zx, BB = K_xx - K_xZ P, mean = q_mu A^T, cov[c] = A diag(q_var[c]) A^T + BB
  SMN_TRY(gemm(ctx, 1, 0, B, I, I, 1.0, kzx, ldk, 0, kinv, I, 0, 0.0, a, I, 0));
  SMN_TRY(gemm(ctx, 0, 0, I, B, I, 1.0, krel_inv, I, 0, kzx, ldk, 0, 0.0, pm, B, 0));
  hipLaunchKernelGGL(bcast_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)B, 1), dim3(256), 0, st, kxx, ldk, B, B, bb);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 1, 0, B, B, I, -1.0, kzx, ldk, 0, pm, B, 0, 1.0, bb, B, 0));
  SMN_TRY(gemm(ctx, 0, 1, C, B, I, 1.0, q_mu, I, 0, a, I, 0, 0.0, mean, B, 0));
  hipLaunchKernelGGL(scale_cols_kernel, dim3((unsigned)((I + 255) / 256), (unsigned)B, (unsigned)C), dim3(256), 0, st, a, q_var, B, I, aq);
  hipLaunchKernelGGL(bcast_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)B, (unsigned)C), dim3(256), 0, st, bb, B, B, B, cov);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 0, 1, B, B, I, 1.0, aq, I, (int64_t)nib, a, I, 0, 1.0, cov, B, (int64_t)nbb, C));
  HeadOut ho{};
  SMN_TRY((head_run<T>(ctx, mean, cov, labels_h, B, C, S, df, scale, seed, point0, noise, dnoise, gmean, gcov, &ho)));
  // backward
  SMN_TRY(gemm(ctx, 0, 0, C, I, I, 1.0, q_mu, I, 0, kinv, I, 0, 0.0, kq, I, 0));                       // kq = q_mu Kinv
  SMN_TRY(gemm(ctx, 0, 0, C, I, B, 1.0, gmean, B, 0, a, I, 0, 0.0, g_q_mu, I, 0));                     // gmean A
  SMN_TRY(gemm(ctx, 0, 0, B, I, B, 1.0, gcov, B, (int64_t)nbb, a, I, 0, 0.0, t1, I, (int64_t)nib, C)); // T1[c] = gcov[c] A
  SMN_TRY(gemm(ctx, 1, 0, B, I, C, 1.0, gmean, B, 0, q_mu, I, 0, 0.0, ga, I, 0));                      // gmean^T q_mu
  hipLaunchKernelGGL(per_inducing_kernel, dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st, a, t1, kinv, q_mu, q_var, kq, k, ldk,
                     I, B, C, s, n_train, g_q_mu, g_q_var, ga, parts);
  SMN_CHECK_LAUNCH(ctx);
  for (int t = 0; t < 4; ++t)
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, parts + (size_t)t * I, I, (int64_t)1, 1.0, sums + t);
  hipLaunchKernelGGL(class_sum_kernel, dim3((unsigned)((nbb + 255) / 256)), dim3(256), 0, st, gcov, (int64_t)nbb, C, gbb);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 0, 0, I, I, B, 1.0, kzx, ldk, 0, ga, I, 0, 0.0, m1, I, 0));                        // K_Zx gA
  SMN_TRY(gemm(ctx, 1, 0, I, I, C, 1.0, q_mu, I, 0, q_mu, I, 0, 0.0, m2, I, 0));                       // q_mu^T q_mu
  hipLaunchKernelGGL(gkinv_kernel, dim3((unsigned)((I + 255) / 256), (unsigned)I), dim3(256), 0, st, m1, m2, q_var, I, C, s, n_train);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 0, 0, I, I, I, 1.0, kinv, I, 0, m1, I, 0, 0.0, m2, I, 0));                         // Kinv gKinv
  SMN_TRY(gemm(ctx, 0, 0, I, I, I, -1.0, m2, I, 0, kinv, I, 0, 0.0, gk_abs, I, 0));                    // gK_abs
  SMN_TRY(gemm(ctx, 0, 0, I, B, B, 1.0, pm, B, 0, gbb, B, 0, 0.0, t2, B, 0));                          // P gBB
  SMN_TRY(gemm(ctx, 0, 1, I, I, B, 1.0, t2, B, 0, pm, B, 0, 0.0, m2, I, 0));                           // gK_rel = P gBB P^T
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, gk_abs, I, I + 1, 1.0, tr + 0);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, m2, I, I + 1, 1.0, tr + 1);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gemm(ctx, 0, 0, B, I, I, 1.0, ga, I, 0, kinv, I, 0, 0.0, gxz, I, 0));                        // gA Kinv
  SMN_TRY(gemm(ctx, 0, 1, B, I, B, -2.0, gbb, B, 0, pm, B, 0, 1.0, gxz, I, 0));                        // - 2 gBB P^T
  const int64_t U = I + B;
  hipLaunchKernelGGL(gbar_kernel, dim3((unsigned)((U + 255) / 256), (unsigned)U), dim3(256), 0, st, gk_abs, m2, kzz_inv, gbb, gxz, tr,
                     I, B, C, eps, n_train, gbar, ldg);
  hipLaunchKernelGGL(elbo_scalars_kernel, dim3(1), dim3(1), 0, st, ho.scal, ho.info, sums, tr, logdets, infos, I, C, s, n_train, res);
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipMemcpyAsync(res_h, res, sizeof(double) * 7, hipMemcpyDeviceToHost, st));
  SMN_HIP(ctx, hipStreamSynchronize(st));   // the one synchronisation of the call (labels_h is borrowed until here)
  if (res_h[6] != 0.0) {
    // not positive definite somewhere: every dependent output is NaN (all-ones bytes are a quiet NaN)
    SMN_HIP(ctx, hipMemsetAsync(g_q_mu, 0xFF, sizeof(double) * nci, st));
    SMN_HIP(ctx, hipMemsetAsync(g_q_var, 0xFF, sizeof(double) * nci, st));
    SMN_HIP(ctx, hipMemset2DAsync(gbar, sizeof(double) * (size_t)ldg, 0xFF, sizeof(double) * (size_t)U, (size_t)U, st));
    for (int t = 0; t < 6; ++t) res_h[t] = std::nan("");
  }
  return SMN_OK;
}

}  // namespace

extern "C" int smn_rng_variates_ddf(smn_ctx* ctx, int dtype, uint64_t seed, double df, int64_t point0, int64_t npoints, int64_t C,
                                    int64_t S, void* out_d, void* dout_d) {
  if (!ctx || !out_d || !dout_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (C <= 0 || C > kMaxC) return smn_fail(ctx, SMN_EINVAL, "smn_rng_variates_ddf: 1 <= C <= %d classes", kMaxC);
  if (!rng_range_ok(point0, npoints, S) || df != df)
    return smn_fail(ctx, SMN_EINVAL, "smn_rng_variates_ddf: bad sizes (point indices and draws are 32-bit counter words)");
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const dim3 grid((unsigned)npoints, (unsigned)((C + 3) / 4));
  const double dfe = df > 0.0 ? df : 0.0;
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL((variates_kernel<T, T>), grid, dim3(256), 0, ctx->stream, k0, k1, (T)dfe, (uint32_t)point0, (int)C, S,
                       C * S, S, static_cast<T*>(out_d), static_cast<T*>(dout_d));
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

extern "C" int smn_svsp_head_grad(smn_ctx* ctx, int dtype, const void* mean_d, const void* cov_d, const int* labels_h, int64_t B,
                                  int64_t C, int64_t S, double df, double scale, uint64_t seed, int64_t point0,
                                  const void* noise_d, const void* dnoise_d, double* ll_h, void* gmean_d, void* gcov_d,
                                  double* gscale_h, double* dfterm_h, int* info_h) {
  if (!ctx || !mean_d || !cov_d || !labels_h || !gmean_d || !gcov_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(head_check(ctx, "smn_svsp_head_grad", dtype, labels_h, B, C, S, df, scale, point0));
  if (dnoise_d && !noise_d) return smn_fail(ctx, SMN_EINVAL, "smn_svsp_head_grad: dnoise_d without noise_d");
  const double* mean = static_cast<const double*>(mean_d);
  const double* cov = static_cast<const double*>(cov_d);
  double* gmean = static_cast<double*>(gmean_d);
  double* gcov = static_cast<double*>(gcov_d);
  HeadOut ho{};
  SMN_TRY(by_dtype(dtype, [&](auto e) {
    return head_run<decltype(e)>(ctx, mean, cov, labels_h, B, (int)C, S, df, scale, seed, point0, noise_d, dnoise_d, gmean, gcov, &ho);
  }));
  double s[3];
  int info = 0;
  SMN_HIP(ctx, hipMemcpyAsync(s, ho.scal, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipMemcpyAsync(&info, ho.info, sizeof info, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (info != 0) {
    SMN_HIP(ctx, hipMemsetAsync(gmean, 0xFF, sizeof(double) * (size_t)(C * B), ctx->stream));
    SMN_HIP(ctx, hipMemsetAsync(gcov, 0xFF, sizeof(double) * (size_t)(C * B * B), ctx->stream));
    s[0] = s[1] = s[2] = std::nan("");
  }
  if (ll_h) *ll_h = s[0];
  if (gscale_h) *gscale_h = s[1];
  if (dfterm_h) *dfterm_h = s[2];
  if (info_h) *info_h = info;
  return SMN_OK;
}

extern "C" int smn_svsp_elbo_grad(smn_ctx* ctx, int dtype, const void* k_d, int64_t ldk, int64_t I, int64_t B, int64_t C,
                                  const void* q_mu_d, const void* q_var_d, double eps, double s, double num_train,
                                  const int* labels_h, int64_t S, double df, double scale, uint64_t seed, int64_t point0,
                                  const void* noise_d, const void* dnoise_d, double* nll_h, double* kl_n_h, void* g_q_mu_d,
                                  void* g_q_var_d, double* g_eps_h, double* gscale_h, double* g_s_h, double* dfterm_h, void* gbar_d,
                                  int64_t ldg, int* info_h) {
  if (!ctx || !k_d || !q_mu_d || !q_var_d || !labels_h || !g_q_mu_d || !g_q_var_d || !gbar_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(head_check(ctx, "smn_svsp_elbo_grad", dtype, labels_h, B, C, S, df, scale, point0));
  if (I <= 0 || I + B > 65535 || !(eps >= 0.0) || !(num_train > 0.0) || !(s > 0.0))
    return smn_fail(ctx, SMN_EINVAL, "smn_svsp_elbo_grad: bad sizes (at most 65535 inducing points), eps < 0, or num_train, s not > 0");
  SMN_CHECK_LD(ctx, "smn_svsp_elbo_grad", ldk, I + B);
  SMN_CHECK_LD(ctx, "smn_svsp_elbo_grad", ldg, I + B);
  if (dnoise_d && !noise_d) return smn_fail(ctx, SMN_EINVAL, "smn_svsp_elbo_grad: dnoise_d without noise_d");
  double res[7] = {};
  const double* k = static_cast<const double*>(k_d);
  const double* qm = static_cast<const double*>(q_mu_d);
  const double* qv = static_cast<const double*>(q_var_d);
  double* gqm = static_cast<double*>(g_q_mu_d);
  double* gqv = static_cast<double*>(g_q_var_d);
  double* gbar = static_cast<double*>(gbar_d);
  SMN_TRY(by_dtype(dtype, [&](auto e) {
    return elbo_t<decltype(e)>(ctx, k, ldk, I, B, (int)C, qm, qv, eps, s, num_train, labels_h, S, df, scale, seed, point0, noise_d,
                               dnoise_d, gqm, gqv, gbar, ldg, res);
  }));
  if (nll_h) *nll_h = res[0];
  if (kl_n_h) *kl_n_h = res[1];
  if (g_eps_h) *g_eps_h = res[2];
  if (gscale_h) *gscale_h = res[3];
  if (g_s_h) *g_s_h = res[4];
  if (dfterm_h) *dfterm_h = res[5];
  if (info_h) *info_h = (int)res[6];
  return SMN_OK;
}
