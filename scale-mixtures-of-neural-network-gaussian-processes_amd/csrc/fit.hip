// fit.hip — fit once, predict many: a device-resident posterior (smn_fit_*).
//
// Every other predictive entry factors the joint kernel of [x_train; x_test] from scratch.  A state keeps what does not
// depend on the test points -- the Cholesky factor L of K~ = K_dd + (ridge_abs + ridge_rel tr(K_dd) / n) I and beta^T =
// Y^T L^-T -- and answers a prediction call with the cross kernel, one triangular solve and one read-out pass:
//
//        [ L             .            .  ]   rows 0 .. n_pad              (factor, identity padding)
//   A =  [ K_td -> V^T   K_tt -> S    .  ]   rows n_pad .. + cap_pad      (one chunk of test rows; cap_pad = round_up(capacity, 128))
//        [ beta^T        0            0  ]   rows n_pad + cap_pad .. +128 (c <= 48 of them used)
//
//   V^T = K_td L^-T (solve_rows_padded on the chunk's tile rows only), mean = V^T beta, var = k_tt - |V_r|^2,
//   S = K_tt - V^T V (schur_rows_padded, the factorisation's far update) when the full covariance is asked for.
//
// beta^T sits in a tile row of its own BEHIND the test rows: the solve and the Schur update work on whole 128-row tiles of
// [n_pad, n_pad + round_up(rows, 128)), and a right-hand-side row sharing a tile with test rows would be solved a second time.
// The matrix is therefore [n_pad + cap_pad + 128]^2, at most one tile row more than [n_pad + round_up(capacity + c, 128)]^2.
// The state owns A and (fused form) its padded copy of x with the row norms q; the context's workspace slots are used only
// inside a call (padded test chunk: slot 0, layer tables: slot 1, factored diagonal blocks: slot 3), so a state survives any
// other call on its context.  No prediction entry changes what another reads; the first smn_fit_predict_grad call adds what the
// gradients alone read (below) beside it.
//
// Appending training points (smn_fit_append, smn_fit_append_from_kernel, smn_fit_reserve; include/smnngp.h has the algebra and
// the frozen-ridge rule).  The k new rows take the place of the identity padding behind row n -- a state has room for n_pad
// rows and grows by reallocation when that is not enough.  A chunk of r <= capacity rows is a cov = full prediction of those
// rows (cross build, K(x+, x+) into the trailing block, solve_rows_padded, schur_rows_padded), then one splice pass over the
// solved rows (V_i into row n + i of L, the residuals y+ - V beta transposed into the tile row behind the window: the test rows'
// next tile row, or the beta rows' columns behind n_pad when r fills the capacity), then cholesky_padded on the trailing window
// [n_pad, n_pad + round_up(r, 128)) with those residual rows as its appended rows -- which leaves L22 in the window, z^T in the
// residual rows, |z_c|^2 on the Schur diagonal and log det S in the scalars, as at creation.  Only when S was positive definite
// are L22 and z copied next to L and beta and n moved; otherwise rows [n, n + r) of L are made identity padding again (they
// held zeros and a one: the state is bit for bit what it was).  Either way the window, its residual rows and the beta rows'
// tail are cleared.
//
// Removing training points (smn_fit_remove) is fit_remove.hip; the state's layout is fit_state.hpp.  A removal restores what the
// entries here rely on: identity padding behind row n, and zeros in columns [n, n_pad) of the beta rows and of the test rows (a
// chunk's cross kernel is written in columns [0, n) only, while the solve and the read-out run over the whole padded row).
//
// Predictive gradients (smn_fit_predict_grad; the kernel-side derivative is input_grad.hip).  With alpha = K~^-1 Y = L^-T beta and
// U = K_td K~^-1 = V^T L^-1:
//     dmean[r, k, :] = (F_1 diag(alpha_k) X + 2 (F_2 alpha)[r, k] x_r) / d          (F_1, F_2 formed ONCE per chunk for all c outputs)
//     dvar[r, :]     = 2 x_r / d * dk_rr/dq0 - 2 gx(seed = U)[r, :]                 (k_rr the closed-form diagonal, K or Theta)
// Both backward substitutions run as forward sweeps on L' = J L^T J (J reverses the order; smn_trsm's trans = 1 form): the
// state keeps L' with one chunk of appended rows, alpha^T [c, n_pad] and X^T from the first gradient call on.
//
// Why trsm on L and not the explicit -K~^-1 the gradient pipeline leaves behind: k^T K~^-1 k through an explicit inverse loses
// cond(K~) u in fp32, while k_tt - |L^-1 k|^2 is a difference of two non-negative numbers each good to n u of k_tt.
//
// Read-out kernel (the hot path of a diag-only call once the cross kernel is solved): a fixed group of four waves per test
// row (a chunk of 2048 rows puts 8192 waves on the chip; one wave per row would leave it at two waves per SIMD with one load
// each in flight), 16-byte loads of the row (n_pad is a multiple of 128 elements), fp64 accumulation per lane in column order,
// the fixed xor tree over each wave, the four waves added in wave order -- the order of every sum depends on n_pad alone, not
// on the grid, the chunking or c, so repeated calls give the same bits.  The mean of c columns is taken in the same kernel,
// CB columns per pass over the row (CB = 1, 4 or 8 by c): for c = 1 -- SPR, the flagship -- the row is streamed from HBM
// exactly once.  For wide Y (c up to 48) the alternative is the NT tile engine (gemm_nt.hpp, as smn_gram uses it) for V^T beta
// with the kernel keeping only the sum of squares.  Both were timed on an MI355X in fp32 at T = 2048, c = 48
// (profiles/r18_fit_predict.txt): this kernel, six passes of eight columns, 0.301 ms at N = 16384 and 0.092 ms at N = 4096;
// the sum-of-squares pass (0.027 / 0.012 ms) plus the tile engine on [T, n_pad] x [48, n_pad] operands (1.049 / 0.273 ms of
// kernel time) 1.076 / 0.285 ms -- a 128-column tile holds 48 live columns and the launch is 16 workgroups on a 256-CU chip,
// while the extra passes here re-read a row (n_pad * es <= 64 KB) that the first pass left in L2.  So the mean stays in this
// kernel, in fp64, for every c.  Compiler figures (HIP 7.2, gfx950, -O3), VGPRs / waves per SIMD, no scratch in any form:
// f32 CB = 1: 53 / 8, CB = 4: 75 / 6, CB = 8: 107 / 4; f64 40 / 8, 50 / 8, 70 / 7.
#include <algorithm>
#include <cmath>
#include <new>

#include "fit_state.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

template <typename T>
struct Vec16;
template <>
struct Vec16<float> { using type = float4; static constexpr int N = 4; };
template <>
struct Vec16<double> { using type = double2; static constexpr int N = 2; };

// One workgroup (four waves) per solved test row r:
//   var[r] = ktt[r * ktt_stride] - sum_j v[r, j]^2,   mean[r, k] = sum_j v[r, j] beta[k, j]   (j < n_pad, k < c)
// Each lane walks the row in 16-byte pieces 256 lanes apart and adds in fp64 in that order; a wave's 64 partial sums meet in
// the xor tree and the four waves' sums are added in wave order by one thread.  Column k's sum does not depend on CB (the
// columns of a group are independent accumulators), on the grid or on which rows share a call.
template <typename T, int CB>
__global__ void __launch_bounds__(256) fit_readout_kernel(const T* __restrict__ v, int64_t lda, int64_t n_pad,
                                                          const T* __restrict__ beta, int c, const T* __restrict__ ktt,
                                                          int64_t ktt_stride, T* __restrict__ mean, T* __restrict__ var) {
  using V = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  __shared__ double red[4][CB + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const T* vr = v + row * lda;
  for (int c0 = 0; c0 < c; c0 += CB) {
    double s[CB];
#pragma unroll
    for (int e = 0; e < CB; ++e) s[e] = 0.0;
    double ss = 0.0;
#pragma unroll 2
    for (int64_t k = (int64_t)threadIdx.x * VN; k < n_pad; k += 256 * VN) {
      const V xv = *reinterpret_cast<const V*>(vr + k);
      const T* xe = reinterpret_cast<const T*>(&xv);
      if (c0 == 0) {
#pragma unroll
        for (int u = 0; u < VN; ++u) ss += (double)xe[u] * (double)xe[u];
      }
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        const int ce = c0 + e < c ? c0 + e : c - 1;
        const V bv = *reinterpret_cast<const V*>(beta + (int64_t)ce * lda + k);
        const T* be = reinterpret_cast<const T*>(&bv);
#pragma unroll
        for (int u = 0; u < VN; ++u) s[e] += (double)xe[u] * (double)be[u];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
#pragma unroll
    for (int e = 0; e < CB; ++e) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[e] += __shfl_xor(s[e], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < CB; ++e) red[wave][e] = s[e];
      red[wave][CB] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (c0 == 0 && var) var[row] = (T)((double)ktt[row * ktt_stride] - (((red[0][CB] + red[1][CB]) + red[2][CB]) + red[3][CB]));
      for (int e = 0; e < CB && c0 + e < c; ++e) mean[row * c + c0 + e] = (T)(((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
    }
    __syncthreads();   // (the next group of columns rewrites red)
  }
}

template <typename T>
__global__ void fit_nan_kernel(T* __restrict__ p, int64_t rows, int64_t cols, int64_t ld) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  for (int64_t i = blockIdx.y; i < rows; i += gridDim.y) p[i * ld + j] = (T)NAN;
}

template <typename T>
int readout_t(smn_fit* f, int64_t rows, const void* ktt, int64_t ktt_stride, void* mean, void* var) {
  smn_ctx* ctx = f->ctx;
  const T* v = reinterpret_cast<const T*>(f->at(f->n_pad, 0));
  const T* beta = reinterpret_cast<const T*>(f->at(f->beta_row(), 0));
  const dim3 g((unsigned)rows), b(256);
  ProfScope ps(ctx, PROF_MISC, ctx->stream);
#define SMN_FIT_READOUT(CB)                                                                                                  \
  hipLaunchKernelGGL((fit_readout_kernel<T, CB>), g, b, 0, ctx->stream, v, f->lda, f->n_pad, beta, (int)f->c,                 \
                     static_cast<const T*>(ktt), ktt_stride, static_cast<T*>(mean), static_cast<T*>(var))
  if (f->c == 1) SMN_FIT_READOUT(1);
  else if (f->c <= 4) SMN_FIT_READOUT(4);
  else SMN_FIT_READOUT(8);
#undef SMN_FIT_READOUT
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

int readout(smn_fit* f, int64_t rows, const void* ktt, int64_t ktt_stride, void* mean, void* var) {
  return by_dtype(f->dtype, [&](auto e) { return readout_t<decltype(e)>(f, rows, ktt, ktt_stride, mean, var); });
}

int fill_nan(smn_fit* f, void* p, int64_t rows, int64_t cols, int64_t ld) {
  if (!p || rows <= 0 || cols <= 0) return SMN_OK;
  smn_ctx* ctx = f->ctx;
  const dim3 g((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768));
  by_dtype(f->dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(fit_nan_kernel<T>, g, dim3(256), 0, ctx->stream, static_cast<T*>(p), rows, cols, ld);
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

void fit_free(smn_fit* f) {
  if (!f) return;
  if (f->a) (void)hipFree(f->a);
  if (f->xs) (void)hipFree(f->xs);
  if (f->lt) (void)hipFree(f->lt);
  if (f->alpha) (void)hipFree(f->alpha);
  if (f->xt) (void)hipFree(f->xt);
  delete f;
}

// frees a half-made state on every error return of a create entry
struct FitGuard {
  smn_fit* f;
  ~FitGuard() { fit_free(f); }
  smn_fit* release() { smn_fit* r = f; f = nullptr; return r; }
};

int fit_alloc(smn_ctx* ctx, const char* who, int dtype, int64_t n, int64_t c, int64_t capacity, int64_t d, bool fused,
              smn_fit** out) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (n <= 0 || c <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes (n = %lld, c = %lld)", who, (long long)n, (long long)c);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: c = %lld: more than 48 output columns", who, (long long)c);
  if (capacity < 1) return smn_fail(ctx, SMN_EINVAL, "%s: capacity = %lld must be at least 1", who, (long long)capacity);
  smn_fit* f = new (std::nothrow) smn_fit;
  if (!f) return smn_fail(ctx, SMN_ENOMEM, "%s: out of host memory", who);
  FitGuard guard{f};
  f->ctx = ctx; f->dtype = dtype; f->fused = fused;
  f->n = n; f->c = c; f->capacity = capacity; f->d = d;
  f->n_pad = round_up(n, kTile);
  f->cap_pad = round_up(capacity, kTile);
  f->n_total = f->n_pad + f->cap_pad + kTile;
  f->lda = f->n_total;
  const size_t abytes = f->es() * (size_t)f->n_total * (size_t)f->lda;
  SMN_HIP(ctx, hipMalloc(&f->a, abytes));
  f->bytes = abytes;
  if (fused) {
    f->kp = k_pad(dtype, d);
    const size_t xbytes = sizeof(double) * (size_t)f->n_pad + f->es() * (size_t)f->n_pad * (size_t)f->kp;
    SMN_HIP(ctx, hipMalloc(&f->xs, xbytes));
    f->bytes += xbytes;
  }
  SMN_HIP(ctx, hipMemsetAsync(f->a, 0, abytes, ctx->stream));
  *out = guard.release();
  return SMN_OK;
}

// The factorisation of the leading block with Y^T as its only appended rows (in the test rows' first tile row), the heads'
// scalars, then beta^T moved behind the test rows, whose tile rows are cleared.  prepped: aug_prep has written Y^T and shifted
// the diagonal already.
int fit_factor(smn_fit* f, const void* y_d, bool prepped, double ridge_rel, double ridge_abs, double* quad_h, double* logdet_h,
               int* info_h) {
  smn_ctx* ctx = f->ctx;
  if (!prepped) SMN_TRY(set_aug_rows(ctx, f->dtype, f->a, f->lda, f->n_pad, f->n_pad + kTile, y_d, f->n, f->c, f->c));
  FactorCall fc{f->dtype, f->a, f->n_pad + kTile, f->n_pad, f->lda, f->n, ridge_abs, ridge_rel, true};
  fc.prepped = prepped;
  SMN_TRY(cholesky_padded(ctx, fc));
  SMN_TRY(extract_posterior(ctx, f->dtype, f->a, f->lda, f->n_pad, 0, f->c, nullptr, nullptr, 0, ctx->d_scal + 8, true));
  HeadScalars h;
  SMN_TRY(fetch_mail(ctx, (int)f->c, &h));
  f->info = h.info;
  publish_head(h, f->c, true, f->n, 0.0, 1.0, nullptr, nullptr, quad_h, logdet_h, info_h);   // (the per-column forms only)
  for (int64_t k = 0; k < f->c; ++k) f->quad[k] = h.quad[k];
  f->logdet = h.logdet;
  f->ridge = ridge_abs;
  if (ridge_rel != 0.0) {   // the shift the device applied, from the trace it read (diag_shift_kernel's expression)
    double trace = 0.0;
    SMN_HIP(ctx, hipMemcpy(&trace, ctx->d_scal + 1, sizeof(double), hipMemcpyDeviceToHost));
    f->ridge = ridge_abs + ridge_rel * trace / (double)f->n;
  }
  // (columns [0, n_pad) only: what lies behind them is the creation-time Schur block -beta beta^T, which stays out of the beta rows)
  const size_t pitch = f->es() * (size_t)f->lda;
  SMN_HIP(ctx, hipMemcpy2DAsync(f->at(f->beta_row(), 0), pitch, f->at(f->n_pad, 0), pitch, f->es() * (size_t)f->n_pad, (size_t)kTile,
                                hipMemcpyDeviceToDevice, ctx->stream));
  SMN_HIP(ctx, hipMemsetAsync(f->at(f->n_pad, 0), 0, f->es() * (size_t)f->cap_pad * (size_t)f->lda, ctx->stream));
  return SMN_OK;
}

// rows [r, round_up(r, 128)) of the test block: cleared, so that the tile-wise solve carries zeros and not an earlier chunk
int clear_tail_rows(smn_fit* f, int64_t r) {
  const int64_t rp = round_up(r, kTile);
  if (rp == r) return SMN_OK;
  SMN_HIP(f->ctx, hipMemsetAsync(f->at(f->n_pad + r, 0), 0, f->es() * (size_t)(rp - r) * (size_t)f->lda, f->ctx->stream));
  return SMN_OK;
}

// solved rows -> outputs of one chunk.  ktt: the chunk's prior variances (stride ktt_stride).  cov: the trailing block holds
// the lower triangle of K_tt.
int finish_chunk(smn_fit* f, int64_t r, const void* ktt, int64_t ktt_stride, void* mean, void* var, void* cov, int64_t ldcov) {
  smn_ctx* ctx = f->ctx;
  const int64_t rp = round_up(r, kTile);
  SMN_TRY(solve_rows_padded(ctx, f->dtype, f->a, f->n_pad + rp, f->n_pad, f->lda));
  SMN_TRY(readout(f, r, ktt, ktt_stride, mean, var));
  if (cov) {
    SMN_TRY(schur_rows_padded(ctx, f->dtype, f->a, f->n_pad + rp, f->n_pad, f->lda));
    SMN_TRY(extract_posterior(ctx, f->dtype, f->a, f->lda, f->n_pad, r, 0, nullptr, cov, ldcov, nullptr, false));
  }
  return SMN_OK;
}

// The build of one padded chunk of test rows (xp, q: pad_rows) against whatever second operand the caller fills in.
BuildCall chunk_build_call(const smn_fit* f, const void* xp, const double* q, int64_t rp) {
  BuildCall b{};
  b.spec = BuildSpec{f->dtype, f->net, f->act, f->num_hiddens, f->w_std, f->b_std, f->last_w_std};
  b.kp = (int)f->kp; b.d = f->d;
  b.get_mask = f->ntk ? SMN_GET_NTK : SMN_GET_NNGP;
  b.store_mode = STORE_BOUNDS;
  b.ldo = f->lda;
  b.x1p = xp; b.ld1 = f->kp; b.rows1 = rp; b.q1 = q;
  return b;
}

// the cross kernel K(x_chunk, X) straight into the appended rows
int build_cross(smn_fit* f, BuildCall b, int64_t r, BuildOut* built) {
  b.x2p = f->xp(); b.ld2 = f->kp; b.rows2 = f->n_pad; b.q2 = f->q();
  b.symmetric = 0; b.exact_diag = 0;
  b.out_rows = r; b.out_cols = f->n;
  void* dst = f->at(f->n_pad, 0);
  b.out_k = f->ntk ? nullptr : dst; b.out_t = f->ntk ? dst : nullptr;
  return run_build(f->ctx, b, built);
}

// What the gradients read beside the factor, made once: L' = J L^T J (rows below it cleared), alpha^T = (L^-T beta)^T by the
// forward sweep on L' of the reversed beta rows, and (fused states only: a matrix-form state keeps no x) X^T.
int ensure_grad_state(smn_fit* f) {
  if (f->grad_ready) return SMN_OK;
  smn_ctx* ctx = f->ctx;
  const size_t es = f->es();
  const size_t lt_bytes = es * (size_t)(f->n_pad + f->cap_pad) * (size_t)f->n_pad, al_bytes = es * (size_t)f->c * (size_t)f->n_pad,
               xt_bytes = es * (size_t)round_up(f->d, kTile) * (size_t)f->n_pad;
  if (!f->lt) { SMN_HIP(ctx, hipMalloc(&f->lt, lt_bytes)); f->bytes += lt_bytes; }
  if (!f->alpha) { SMN_HIP(ctx, hipMalloc(&f->alpha, al_bytes)); f->bytes += al_bytes; }
  if (f->fused && !f->xt) { SMN_HIP(ctx, hipMalloc(&f->xt, xt_bytes)); f->bytes += xt_bytes; }
  SMN_HIP(ctx, hipMemsetAsync(f->lt, 0, lt_bytes, ctx->stream));
  SMN_TRY(flip_transpose_lower(ctx, f->dtype, f->lt, f->n_pad, f->a, f->lda, f->n_pad));
  SMN_TRY(flip_rows(ctx, f->dtype, f->lt_at(f->n_pad), f->n_pad, f->at(f->beta_row(), 0), f->lda, f->c, f->n_pad));
  SMN_TRY(solve_rows_padded(ctx, f->dtype, f->lt, f->n_pad + kTile, f->n_pad, f->n_pad));
  SMN_TRY(flip_rows(ctx, f->dtype, f->alpha, f->n_pad, f->lt_at(f->n_pad), f->n_pad, f->c, f->n_pad));
  if (f->fused) SMN_TRY(input_grad_transpose(ctx, f->dtype, f->xp(), f->n_pad, f->kp, f->d, f->xt));
  f->grad_ready = true;
  return SMN_OK;
}

int check_outputs(smn_fit* f, const char* who, int64_t t, const void* mean_d, const void* cov_d, int64_t ldcov) {
  smn_ctx* ctx = f->ctx;
  if (!mean_d) return smn_fail(ctx, SMN_EINVAL, "%s: mean_d is NULL", who);
  if (t <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: t = %lld must be at least 1", who, (long long)t);
  if (cov_d) {
    if (t > f->capacity)
      return smn_fail(ctx, SMN_EINVAL, "%s: cov_d needs t = %lld <= capacity = %lld (the Schur block sits behind the factor)", who,
                      (long long)t, (long long)f->capacity);
    SMN_CHECK_LD(ctx, who, ldcov, t);
  }
  return SMN_OK;
}

int nan_outputs(smn_fit* f, int64_t t, void* mean_d, void* var_d, void* cov_d, int64_t ldcov) {
  SMN_TRY(fill_nan(f, mean_d, t, f->c, f->c));
  SMN_TRY(fill_nan(f, var_d, 1, t, t));
  return fill_nan(f, cov_d, t, t, ldcov);
}

// ---- appending training points (smn_fit_append / smn_fit_append_from_kernel) ----
// The splice pass of an append, one workgroup (four waves) per solved new row i -- the read-out's scheme: 16-byte loads of
// V_i = row i of the test block, fp64 sums per lane in column order, the xor tree, the four waves in wave order.  The pass that
// forms the first group of columns also stores the row, 16 bytes at a time, into row n + i of the factor (columns [0, n); the
// last piece may reach into [n, n + VN), where V is zero and the block L_22 is written afterwards).  res[k, i] = y[i, k] - V_i .
// beta_k: the sum is the read-out's mean of row i, bit for bit, before its rounding to T; the difference is rounded once.
template <typename T, int CB>
__global__ void __launch_bounds__(256) fit_splice_kernel(const T* __restrict__ v, int64_t lda, int64_t n_pad, int64_t n,
                                                         const T* __restrict__ beta, int c, const T* __restrict__ y,
                                                         T* __restrict__ lrow, T* __restrict__ res) {
  using V = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  __shared__ double red[4][CB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const T* vr = v + row * lda;
  T* lr = lrow + row * lda;
  for (int c0 = 0; c0 < c; c0 += CB) {
    double s[CB];
#pragma unroll
    for (int e = 0; e < CB; ++e) s[e] = 0.0;
#pragma unroll 2
    for (int64_t k = (int64_t)threadIdx.x * VN; k < n_pad; k += 256 * VN) {
      const V xv = *reinterpret_cast<const V*>(vr + k);
      const T* xe = reinterpret_cast<const T*>(&xv);
      if (c0 == 0 && k < n) *reinterpret_cast<V*>(lr + k) = xv;
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        const int ce = c0 + e < c ? c0 + e : c - 1;
        const V bv = *reinterpret_cast<const V*>(beta + (int64_t)ce * lda + k);
        const T* be = reinterpret_cast<const T*>(&bv);
#pragma unroll
        for (int u = 0; u < VN; ++u) s[e] += (double)xe[u] * (double)be[u];
      }
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[e] += __shfl_xor(s[e], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < CB; ++e) red[wave][e] = s[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int e = 0; e < CB && c0 + e < c; ++e)
        res[(int64_t)(c0 + e) * lda + row] = (T)((double)y[row * c + c0 + e] - (((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]));
    }
    __syncthreads();   // (the next group of columns rewrites red)
  }
}

// the splice pass over the r solved rows of the test block; y_chunk [r, c] their targets, rp = round_up(r, 128)
template <typename T>
int splice_t(smn_fit* f, int64_t r, int64_t rp, const void* y_chunk) {
  smn_ctx* ctx = f->ctx;
  const T* v = reinterpret_cast<const T*>(f->at(f->n_pad, 0));
  const T* beta = reinterpret_cast<const T*>(f->at(f->beta_row(), 0));
  T* lrow = reinterpret_cast<T*>(f->at(f->n, 0));
  T* res = reinterpret_cast<T*>(f->at(f->n_pad + rp, f->n_pad));
  const dim3 g((unsigned)r), b(256);
  ProfScope ps(ctx, PROF_MISC, ctx->stream);
#define SMN_FIT_SPLICE(CB)                                                                                                   \
  hipLaunchKernelGGL((fit_splice_kernel<T, CB>), g, b, 0, ctx->stream, v, f->lda, f->n_pad, f->n, beta, (int)f->c,            \
                     static_cast<const T*>(y_chunk), lrow, res)
  if (f->c == 1) SMN_FIT_SPLICE(1);
  else if (f->c <= 4) SMN_FIT_SPLICE(4);
  else SMN_FIT_SPLICE(8);
#undef SMN_FIT_SPLICE
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

// Room for new_pad (a multiple of 128, > n_pad) training rows: a new matrix and padded x copy, the factor's lower triangle,
// the beta rows and x copied over, identity on the new rows' diagonal, zeros elsewhere.  The old state is released only once
// the new one is complete; what the gradients read is dropped (ensure_grad_state makes it again at the new size).
int fit_grow(smn_fit* f, const char* who, int64_t new_pad) {
  smn_ctx* ctx = f->ctx;
  const size_t es = f->es();
  const int64_t nt = new_pad + f->cap_pad + kTile;
  const size_t abytes = es * (size_t)nt * (size_t)nt;
  const size_t xbytes_new = f->fused ? sizeof(double) * (size_t)new_pad + es * (size_t)new_pad * (size_t)f->kp : 0;
  const size_t xbytes_old = f->fused ? sizeof(double) * (size_t)f->n_pad + es * (size_t)f->n_pad * (size_t)f->kp : 0;
  void *na = nullptr, *nx = nullptr;
  if (hipMalloc(&na, abytes) != hipSuccess) {
    (void)hipGetLastError();
    return smn_fail(ctx, SMN_ENOMEM, "%s: no device memory for %lld training rows (%zu bytes beside the state's %zu)", who,
                    (long long)new_pad, abytes, f->bytes);
  }
  if (f->fused && hipMalloc(&nx, xbytes_new) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(na);
    return smn_fail(ctx, SMN_ENOMEM, "%s: no device memory for %lld training rows", who, (long long)new_pad);
  }
  smn_fit g = *f;   // the new layout, for the addressing helpers
  g.a = na; g.xs = nx; g.n_pad = new_pad; g.n_total = nt; g.lda = nt;
  auto fill = [&]() -> int {
    SMN_HIP(ctx, hipMemsetAsync(na, 0, abytes, ctx->stream));
    SMN_TRY(copy_matrix(ctx, f->dtype, na, nt, f->a, f->lda, f->n_pad, f->n_pad, 1));
    SMN_TRY(fill_identity_pad(ctx, f->dtype, na, nt, new_pad, f->n_pad));
    SMN_TRY(copy_matrix(ctx, f->dtype, g.at(g.beta_row(), 0), nt, f->at(f->beta_row(), 0), f->lda, f->c, f->n_pad, 0));
    if (f->fused) {
      SMN_HIP(ctx, hipMemsetAsync(nx, 0, xbytes_new, ctx->stream));
      SMN_HIP(ctx, hipMemcpyAsync(g.q(), f->q(), sizeof(double) * (size_t)f->n_pad, hipMemcpyDeviceToDevice, ctx->stream));
      SMN_HIP(ctx, hipMemcpyAsync(g.xp(), f->xp(), es * (size_t)f->n_pad * (size_t)f->kp, hipMemcpyDeviceToDevice, ctx->stream));
    }
    SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SMN_OK;
  };
  const int rc = fill();
  if (rc != SMN_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(na);
    if (nx) (void)hipFree(nx);
    return rc;
  }
  (void)hipFree(f->a);
  if (f->xs) (void)hipFree(f->xs);
  size_t gone = es * (size_t)f->n_total * (size_t)f->lda + xbytes_old;
  if (f->lt) { (void)hipFree(f->lt); gone += es * (size_t)(f->n_pad + f->cap_pad) * (size_t)f->n_pad; }
  if (f->alpha) { (void)hipFree(f->alpha); gone += es * (size_t)f->c * (size_t)f->n_pad; }
  if (f->xt) { (void)hipFree(f->xt); gone += es * (size_t)round_up(f->d, kTile) * (size_t)f->n_pad; }
  f->lt = f->alpha = f->xt = nullptr;
  f->grad_ready = false;
  f->a = na; f->xs = nx; f->n_pad = new_pad; f->n_total = nt; f->lda = nt;
  f->bytes = f->bytes - gone + abytes + xbytes_new;
  return SMN_OK;
}

// the test rows an append chunk of rp padded rows works in (its appended right-hand-side rows included), cleared
int clear_append_rows(smn_fit* f, int64_t rp) {
  const int64_t rows = std::min(rp + (int64_t)kTile, f->cap_pad);
  SMN_HIP(f->ctx, hipMemsetAsync(f->at(f->n_pad, 0), 0, f->es() * (size_t)rows * (size_t)f->lda, f->ctx->stream));
  return SMN_OK;
}

// what an append chunk left in the beta rows behind column n_pad (its right-hand sides when rp == cap_pad, their Schur block)
int clear_beta_tail(smn_fit* f) {
  const size_t pitch = f->es() * (size_t)f->lda;
  SMN_HIP(f->ctx, hipMemset2DAsync(f->at(f->beta_row(), f->n_pad), pitch, 0, f->es() * (size_t)(f->lda - f->n_pad), (size_t)kTile,
                                   f->ctx->stream));
  return SMN_OK;
}

// One chunk of r <= capacity new rows whose cross kernel K(x+, X) sits in the test rows (columns [0, n)) and whose K(x+, x+)
// (lower) sits in the trailing block: V, S, the splice pass, the factorisation of the trailing window with the residual rows
// as its appended rows, and -- only when S is positive definite -- L_22, z and the totals.  *info = 0 or the failing pivot's
// 1-based index among all training rows; the state is then as it was before the chunk.
int append_chunk(smn_fit* f, int64_t r, const void* y_chunk, int* info) {
  smn_ctx* ctx = f->ctx;
  const int64_t rp = round_up(r, kTile), n = f->n, n_pad = f->n_pad;
  const size_t pitch = f->es() * (size_t)f->lda;
  SMN_TRY(solve_rows_padded(ctx, f->dtype, f->a, n_pad + rp, n_pad, f->lda));
  SMN_TRY(schur_rows_padded(ctx, f->dtype, f->a, n_pad + rp, n_pad, f->lda));
  SMN_TRY(fill_identity_pad(ctx, f->dtype, f->at(n_pad, n_pad), f->lda, rp, r));
  SMN_TRY(by_dtype(f->dtype, [&](auto e) { return splice_t<decltype(e)>(f, r, rp, y_chunk); }));
  FactorCall fc{f->dtype, f->at(n_pad, n_pad), rp + kTile, rp, f->lda, r, f->ridge, 0.0, true};
  SMN_TRY(cholesky_padded(ctx, fc));
  SMN_TRY(extract_posterior(ctx, f->dtype, f->at(n_pad, n_pad), f->lda, rp, 0, f->c, nullptr, nullptr, 0, ctx->d_scal + 8, true));
  HeadScalars h;
  SMN_TRY(fetch_mail(ctx, (int)f->c, &h));
  if (h.info != 0) {   // rows [n, n + r) of the factor back to identity padding, bit for bit
    SMN_HIP(ctx, hipMemset2DAsync(f->at(n, 0), pitch, 0, f->es() * (size_t)n_pad, (size_t)r, ctx->stream));
    SMN_TRY(fill_identity_pad(ctx, f->dtype, f->a, f->lda, n + r, n));
    SMN_TRY(clear_append_rows(f, rp));
    SMN_TRY(clear_beta_tail(f));
    *info = (int)(n + h.info);
    return SMN_OK;
  }
  SMN_TRY(copy_matrix(ctx, f->dtype, f->at(n, n), f->lda, f->at(n_pad, n_pad), f->lda, r, r, 1));
  SMN_TRY(copy_matrix(ctx, f->dtype, f->at(f->beta_row(), n), f->lda, f->at(n_pad + rp, n_pad), f->lda, f->c, r, 0));
  SMN_TRY(clear_append_rows(f, rp));
  SMN_TRY(clear_beta_tail(f));
  f->n = n + r;
  for (int64_t k = 0; k < f->c; ++k) f->quad[k] += h.quad[k];
  f->logdet += h.logdet;
  f->grad_ready = false;
  *info = 0;
  return SMN_OK;
}

// the checks both append entries share, and the growth of a state that has no room for n + k rows: to
// round_up(max(n + k, n + n / 2), 128) rows, so that a run of small appends copies the factor O(log) times
int append_enter(smn_fit* f, const char* who, int64_t k, const void* y_new_d) {
  smn_ctx* ctx = f->ctx;
  if (k < 1) return smn_fail(ctx, SMN_EINVAL, "%s: k = %lld must be at least 1", who, (long long)k);
  if (!y_new_d) return smn_fail(ctx, SMN_EINVAL, "%s: y_new_d is NULL", who);
  if (f->info != 0)
    return smn_fail(ctx, SMN_EINVAL, "%s: the state's matrix was not positive definite (info = %d): nothing to append to", who, f->info);
  if (f->n + k > f->n_pad) SMN_TRY(fit_grow(f, who, round_up(std::max(f->n + k, f->n + f->n / 2), kTile)));
  return SMN_OK;
}

void append_publish(const smn_fit* f, int info, double* quad_h, double* logdet_h, int* info_h) {
  for (int64_t k = 0; k < f->c && quad_h; ++k) quad_h[k] = f->quad[k];
  if (logdet_h) *logdet_h = f->logdet;
  if (info_h) *info_h = info;
}

}  // namespace

extern "C" int smn_fit_create(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                              double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                              double ridge_rel, double ridge_abs, int64_t capacity, smn_fit** out, double* quad_h,
                              double* logdet_h, int* info_h) {
  if (!ctx || !x_d || !y_d || !out) return SMN_EINVAL;
  SMN_ENTER(ctx);
  *out = nullptr;
  if (d <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_fit_create: d = %lld", (long long)d);
  SMN_CHECK_LD(ctx, "smn_fit_create", ldx, d);
  bool ntk = false;
  SMN_TRY(split_net(ctx, &net, &ntk));
  smn_fit* f = nullptr;
  SMN_TRY(fit_alloc(ctx, "smn_fit_create", dtype, n, c, capacity, d, true, &f));
  FitGuard guard{f};
  f->net = net; f->act = act; f->num_hiddens = num_hiddens; f->ntk = ntk;
  f->w_std = w_std; f->b_std = b_std; f->last_w_std = last_w_std;
  SMN_TRY(pad_rows(ctx, dtype, x_d, n, ldx, d, f->xp(), f->n_pad, f->kp, f->q()));
  BuildCall b{};
  b.spec = BuildSpec{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};
  b.x1p = f->xp(); b.ld1 = f->kp; b.rows1 = f->n_pad; b.q1 = f->q();
  b.x2p = f->xp(); b.ld2 = f->kp; b.rows2 = f->n_pad; b.q2 = f->q();
  b.kp = (int)f->kp; b.d = d;
  b.symmetric = 1; b.exact_diag = 1;
  b.store_mode = STORE_PAD_IDENTITY;
  b.nv0 = n; b.aug0 = f->n_pad; b.nv1 = 0;
  b.get_mask = ntk ? SMN_GET_NTK : SMN_GET_NNGP;
  b.out_k = ntk ? nullptr : f->a; b.out_t = ntk ? f->a : nullptr; b.ldo = f->lda;
  b.want_trace = ridge_rel != 0.0 ? 1 : 0;
  BuildOut built;
  SMN_TRY(run_build(ctx, b, &built));
  const bool prepped = ridge_rel == 0.0 || built.trace;
  if (prepped) {
    const int64_t n_sh = (ridge_abs != 0.0 || ridge_rel != 0.0) ? n : 0;
    SMN_TRY(aug_prep(ctx, dtype, f->a, f->lda, f->n_pad, f->n_pad + kTile, y_d, n, c, c, n_sh, ridge_abs, 0, nullptr, ridge_rel, n));
  }
  SMN_TRY(fit_factor(f, y_d, prepped, ridge_rel, ridge_abs, quad_h, logdet_h, info_h));
  *out = guard.release();
  return SMN_OK;
}

extern "C" int smn_fit_create_from_kernel(smn_ctx* ctx, int dtype, const void* k_d, int64_t n, int64_t ldk, const void* y_d,
                                          int64_t c, double ridge_rel, double ridge_abs, int64_t capacity, smn_fit** out,
                                          double* quad_h, double* logdet_h, int* info_h) {
  if (!ctx || !k_d || !y_d || !out) return SMN_EINVAL;
  SMN_ENTER(ctx);
  *out = nullptr;
  SMN_CHECK_LD(ctx, "smn_fit_create_from_kernel", ldk, n);
  smn_fit* f = nullptr;
  SMN_TRY(fit_alloc(ctx, "smn_fit_create_from_kernel", dtype, n, c, capacity, 0, false, &f));
  FitGuard guard{f};
  SMN_TRY(copy_matrix(ctx, dtype, f->a, f->lda, k_d, ldk, n, n, 1));
  SMN_TRY(fill_identity_pad(ctx, dtype, f->a, f->lda, f->n_pad, n));
  SMN_TRY(fit_factor(f, y_d, false, ridge_rel, ridge_abs, quad_h, logdet_h, info_h));
  *out = guard.release();
  return SMN_OK;
}

extern "C" int smn_fit_predict(smn_fit* fit, const void* xt_d, int64_t t, int64_t ldxt, void* mean_d, void* var_d, void* cov_d,
                               int64_t ldcov) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  if (!fit->fused) return smn_fail(ctx, SMN_EINVAL, "smn_fit_predict: the state was made from a kernel matrix (use smn_fit_apply)");
  if (!xt_d) return smn_fail(ctx, SMN_EINVAL, "smn_fit_predict: xt_d is NULL");
  SMN_TRY(check_outputs(fit, "smn_fit_predict", t, mean_d, cov_d, ldcov));
  SMN_CHECK_LD(ctx, "smn_fit_predict", ldxt, fit->d);
  if (fit->info != 0) return nan_outputs(fit, t, mean_d, var_d, cov_d, ldcov);
  const size_t es = fit->es();
  {
    // Workspace of the largest chunk, taken before anything is launched: the padded chunk (slot 0) and the cross build's
    // per-row tables (slot 1: 2 (activation layers) + 2 rows of rows1 + rows2 elements, run_build; larger than the K_tt
    // build's).  A slot that has to grow synchronises the stream, so it grows here and not between two launches of the call.
    const int64_t rp_max = round_up(std::min(fit->capacity, t), kTile);
    void* w = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp_max + es * (size_t)rp_max * (size_t)fit->kp, &w));
    SMN_TRY(smn_workspace(ctx, 1, es * (size_t)(2 * (fit->num_hiddens + 1) + 2) * (size_t)(rp_max + fit->n_pad), &w));
  }
  for (int64_t start = 0; start < t; start += fit->capacity) {
    const int64_t r = std::min(fit->capacity, t - start), rp = round_up(r, kTile);
    void* xs = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp + es * (size_t)rp * (size_t)fit->kp, &xs));
    double* q = static_cast<double*>(xs);
    char* xp = reinterpret_cast<char*>(q + rp);
    SMN_TRY(pad_rows(ctx, fit->dtype, static_cast<const char*>(xt_d) + es * (size_t)(start * ldxt), r, ldxt, fit->d, xp, rp, fit->kp, q));
    SMN_TRY(clear_tail_rows(fit, r));
    const BuildCall b = chunk_build_call(fit, xp, q, rp);
    if (cov_d) {   // K_tt (lower tiles, exact diagonal) into the trailing block; the cross build after it leaves the same table
      BuildCall s = b;
      s.x2p = xp; s.ld2 = fit->kp; s.rows2 = rp; s.q2 = q;
      s.symmetric = 1; s.exact_diag = 1;
      s.out_rows = r; s.out_cols = r;
      void* dst = fit->at(fit->n_pad, fit->n_pad);
      s.out_k = fit->ntk ? nullptr : dst; s.out_t = fit->ntk ? dst : nullptr;
      SMN_TRY(run_build(ctx, s));
    }
    BuildOut built;
    SMN_TRY(build_cross(fit, b, r, &built));
    // k_tt: the closed-form diagonal of the chunk's rows from the build's own table (what exact_diag writes)
    const void* ktt = fit->ntk ? built.diag_t : built.diag_k;
    SMN_TRY(finish_chunk(fit, r, ktt, 1, static_cast<char*>(mean_d) + es * (size_t)(start * fit->c),
                         var_d ? static_cast<char*>(var_d) + es * (size_t)start : nullptr, cov_d, ldcov));
  }
  return SMN_OK;
}

extern "C" int smn_fit_predict_grad(smn_fit* fit, const void* xt_d, int64_t t, int64_t ldxt, void* dmean_d, void* dvar_d) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  const char* who = "smn_fit_predict_grad";
  if (!fit->fused) return smn_fail(ctx, SMN_EINVAL, "%s: the state was made from a kernel matrix (no kernel to differentiate)", who);
  if (!xt_d) return smn_fail(ctx, SMN_EINVAL, "%s: xt_d is NULL", who);
  if (!dmean_d && !dvar_d) return smn_fail(ctx, SMN_EINVAL, "%s: dmean_d and dvar_d are both NULL", who);
  if (t <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: t = %lld must be at least 1", who, (long long)t);
  SMN_CHECK_LD(ctx, who, ldxt, fit->d);
  const int64_t c = fit->c, d = fit->d, n_pad = fit->n_pad;
  if (fit->info != 0) {
    SMN_TRY(fill_nan(fit, dmean_d, t, c * d, c * d));
    return fill_nan(fit, dvar_d, t, d, d);
  }
  InputGradOps o{};
  o.spec = BuildSpec{fit->dtype, fit->net, fit->act, fit->num_hiddens, fit->w_std, fit->b_std, fit->last_w_std};
  o.ntk = fit->ntk;
  const int nsets = input_grad_nsets(o.spec);
  if (nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "%s: num_hiddens too large (max %d activation layers)", who, kMaxSets);
  const size_t es = fit->es();
  // Workspace of the largest chunk before the first launch, as in smn_fit_predict: the padded chunk (slot 0), the cross build's
  // tables (slot 1), and in slot 4 the gradient's own scratch with U [rp, n_pad] behind it.
  const int64_t rp_max = round_up(std::min(fit->capacity, t), kTile);
  const size_t ig_bytes = input_grad_ws_bytes(fit->dtype, nsets, rp_max, n_pad, false);
  void *w0 = nullptr, *w4 = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp_max + es * (size_t)rp_max * (size_t)fit->kp, &w0));
  SMN_TRY(smn_workspace(ctx, 1, es * (size_t)(2 * (fit->num_hiddens + 1) + 2) * (size_t)(rp_max + n_pad), &w0));
  SMN_TRY(smn_workspace(ctx, 4, ig_bytes + es * (size_t)rp_max * (size_t)n_pad, &w4));
  SMN_TRY(ensure_grad_state(fit));
  o.x2p = fit->xp(); o.q2 = fit->q(); o.n2 = fit->n; o.rows2 = n_pad; o.x2t = fit->xt;
  o.kp = fit->kp; o.d = d;
  const double inv_d = 1.0 / (double)d;
  for (int64_t start = 0; start < t; start += fit->capacity) {
    const int64_t r = std::min(fit->capacity, t - start), rp = round_up(r, kTile);
    void* xs = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp + es * (size_t)rp * (size_t)fit->kp, &xs));
    double* q = static_cast<double*>(xs);
    char* xp = reinterpret_cast<char*>(q + rp);
    SMN_TRY(pad_rows(ctx, fit->dtype, static_cast<const char*>(xt_d) + es * (size_t)(start * ldxt), r, ldxt, d, xp, rp, fit->kp, q));
    o.x1p = xp; o.q1 = q; o.n1 = r; o.rows1 = rp;
    const InputGradWs w = input_grad_ws_carve(w4, fit->dtype, nsets, rp, n_pad, false);
    void* u = static_cast<char*>(w4) + ig_bytes;
    if (dvar_d) {   // V^T = K_td L^-T as smn_fit_predict forms it, then U = V^T L^-1 by the forward sweep on L'
      SMN_TRY(clear_tail_rows(fit, r));
      SMN_TRY(build_cross(fit, chunk_build_call(fit, xp, q, rp), r, nullptr));
      SMN_TRY(solve_rows_padded(ctx, fit->dtype, fit->a, n_pad + rp, n_pad, fit->lda));
      SMN_TRY(flip_rows(ctx, fit->dtype, fit->lt_at(n_pad), n_pad, fit->at(n_pad, 0), fit->lda, rp, n_pad));
      SMN_TRY(solve_rows_padded(ctx, fit->dtype, fit->lt, n_pad + rp, n_pad, n_pad));
      SMN_TRY(flip_rows(ctx, fit->dtype, u, n_pad, fit->lt_at(n_pad), n_pad, rp, n_pad));
    }
    SMN_TRY(input_grad_factors(ctx, o, w, nullptr, 0));
    for (int64_t k = 0; k < c && dmean_d; ++k) {
      SMN_TRY(input_grad_seed(ctx, o, w, static_cast<const char*>(fit->alpha) + es * (size_t)(k * n_pad), 0));
      SMN_TRY(input_grad_contract(ctx, o, w, inv_d, 2.0 * inv_d, 0.0, static_cast<char*>(dmean_d) + es * (size_t)((start * c + k) * d),
                                  c * d));
    }
    if (dvar_d) {
      SMN_TRY(input_grad_seed(ctx, o, w, u, n_pad));
      SMN_TRY(input_grad_contract(ctx, o, w, -2.0 * inv_d, -4.0 * inv_d, 2.0 * inv_d, static_cast<char*>(dvar_d) + es * (size_t)(start * d), d));
    }
  }
  return SMN_OK;
}

extern "C" int smn_fit_apply(smn_fit* fit, const void* k_td_d, int64_t t, int64_t ldk, const void* ktt_diag_d, const void* k_tt_d,
                             int64_t ldtt, void* mean_d, void* var_d, void* cov_d, int64_t ldcov) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  if (!k_td_d) return smn_fail(ctx, SMN_EINVAL, "smn_fit_apply: k_td_d is NULL");
  SMN_TRY(check_outputs(fit, "smn_fit_apply", t, mean_d, cov_d, ldcov));
  SMN_CHECK_LD(ctx, "smn_fit_apply", ldk, fit->n);
  if (k_tt_d) SMN_CHECK_LD(ctx, "smn_fit_apply", ldtt, t);
  if (cov_d && !k_tt_d) return smn_fail(ctx, SMN_EINVAL, "smn_fit_apply: cov_d needs k_tt_d");
  if (var_d && !ktt_diag_d && !k_tt_d) return smn_fail(ctx, SMN_EINVAL, "smn_fit_apply: var_d needs ktt_diag_d or k_tt_d");
  if (fit->info != 0) return nan_outputs(fit, t, mean_d, var_d, cov_d, ldcov);
  const size_t es = fit->es();
  for (int64_t start = 0; start < t; start += fit->capacity) {
    const int64_t r = std::min(fit->capacity, t - start);
    SMN_TRY(clear_tail_rows(fit, r));
    SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(fit->n_pad, 0), fit->lda, static_cast<const char*>(k_td_d) + es * (size_t)(start * ldk),
                        ldk, r, fit->n, 0));
    if (cov_d) SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(fit->n_pad, fit->n_pad), fit->lda, k_tt_d, ldtt, r, r, 1));
    const void* ktt = nullptr;
    int64_t stride = 1;
    if (ktt_diag_d) ktt = static_cast<const char*>(ktt_diag_d) + es * (size_t)start;
    else if (k_tt_d) { ktt = static_cast<const char*>(k_tt_d) + es * (size_t)(start * ldtt + start); stride = ldtt + 1; }
    SMN_TRY(finish_chunk(fit, r, ktt, stride, static_cast<char*>(mean_d) + es * (size_t)(start * fit->c),
                         (var_d && ktt) ? static_cast<char*>(var_d) + es * (size_t)start : nullptr, cov_d, ldcov));
  }
  return SMN_OK;
}

// The solve a state knows how to do, handed out: U = K_td K~^-1 for a cross kernel of the caller's and alpha = K~^-1 Y -- the two
// sweeps of smn_fit_predict_grad's variance path (V^T = K_td L^-T on L, then U = V^T L^-1 as the forward sweep on L') with
// K_td copied into the test rows as smn_fit_apply does.  Either kind of state; what the call adds to it is L' and alpha^T.
extern "C" int smn_fit_weights(smn_fit* fit, const void* k_td_d, int64_t t, int64_t ldk, void* u_d, int64_t ldu, void* alpha_d) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  const char* who = "smn_fit_weights";
  if (!u_d && !alpha_d) return smn_fail(ctx, SMN_EINVAL, "%s: u_d and alpha_d are both NULL", who);
  const int64_t n = fit->n, n_pad = fit->n_pad, c = fit->c;
  if (u_d) {
    if (!k_td_d) return smn_fail(ctx, SMN_EINVAL, "%s: u_d needs k_td_d", who);
    if (t < 1 || t > fit->capacity)
      return smn_fail(ctx, SMN_EINVAL, "%s: t = %lld outside [1, capacity = %lld]", who, (long long)t, (long long)fit->capacity);
    SMN_CHECK_LD(ctx, who, ldk, n);
    SMN_CHECK_LD(ctx, who, ldu, n);
  }
  if (fit->info != 0) {
    if (u_d) SMN_TRY(fill_nan(fit, u_d, t, n, ldu));
    return fill_nan(fit, alpha_d, n, c, c);
  }
  SMN_TRY(ensure_grad_state(fit));
  const size_t es = fit->es();
  if (u_d) {
    const int64_t rp = round_up(t, kTile);
    SMN_TRY(clear_tail_rows(fit, t));
    SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(n_pad, 0), fit->lda, k_td_d, ldk, t, n, 0));
    SMN_TRY(solve_rows_padded(ctx, fit->dtype, fit->a, n_pad + rp, n_pad, fit->lda));
    SMN_TRY(flip_rows(ctx, fit->dtype, fit->lt_at(n_pad), n_pad, fit->at(n_pad, 0), fit->lda, rp, n_pad));
    SMN_TRY(solve_rows_padded(ctx, fit->dtype, fit->lt, n_pad + rp, n_pad, n_pad));
    // columns [0, n) of the row put back in order: the reversed row's last n entries
    SMN_TRY(flip_rows(ctx, fit->dtype, u_d, ldu, fit->lt_at(n_pad) + es * (size_t)(n_pad - n), n_pad, t, n));
  }
  if (alpha_d) SMN_TRY(transpose_matrix(ctx, fit->dtype, alpha_d, c, fit->alpha, n_pad, c, n));
  return SMN_OK;
}

extern "C" int smn_fit_reserve(smn_fit* fit, int64_t max_points) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  if (max_points < fit->n)
    return smn_fail(ctx, SMN_EINVAL, "smn_fit_reserve: max_points = %lld is below the state's n = %lld training rows",
                    (long long)max_points, (long long)fit->n);
  const int64_t new_pad = round_up(max_points, kTile);
  if (new_pad <= fit->n_pad) return SMN_OK;
  return fit_grow(fit, "smn_fit_reserve", new_pad);
}

extern "C" int smn_fit_append(smn_fit* fit, const void* x_new_d, int64_t k, int64_t ldx, const void* y_new_d, double* quad_h,
                              double* logdet_h, int* info_h) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  const char* who = "smn_fit_append";
  if (!fit->fused) return smn_fail(ctx, SMN_EINVAL, "%s: the state was made from a kernel matrix (use smn_fit_append_from_kernel)", who);
  if (!x_new_d) return smn_fail(ctx, SMN_EINVAL, "%s: x_new_d is NULL", who);
  SMN_CHECK_LD(ctx, who, ldx, fit->d);
  SMN_TRY(append_enter(fit, who, k, y_new_d));
  const size_t es = fit->es();
  {   // workspace of the largest chunk before the first launch, as in smn_fit_predict (at the grown n_pad)
    const int64_t rp_max = round_up(std::min(fit->capacity, k), kTile);
    void* w = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp_max + es * (size_t)rp_max * (size_t)fit->kp, &w));
    SMN_TRY(smn_workspace(ctx, 1, es * (size_t)(2 * (fit->num_hiddens + 1) + 2) * (size_t)(rp_max + fit->n_pad), &w));
  }
  int info = 0;
  for (int64_t start = 0; start < k && info == 0; start += fit->capacity) {
    const int64_t r = std::min(fit->capacity, k - start), rp = round_up(r, kTile), n0 = fit->n;
    void* xs = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)rp + es * (size_t)rp * (size_t)fit->kp, &xs));
    double* q = static_cast<double*>(xs);
    char* xp = reinterpret_cast<char*>(q + rp);
    SMN_TRY(pad_rows(ctx, fit->dtype, static_cast<const char*>(x_new_d) + es * (size_t)(start * ldx), r, ldx, fit->d, xp, rp, fit->kp, q));
    SMN_TRY(clear_append_rows(fit, rp));
    const BuildCall b = chunk_build_call(fit, xp, q, rp);
    BuildCall s = b;   // K(x+, x+): lower tiles, exact diagonal, into the trailing block (smn_fit_predict's cov build)
    s.x2p = xp; s.ld2 = fit->kp; s.rows2 = rp; s.q2 = q;
    s.symmetric = 1; s.exact_diag = 1;
    s.out_rows = r; s.out_cols = r;
    void* dst = fit->at(fit->n_pad, fit->n_pad);
    s.out_k = fit->ntk ? nullptr : dst; s.out_t = fit->ntk ? dst : nullptr;
    SMN_TRY(run_build(ctx, s));
    SMN_TRY(build_cross(fit, b, r, nullptr));
    SMN_TRY(append_chunk(fit, r, static_cast<const char*>(y_new_d) + es * (size_t)(start * fit->c), &info));
    if (info == 0) {   // the chunk's padded rows and their q join the state's copy: the bits pad_rows gives a fresh state
      SMN_HIP(ctx, hipMemcpyAsync(fit->q() + n0, q, sizeof(double) * (size_t)r, hipMemcpyDeviceToDevice, ctx->stream));
      SMN_HIP(ctx, hipMemcpyAsync(fit->xp() + es * (size_t)(n0 * fit->kp), xp, es * (size_t)r * (size_t)fit->kp, hipMemcpyDeviceToDevice,
                                  ctx->stream));
    }
  }
  append_publish(fit, info, quad_h, logdet_h, info_h);
  return SMN_OK;
}

extern "C" int smn_fit_append_from_kernel(smn_fit* fit, const void* k_nd_d, int64_t k, int64_t n, int64_t ldk, const void* k_nn_d,
                                          int64_t ldnn, const void* y_new_d, double* quad_h, double* logdet_h, int* info_h) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  const char* who = "smn_fit_append_from_kernel";
  if (fit->fused)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: the state was made from inputs and keeps its own copy of x (use smn_fit_append)", who);
  if (!k_nd_d) return smn_fail(ctx, SMN_EINVAL, "%s: k_nd_d is NULL", who);
  if (!k_nn_d) return smn_fail(ctx, SMN_EINVAL, "%s: k_nn_d is NULL", who);
  if (k < 1) return smn_fail(ctx, SMN_EINVAL, "%s: k = %lld must be at least 1", who, (long long)k);
  if (n != fit->n)
    return smn_fail(ctx, SMN_EINVAL, "%s: n = %lld, the state holds %lld training rows", who, (long long)n, (long long)fit->n);
  SMN_CHECK_LD(ctx, who, ldk, n);
  SMN_CHECK_LD(ctx, who, ldnn, k);
  SMN_TRY(append_enter(fit, who, k, y_new_d));
  const size_t es = fit->es();
  int info = 0;
  for (int64_t start = 0; start < k && info == 0; start += fit->capacity) {
    const int64_t r = std::min(fit->capacity, k - start), rp = round_up(r, kTile);
    const char* nn_row = static_cast<const char*>(k_nn_d) + es * (size_t)(start * ldnn);
    SMN_TRY(clear_append_rows(fit, rp));
    // K(chunk, all rows so far) = [k_nd rows | the chunk's rows of k_nn left of its own block]
    SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(fit->n_pad, 0), fit->lda, static_cast<const char*>(k_nd_d) + es * (size_t)(start * ldk),
                        ldk, r, n, 0));
    SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(fit->n_pad, n), fit->lda, nn_row, ldnn, r, start, 0));
    SMN_TRY(copy_matrix(ctx, fit->dtype, fit->at(fit->n_pad, fit->n_pad), fit->lda, nn_row + es * (size_t)start, ldnn, r, r, 1));
    SMN_TRY(append_chunk(fit, r, static_cast<const char*>(y_new_d) + es * (size_t)(start * fit->c), &info));
  }
  append_publish(fit, info, quad_h, logdet_h, info_h);
  return SMN_OK;
}

extern "C" int smn_fit_stats(smn_fit* fit, int64_t* max_points, double* ridge, double* quad_h, double* logdet_h) {
  if (!fit) return SMN_EINVAL;
  if (max_points) *max_points = fit->n_pad;
  if (ridge) *ridge = fit->ridge;
  for (int64_t k = 0; k < fit->c && quad_h; ++k) quad_h[k] = fit->quad[k];
  if (logdet_h) *logdet_h = fit->logdet;
  return SMN_OK;
}

extern "C" int smn_fit_info(smn_fit* fit, int64_t* n, int64_t* c, int64_t* capacity, size_t* bytes) {
  if (!fit) return SMN_EINVAL;
  if (n) *n = fit->n;
  if (c) *c = fit->c;
  if (capacity) *capacity = fit->capacity;
  if (bytes) *bytes = fit->bytes;
  return SMN_OK;
}

extern "C" int smn_fit_destroy(smn_fit* fit) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  (void)hipStreamSynchronize(ctx->stream);   // nothing the state's calls issued may still run on its memory
  fit->ctx = nullptr;
  fit_free(fit);
  return SMN_OK;
}
