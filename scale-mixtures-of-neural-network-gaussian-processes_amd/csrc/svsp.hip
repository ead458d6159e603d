// svsp.hip — evaluation of the sparse variational scale-mixture classifier, SVSP.test_acc_nll (spax/models.py:58-78,
// spax/priors.py:28-34,60-68, spax/utils.py:61-74 of the reference):
//   smn_kernel_conv_diag   K(x_t, x_t) of the conv kernels (the per-image pass of cnn.hip / cnn_resnet.hip, exposed)
//   smn_svsp_moments       mean [T,C] and var [T,C] of the latent function at the test points from K_ZZ, K_Zt, diag K_tt, q_mu, q_var
//   smn_mc_softmax         the Monte-Carlo softmax head: S draws per (point, class), log-softmax over classes per draw,
//                          log-sum-exp over draws per class -> log-likelihood of the label, class scores, prediction
//   smn_rng_variates       the variates the head draws, written out (the seam the head is tested through)
//   smn_debug_philox       one raw Philox4x32-10 block
//
// The head is the hot path: a CIFAR-10 test set at the reference's default S = 10000 is 1e9 variates, each through a fused
// multiply-add, two exponentials and a share of a logarithm.  Nothing of size T C S exists: a variate is a pure function of
// (seed, point, class, draw, df) (counter-based generator, include/smnngp.h), made in registers where it is consumed.
//   One workgroup (4 waves) per test point, lanes over draws.  A draw needs its C values twice (log-sum-exp over the
//   classes, then the C log-softmax values), and every class needs a running (max, sum) over the draws:
//     C <= 16  the draw's values and the per-lane running pairs of all classes live in registers; lanes merge once, at the end;
//     C >  16  the values are generated twice (the generator is cheaper than 2 C registers per lane) and every 64 draws of a
//              class are merged across the wave into one running pair per wave and class in LDS.
// VALU / transcendental bound by construction; no MFMA: there is no GEMM here.
#include <cmath>
#include <limits>
#include <vector>

#include "internal.hpp"

namespace {

#include "svsp_rng.hpp"

template <typename T>
__global__ void __launch_bounds__(256) rng_variates_kernel(uint32_t k0, uint32_t k1, T df, uint32_t point0, int C, int64_t S,
                                                           T* __restrict__ out) {
  const int64_t p = blockIdx.x;
  const int g = blockIdx.y;
  for (int64_t s = threadIdx.x; s < S; s += 256) {
    T z[4];
    draw4<T>(k0, k1, (uint32_t)s, point0 + (uint32_t)p, g, C, df, z);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * g + k < C) out[(p * C + 4 * g + k) * S + s] = z[k];
  }
}

__global__ void philox_kernel(U4 ctr, uint32_t k0, uint32_t k1, uint32_t* out) {
  const U4 r = philox4x32_10(ctr, k0, k1);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

// ---------------------------------------------------------------- the head
constexpr int kMaxC = SMN_SVSP_MAX_CLASSES;
constexpr int kRegC = 16;   // classes whose per-lane state fits in registers
constexpr double kNegInf = -std::numeric_limits<double>::infinity();

template <typename T>
struct McArgs {
  const T* mean; const T* sigma; const int* labels; const T* noise;
  double* ll; int* pred; double* score;
  int C; int64_t S;
  uint32_t k0, k1, point0;
  T df;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// running log-sum-exp pair (m, s): the terms seen so far sum to s exp(m).  One exponential per term.
template <typename T, typename A>
__device__ __forceinline__ void lse_push(double& m, A& s, double l) {
  const double d = l - m;                            // +inf on the first term (m = -inf, s = 0)
  const A e = (A)Real<T>::exp_((T)(-fabs(d)));
  const bool up = d > 0.0;
  s = up ? fma(s, e, A(1)) : s + e;
  m = up ? l : m;
}

template <typename T, bool REG>
__global__ void __launch_bounds__(256) mc_softmax_kernel(McArgs<T> a) {
  __shared__ T s_mu[kMaxC], s_sg[kMaxC];
  __shared__ double s_m[4][kMaxC], s_s[4][kMaxC];
  const int64_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C;
  const int64_t S = a.S;
  // classes >= C: mean -inf, sigma 0, so their value is -inf for every (finite) variate and they drop out of every sum
  for (int c = tid; c < kMaxC; c += 256) {
    s_mu[c] = c < C ? a.mean[t * C + c] : -std::numeric_limits<T>::infinity();
    s_sg[c] = c < C ? a.sigma[t * C + c] : T(0);
  }
  for (int i = tid; i < 4 * kMaxC; i += 256) {
    (&s_m[0][0])[i] = kNegInf;
    (&s_s[0][0])[i] = 0.0;
  }
  __syncthreads();
  const uint32_t point = a.point0 + (uint32_t)t;
  const T* nz = a.noise ? a.noise + t * C * S : nullptr;
  auto gen4 = [&](int64_t s, int g, T z[4]) {
    if (nz) {
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = 4 * g + k < C ? nz[(int64_t)(4 * g + k) * S + s] : T(0);
    } else {
      draw4<T>(a.k0, a.k1, (uint32_t)s, point, g, C, a.df, z);
    }
  };
  if (REG) {
    double m[kRegC];
    T sm[kRegC];
#pragma unroll
    for (int c = 0; c < kRegC; ++c) { m[c] = kNegInf; sm[c] = T(0); }
    for (int64_t s = tid; s < S; s += 256) {
      T f[kRegC];
#pragma unroll
      for (int g = 0; g < kRegC / 4; ++g) {
        if (4 * g < C) {
          T z[4];
          gen4(s, g, z);
#pragma unroll
          for (int k = 0; k < 4; ++k) f[4 * g + k] = fma(s_sg[4 * g + k], z[k], s_mu[4 * g + k]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) f[4 * g + k] = -std::numeric_limits<T>::infinity();
        }
      }
      T fm = f[0];
#pragma unroll
      for (int c = 1; c < kRegC; ++c) fm = fmax(fm, f[c]);
      T se = T(0);
#pragma unroll
      for (int c = 0; c < kRegC; ++c) se += Real<T>::exp_(f[c] - fm);
      const double lse = (double)fm + (double)Real<T>::log_(se);
#pragma unroll
      for (int c = 0; c < kRegC; ++c)
        if (c < C) lse_push<T, T>(m[c], sm[c], (double)f[c] - lse);
    }
    // lanes -> one pair per wave and class
#pragma unroll
    for (int c = 0; c < kRegC; ++c) {
      if (c < C) {
        const double M = wave_max(m[c]);
        const double part = sm[c] == T(0) ? 0.0 : (double)sm[c] * exp(m[c] - M);   // (a NaN sum stays NaN)
        const double tot = wave_sum(part);
        if (lane == 0) { s_m[wave][c] = M; s_s[wave][c] = tot; }
      }
    }
  } else {
    const int G = (C + 3) >> 2;
    for (int64_t s0 = (int64_t)wave * 64; s0 < S; s0 += 256) {
      const bool act = s0 + lane < S;
      const int64_t s = act ? s0 + lane : S - 1;
      T fm = -std::numeric_limits<T>::infinity(), se = T(0);
      for (int g = 0; g < G; ++g) {
        T z[4], f[4];
        gen4(s, g, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = fma(s_sg[4 * g + k], z[k], s_mu[4 * g + k]);
        const T nm = fmax(fmax(fm, fmax(f[0], f[1])), fmax(f[2], f[3]));
        se = se * Real<T>::exp_(fm - nm) + ((Real<T>::exp_(f[0] - nm) + Real<T>::exp_(f[1] - nm)) +
                                             (Real<T>::exp_(f[2] - nm) + Real<T>::exp_(f[3] - nm)));
        fm = nm;
      }
      const double lse = (double)fm + (double)Real<T>::log_(se);
      for (int g = 0; g < G; ++g) {
        T z[4];
        gen4(s, g, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = 4 * g + k;
          if (c < C) {   // uniform
            const double l = act ? (double)fma(s_sg[c], z[k], s_mu[c]) - lse : kNegInf;
            const double wm = wave_max(l);
            const double e = act ? (double)Real<T>::exp_((T)(l - wm)) : 0.0;
            const double ws = wave_sum(e);
            if (lane == 0) {
              const double m0 = s_m[wave][c], d = wm - m0;
              const double sc = exp(-fabs(d));
              s_s[wave][c] = d > 0.0 ? fma(s_s[wave][c], sc, ws) : fma(ws, sc, s_s[wave][c]);
              s_m[wave][c] = d > 0.0 ? wm : m0;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // waves -> the class scores; thread 0: label log-likelihood and prediction
  __shared__ double s_score[kMaxC];
  if (tid < C) {
    double M = kNegInf;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmax(M, s_m[w][tid]);
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) tot += s_s[w][tid] == 0.0 ? 0.0 : s_s[w][tid] * exp(s_m[w][tid] - M);   // (a NaN sum stays NaN)
    const double sc = M + log(tot);
    s_score[tid] = sc;
    if (a.score) a.score[t * C + tid] = sc;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int c = 1; c < C; ++c)
      if (s_score[c] > s_score[best]) best = c;
    a.pred[t] = best;
    a.ll[t] = s_score[a.labels[t]] - log((double)S);
  }
}

// ---------------------------------------------------------------- posterior moments
// u [I, T + C] = L_rel^-1 [K_Zt | q_mu^T];  at [I, T] = K_abs^-1 K_Zt;  all fp64
template <typename T>
__global__ void __launch_bounds__(256) svsp_pack_kernel(const T* __restrict__ kzt, const double* __restrict__ q_mu, int64_t I,
                                                        int64_t Tn, int C, double* __restrict__ u, double* __restrict__ at) {
  const int64_t j = blockIdx.y, ldu = Tn + C;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < Tn) {
    const double v = (double)kzt[j * Tn + i];
    u[j * ldu + i] = v;
    at[j * Tn + i] = v;
  } else if (i < ldu) {
    u[j * ldu + i] = q_mu[(i - Tn) * I + j];
  }
}

constexpr int kMomC = 8;   // classes per thread
template <typename T>
__global__ void __launch_bounds__(256) svsp_moments_kernel(const double* __restrict__ u, const double* __restrict__ at,
                                                           const T* __restrict__ ktt, const double* __restrict__ q_var, int64_t I,
                                                           int64_t Tn, int C, int bad, T* __restrict__ mean, T* __restrict__ var,
                                                           int* __restrict__ nonpos) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, ldu = Tn + C;
  const int c0 = blockIdx.y * kMomC;
  if (t >= Tn) return;
  if (bad) {
    for (int k = 0; k < kMomC && c0 + k < C; ++k) {
      mean[t * C + c0 + k] = std::numeric_limits<T>::quiet_NaN();
      var[t * C + c0 + k] = std::numeric_limits<T>::quiet_NaN();
    }
    return;
  }
  double q = 0.0, mu[kMomC], va[kMomC];
#pragma unroll
  for (int k = 0; k < kMomC; ++k) mu[k] = va[k] = 0.0;
  for (int64_t j = 0; j < I; ++j) {
    const double uj = u[j * ldu + t], aj = at[j * Tn + t], a2 = aj * aj;
    q = fma(uj, uj, q);
#pragma unroll
    for (int k = 0; k < kMomC; ++k) {
      if (c0 + k < C) {
        mu[k] = fma(uj, u[j * ldu + Tn + c0 + k], mu[k]);
        va[k] = fma(a2, q_var[(int64_t)(c0 + k) * I + j], va[k]);
      }
    }
  }
  const double v0 = (double)ktt[t] - q;
#pragma unroll
  for (int k = 0; k < kMomC; ++k) {
    if (c0 + k < C) {
      const double v = v0 + va[k];
      mean[t * C + c0 + k] = (T)mu[k];
      var[t * C + c0 + k] = (T)v;
      if (v <= 0.0) atomicAdd(nonpos, 1);
    }
  }
}

template <typename T>
int moments_t(smn_ctx* ctx, const double* k_zz, const void* k_zt, const void* ktt, const double* q_mu, const double* q_var,
              int64_t I, int64_t Tn, int C, double eps, void* mean, void* var, int* info_h, int64_t* nonpos_h) {
  const size_t nii = (size_t)I * I, nu = (size_t)I * (size_t)(Tn + C), na = (size_t)I * (size_t)Tn;
  void* wv = nullptr;
  SMN_TRY(smn_workspace(ctx, 10, sizeof(double) * (2 * nii + nu + na) + 64, &wv));
  double* k_rel = static_cast<double*>(wv);
  double* k_abs = k_rel + nii;
  double* u = k_abs + nii;
  double* at = u + nu;
  int* cnt = reinterpret_cast<int*>(at + na);
  hipStream_t st = ctx->stream;
  SMN_HIP(ctx, hipMemcpyAsync(k_rel, k_zz, sizeof(double) * nii, hipMemcpyDeviceToDevice, st));
  SMN_HIP(ctx, hipMemcpyAsync(k_abs, k_zz, sizeof(double) * nii, hipMemcpyDeviceToDevice, st));
  SMN_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int), st));
  hipLaunchKernelGGL(svsp_pack_kernel<T>, dim3((unsigned)((Tn + C + 255) / 256), (unsigned)I), dim3(256), 0, st,
                     static_cast<const T*>(k_zt), q_mu, I, Tn, C, u, at);
  SMN_CHECK_LAUNCH(ctx);
  // K_rel = K_ZZ + eps tr(K_ZZ) / I (the relative ridge of NNGPKernel.predict), K_abs = K_ZZ + eps (models.py:68)
  int info_rel = 0, info_abs = 0;
  SMN_TRY(smn_cholesky(ctx, SMN_F64, k_rel, I, I, I, I, 0.0, eps, &info_rel, nullptr));
  SMN_TRY(smn_cholesky(ctx, SMN_F64, k_abs, I, I, I, I, eps, 0.0, &info_abs, nullptr));
  int info = info_rel ? info_rel : info_abs;
  if (info == 0) {
    // A pivot that rounding left a hair above zero passes the factorisation and poisons every solve after it: a matrix with
    // a pivot below I u max_j K_jj (the rank tolerance of a pivoted Cholesky, LAPACK dpstrf) is not numerically positive
    // definite either, and is reported like one that is not (1-based index of the first such pivot).
    std::vector<double> d(3 * (size_t)I);
    SMN_HIP(ctx, hipMemcpy2DAsync(d.data(), 8, k_zz, 8 * (size_t)(I + 1), 8, (size_t)I, hipMemcpyDeviceToHost, st));
    SMN_HIP(ctx, hipMemcpy2DAsync(d.data() + I, 8, k_rel, 8 * (size_t)(I + 1), 8, (size_t)I, hipMemcpyDeviceToHost, st));
    SMN_HIP(ctx, hipMemcpy2DAsync(d.data() + 2 * I, 8, k_abs, 8 * (size_t)(I + 1), 8, (size_t)I, hipMemcpyDeviceToHost, st));
    SMN_HIP(ctx, hipStreamSynchronize(st));
    double dmax = 0.0;
    for (int64_t j = 0; j < I; ++j) dmax = std::fmax(dmax, std::fabs(d[j]));
    const double tol = (double)I * std::numeric_limits<double>::epsilon() * dmax;
    for (int64_t j = 0; j < I && info == 0; ++j)
      if (!(d[I + j] * d[I + j] > tol) || !(d[2 * I + j] * d[2 * I + j] > tol)) info = (int)(j + 1);
  }
  if (info == 0) {
    SMN_TRY(smn_trsm(ctx, SMN_F64, k_rel, I, I, u, Tn + C, Tn + C, 0));
    SMN_TRY(smn_trsm(ctx, SMN_F64, k_abs, I, I, at, Tn, Tn, 0));
    SMN_TRY(smn_trsm(ctx, SMN_F64, k_abs, I, I, at, Tn, Tn, 1));
  }
  hipLaunchKernelGGL(svsp_moments_kernel<T>, dim3((unsigned)((Tn + 255) / 256), (unsigned)((C + kMomC - 1) / kMomC)), dim3(256), 0,
                     st, u, at, static_cast<const T*>(ktt), q_var, I, Tn, C, info != 0 ? 1 : 0, static_cast<T*>(mean),
                     static_cast<T*>(var), cnt);
  SMN_CHECK_LAUNCH(ctx);
  int cnt_h = 0;
  SMN_HIP(ctx, hipMemcpyAsync(&cnt_h, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
  SMN_HIP(ctx, hipStreamSynchronize(st));
  if (info_h) *info_h = info;
  if (nonpos_h) *nonpos_h = cnt_h;
  return SMN_OK;
}

template <typename T>
int mc_softmax_t(smn_ctx* ctx, const void* mean, const void* sigma, const int* labels_h, int64_t Tn, int C, int64_t S, double df,
                 uint64_t seed, int64_t point0, const void* noise, double* ll, int* pred, double* score) {
  void* wv = nullptr;
  SMN_TRY(smn_workspace(ctx, 11, sizeof(int) * (size_t)Tn, &wv));
  int* labels = static_cast<int*>(wv);
  SMN_HIP(ctx, hipMemcpyAsync(labels, labels_h, sizeof(int) * (size_t)Tn, hipMemcpyHostToDevice, ctx->stream));
  McArgs<T> a;
  a.mean = static_cast<const T*>(mean); a.sigma = static_cast<const T*>(sigma); a.labels = labels;
  a.noise = static_cast<const T*>(noise);
  a.ll = ll; a.pred = pred; a.score = score;
  a.C = C; a.S = S;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.point0 = (uint32_t)point0;
  a.df = (T)(df > 0.0 ? df : 0.0);
  if (C <= kRegC)
    hipLaunchKernelGGL((mc_softmax_kernel<T, true>), dim3((unsigned)Tn), dim3(256), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((mc_softmax_kernel<T, false>), dim3((unsigned)Tn), dim3(256), 0, ctx->stream, a);
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));   // labels_h is borrowed for the call
  return SMN_OK;
}

bool rng_range_ok(int64_t point0, int64_t npoints, int64_t S) {
  return point0 >= 0 && npoints > 0 && npoints <= 0x7fffffff && point0 + npoints <= ((int64_t)1 << 32) && S > 0 &&
         S <= ((int64_t)1 << 32);
}

}  // namespace

extern "C" int smn_kernel_conv_diag(smn_ctx* ctx, int dtype, int kind, int act, int num_hiddens, double w_std, double b_std,
                                    double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                    void* diag_d) {
  if (!ctx || !x_d || !diag_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "Unsupported act %d", act);
  if (n <= 0 || H <= 0 || W <= 0 || C <= 0 || num_hiddens < 0 || (kind == 1 && num_hiddens == 0))
    return smn_fail(ctx, SMN_EINVAL, "smn_kernel_conv_diag: bad sizes");
  if (kind == 0) return cnn_diag(ctx, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, diag_d);
  if (kind == 1) return conv_resnet_diag(ctx, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, diag_d);
  return smn_fail(ctx, SMN_EINVAL, "smn_kernel_conv_diag: kind must be 0 (smn_kernel_cnn) or 1 (smn_kernel_conv_resnet)");
}

extern "C" int smn_svsp_moments(smn_ctx* ctx, int dtype, const void* k_zz_d, const void* k_zt_d, const void* ktt_diag_d,
                                const void* q_mu_d, const void* q_var_d, int64_t I, int64_t T, int64_t C, double eps,
                                void* mean_d, void* var_d, int* info_h, int64_t* nonpos_h) {
  if (!ctx || !k_zz_d || !k_zt_d || !ktt_diag_d || !q_mu_d || !q_var_d || !mean_d || !var_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (I <= 0 || T <= 0 || C <= 0 || C > 65535 * kMomC || I > 65535 || !(eps >= 0.0))
    return smn_fail(ctx, SMN_EINVAL, "smn_svsp_moments: bad sizes (at most 65535 inducing points) or eps < 0");
  const double* kzz = static_cast<const double*>(k_zz_d);
  const double* qm = static_cast<const double*>(q_mu_d);
  const double* qv = static_cast<const double*>(q_var_d);
  return by_dtype(dtype, [&](auto e) {   // (T is the number of test points here)
    return moments_t<decltype(e)>(ctx, kzz, k_zt_d, ktt_diag_d, qm, qv, I, T, (int)C, eps, mean_d, var_d, info_h, nonpos_h);
  });
}

extern "C" int smn_mc_softmax(smn_ctx* ctx, int dtype, const void* mean_d, const void* sigma_d, const int* labels_h, int64_t T,
                              int64_t C, int64_t S, double df, uint64_t seed, int64_t point0, const void* noise_d, void* ll_d,
                              void* pred_d, void* score_d) {
  if (!ctx || !mean_d || !sigma_d || !labels_h || !ll_d || !pred_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (C <= 0 || C > kMaxC) return smn_fail(ctx, SMN_EINVAL, "smn_mc_softmax: 1 <= C <= %d classes", kMaxC);
  if (!rng_range_ok(point0, T, S)) return smn_fail(ctx, SMN_EINVAL, "smn_mc_softmax: bad sizes (point indices and draws are 32-bit counter words)");
  if (df != df) return smn_fail(ctx, SMN_EINVAL, "smn_mc_softmax: df is NaN");
  for (int64_t i = 0; i < T; ++i)
    if (labels_h[i] < 0 || labels_h[i] >= C)
      return smn_fail(ctx, SMN_EINVAL, "smn_mc_softmax: label %d of point %lld is outside [0, %lld)", labels_h[i], (long long)i, (long long)C);
  double* ll = static_cast<double*>(ll_d);
  int* pred = static_cast<int*>(pred_d);
  double* score = static_cast<double*>(score_d);
  return by_dtype(dtype, [&](auto e) {
    return mc_softmax_t<decltype(e)>(ctx, mean_d, sigma_d, labels_h, T, (int)C, S, df, seed, point0, noise_d, ll, pred, score);
  });
}

extern "C" int smn_rng_variates(smn_ctx* ctx, int dtype, uint64_t seed, double df, int64_t point0, int64_t npoints, int64_t C,
                                int64_t S, void* out_d) {
  if (!ctx || !out_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (C <= 0 || C > kMaxC) return smn_fail(ctx, SMN_EINVAL, "smn_rng_variates: 1 <= C <= %d classes", kMaxC);
  if (!rng_range_ok(point0, npoints, S) || df != df)
    return smn_fail(ctx, SMN_EINVAL, "smn_rng_variates: bad sizes (point indices and draws are 32-bit counter words)");
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const dim3 grid((unsigned)npoints, (unsigned)((C + 3) / 4));
  const double dfe = df > 0.0 ? df : 0.0;
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(rng_variates_kernel<T>, grid, dim3(256), 0, ctx->stream, k0, k1, (T)dfe, (uint32_t)point0, (int)C, S, static_cast<T*>(out_d));
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

extern "C" int smn_debug_philox(smn_ctx* ctx, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctx || !ctr || !key || !out) return SMN_EINVAL;
  SMN_ENTER(ctx);
  void* wv = nullptr;
  SMN_TRY(smn_workspace(ctx, 11, 16, &wv));
  hipLaunchKernelGGL(philox_kernel, dim3(1), dim3(1), 0, ctx->stream, U4{ctr[0], ctr[1], ctr[2], ctr[3]}, key[0], key[1], static_cast<uint32_t*>(wv));
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipMemcpyAsync(out, wv, 16, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}
