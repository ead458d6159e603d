// cnn_grad.hip — analytic hyper-parameter gradients of the log-marginal likelihood for the conv-NNGP kernel of cnn.hip
// (experiments/nt_kernels.py:34-45), the conv counterpart of grad.hip: what objax.GradValues(model.loss, vars) supplies to
// experiments/regression/train.py:61-67 when the kernel is get_cnn_kernel.
//
// With K~ = K(w, b, lw) + eps I, alpha = K~^-1 y and G = coef * alpha alpha^T - K~^-1 (grad.hip:1-18) the four terms are
// sum_nm G_nm dK~_nm/d theta.  For one image pair (n, m) the forward-mode state is three H x W maps (K, Kw = dK/dw^2,
// Kb = dK/db^2), starting from (K0, 0, 0); per image the diagonal has (q, qw, qb), starting from (q0, 0, 0).  Per layer
// (box = 3x3 zero-padded box sum):
//   Conv:  Kw <- box(K)/9 + w^2 box(Kw)/9     Kb <- 1 + w^2 box(Kb)/9     K <- w^2 box(K)/9 + b^2      (same for q, qw, qb)
//   Act:   (o, phi_A, phi_qi, phi_qj) per pixel (grad.hip:13-18);  Kw <- phi_A Kw + phi_qi qw_n + phi_qj qw_m,  Kb likewise
//          with qb;  K <- o.  Diagonal: qw <- (d o / d q) qw, qb <- (d o / d q) qb, q <- o.
//   Flatten + Dense:  K_nm = lw^2 mean K,  dK_nm/dw^2 = lw^2 mean Kw,  dK_nm/db^2 = lw^2 mean Kb.
//
// Per-image tables.  Both activations factor the same way: with ra = 1/sqrt(q) (ReLU; 0 where q <= 0) or 1/sqrt(1 + 2q) (erf)
//   ReLU:  phi_qi = sqrt(1 - c^2) sqrt(q_i q_j) / (4 pi q_i) = [sqrt(1 - c^2) / (4 pi ra_i ra_j)] * ra_i^2
//   Erf:   phi_qi = -(2/pi) s / (sqrt(1 - s^2) (1 + 2 q_i))  = [-(2/pi) s / sqrt(1 - s^2)]       * ra_i^2
// so phi_qi qw_n + phi_qj qw_m = [pair factor] * (ra_n^2 qw_n + ra_m^2 qw_m): THREE fields per image, layer and pixel --
// ra, ra^2 qw, ra^2 qb -- where grad.hip keeps five per row.  The forward pair kernel is bound by streaming its one table
// out of L2 (cnn.hip), so the fewer the better; sqrt(q_i q_j) is 1 / (ra_i ra_j), one reciprocal, as in the forward kernel
// (act_factors of cnn_pairs.hpp, which also holds the wave's LDS map, the K0 phase, the pair order and the per-image helpers).
// A pixel whose variance is exactly zero (an all-zero neighbourhood with b_std = 0) has ra = 0 and so contributes no q-side
// term: the map is not differentiable there, and 0 * inf must not reach the sums.
#include <algorithm>
#include <cmath>

#include "cnn_pairs.hpp"
#include "internal.hpp"
#include "nngp_math.hpp"

namespace {

using namespace smn_cnn;

constexpr int kCgFields = 3;   // ra, ra^2 dq/dw^2, ra^2 dq/db^2
constexpr int kCgMaxHW = SMN_CNN_GRAD_MAX_PIXELS;

// One workgroup per image (fp64 arithmetic): tab[((img * L + l) * 3 + f) * HW + p] for the pair kernel, and
// dexact[img * 3 + {0, 1, 2}] = the exact K(img, img), dK/dw^2, dK/db^2 (last Dense included).
template <typename T>
__global__ void __launch_bounds__(256) cgrad_q_kernel(const T* __restrict__ x, ConvProg p, T* __restrict__ tab,
                                                      double* __restrict__ dexact) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, W = p.W, HW = H * W, PW = W + 2, PSZ = (H + 2) * PW;
  double* maps = reinterpret_cast<double*>(smem);   // (q, qw, qb) x ping-pong: six padded maps
  const int64_t img = blockIdx.x;
  for (int i = threadIdx.x; i < 6 * PSZ; i += blockDim.x) maps[i] = 0.0;
  __syncthreads();
  q0_into_map(x + img * HW * p.C, HW, W, PW, p.C, maps);
  __syncthreads();
  double* cur = maps;
  double* nxt = maps + 3 * PSZ;
  for (int l = 0; l < p.layers; ++l) {
    for (int px = threadIdx.x; px < HW; px += blockDim.x) {
      const int h = px / W, w = px % W;
      double bs[3];
#pragma unroll
      for (int f = 0; f < 3; ++f) bs[f] = box9(cur + f * PSZ + h * PW + w, PW);
      const double qt = p.w2 * bs[0] / 9.0 + p.b2;
      const double qw = bs[0] / 9.0 + p.w2 * bs[1] / 9.0;
      const double qb = 1.0 + p.w2 * bs[2] / 9.0;
      const DiagAct d = diag_act(p.act, qt);
      const double ra2 = p.act == 0 ? (qt > 0.0 ? 1.0 / qt : 0.0) : 1.0 / (1.0 + 2.0 * qt);
      T* t = tab + ((img * p.layers + l) * kCgFields) * HW + px;
      t[0] = (T)d.ra;
      t[HW] = (T)(ra2 * qw);
      t[2 * HW] = (T)(ra2 * qb);
      const int o = (h + 1) * PW + w + 1;
      nxt[o] = d.qa;
      nxt[PSZ + o] = d.dq * qw;
      nxt[2 * PSZ + o] = d.dq * qb;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  double* red = maps + 6 * PSZ;   // 3 x 256 doubles behind the maps
  for (int f = 0; f < 3; ++f) {
    const double k = block_mean(cur + f * PSZ, H, W, PW, p.lw2, red + f * 256);
    if (threadIdx.x == 0) dexact[img * 3 + f] = k;
  }
}

template <typename T>
struct CGradArgs {
  PairArgs<T> pa;          // x1 = x2 = the images, R1 = R2 = the tables above, the pair order; diag / out are not used
  const double* dexact;    // [n][3]
  const T* nkinv; int64_t ldki;   // -K~^-1 (lower triangle read)
  const T* alpha;
  double coef;
  double* partial;         // [gridDim.x * 4 waves][4]
  int nc;                  // MULTI forms: alpha is [n, nc] row-major
};

// Workgroups per CU a form is compiled for.  The state is three values per owned pixel: 16 pixels in fp64 are 96 VGPRs
// before any temporary, so the 1024-pixel form takes the 256 registers of two waves per SIMD; the small forms fit in 128.
#ifndef SMN_CGRAD_OCC16
#define SMN_CGRAD_OCC16 2
#endif
#ifndef SMN_CGRAD_OCC4
#define SMN_CGRAD_OCC4 4
#endif
template <typename T>
constexpr int cgrad_occ(int np) {
  return np <= 4 ? SMN_CGRAD_OCC4 : SMN_CGRAD_OCC16;
}

// The general LDS-map form of conv_pair_kernel (cnn.hip) carrying (K, Kw, Kb): one wave per image pair of the lower triangle,
// PairWalk order, ONE padded map per wave (WaveMap).  A layer takes the box sum of K through the map, then reuses the map for
// Kw and for Kb, so the LDS footprint is the forward kernel's.  Per-element arithmetic in T, the four sums in double, one
// partial per wave.
// MULTI (the rank-C form, MultiSPR): G_nm = coef sum_c A_nc A_mc + C (-K~^-1)_nm with A = alpha [n, nc], formed once per pair
// BEHIND the layer loop from wave-uniform rows of A, so nothing is added to what lives across the loop; nc = 1 gives the
// single-column form's bits.
template <typename T, int ACT, int NP, bool EXACT, bool MULTI = false>
__global__ void __launch_bounds__(256, cgrad_occ<T>(NP)) cgrad_pair_kernel(CGradArgs<T> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const PairArgs<T>& a = g.pa;
  const ConvProg& p = a.prog;
  const int HW = p.H * p.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  WaveMap<T, NP, EXACT> wm(smem, p.H, p.W, lane, wave);
  auto pix = [&](int i) { return wm.pix(i); };
  // (off0 is re-read in the ragged forms too, where nothing uses it: without it the erf 1024-pixel ragged fp64 form spills 1508
  // bytes per lane, with it 1500: profiles/r11_cnn_shared.txt)
  auto box = [&](T (&v)[NP]) { wm.reread_off0(); wm.box(v); };
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2, inv9 = (T)(1.0 / 9.0);
  const T inv_c = (T)(1.0 / p.C), lw2_hw = (T)(p.lw2 / HW), coef = (T)g.coef;
  constexpr int KB = NP < 4 ? NP : 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum G dK/dw^2, sum G dK/db^2, sum G K, tr G (wave-uniform)
  PairWalk<T> walk(a, wave);
  int64_t n, m;
  while (walk.next(n, m)) {
    wm.reread_lane();
    T k[NP], kw[NP], kb[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) kw[i] = kb[i] = T(0);
    load_k0<KB, false>(a.x1 + n * HW * p.C, a.x2 + m * HW * p.C, p.C, inv_c, pix, k);
    for (int l = 0; l < p.layers; ++l) {
      const T* t1 = a.R1 + (n * p.layers + l) * kCgFields * HW;
      const T* t2 = a.R2 + (m * p.layers + l) * kCgFields * HW;
      box(k);
      if (l > 0) {   // in the first layer Kw = Kb = 0 and so are their box sums
        box(kw);
        box(kb);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int px = pix(i);
        const T rr = t1[px] * t2[px];
        const T uw = t1[HW + px] + t2[HW + px], ub = t1[2 * HW + px] + t2[2 * HW + px];
        const T kt = fma(w2_9, k[i], b2);
        const T kwt = fma(w2_9, kw[i], k[i] * inv9);
        const T kbt = fma(w2_9, kb[i], T(1));
        T dA, tq;
        act_factors<T, ACT>(kt, rr, k[i], dA, tq);
        kw[i] = fma(dA, kwt, tq * uw);
        kb[i] = fma(dA, kbt, tq * ub);
        // the table loads of four pixels in flight at a time: hoisted for all sixteen they cost more registers than the state
        if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
    // Flatten (mean over pixels) + last Dense, then the contraction with G_nm
    T s[3] = {T(0), T(0), T(0)};
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool ok = wm.own(i);
      s[0] += ok ? kw[i] : T(0);
      s[1] += ok ? kb[i] : T(0);
      s[2] += ok ? k[i] : T(0);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
      s[q] *= lw2_hw;
    }
    const bool dg = n == m;
    if (dg) {   // the exact per-image values, as cnn.hip does for K(n, n)
      s[0] = (T)g.dexact[n * 3 + 1];
      s[1] = (T)g.dexact[n * 3 + 2];
      s[2] = (T)g.dexact[n * 3 + 0];
    }
    T gv;
    if (MULTI) {
      gv = (T)g.nc * g.nkinv[n * g.ldki + m];
      const T* rn = g.alpha + n * g.nc;
      const T* rm = g.alpha + m * g.nc;
      for (int c = 0; c < g.nc; ++c) gv = fma(coef * rn[c], rm[c], gv);
    } else {
      gv = fma(coef * g.alpha[n], g.alpha[m], g.nkinv[n * g.ldki + m]);
    }
    const T gm = dg ? gv : T(2) * gv;   // the upper triangle is the mirror image
    acc[0] += (double)(gm * s[0]);
    acc[1] += (double)(gm * s[1]);
    acc[2] += (double)(gm * s[2]);
    if (dg) acc[3] += (double)gv;
  }
  if (lane == 0) {
    double* out = g.partial + ((int64_t)blockIdx.x * 4 + wave) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = acc[q];
  }
}

// Second stage: fixed-order sum of the per-wave partials (bitwise reproducible), as grad_reduce_kernel.
__global__ void __launch_bounds__(256) cgrad_reduce_kernel(const double* __restrict__ partial, int64_t count,
                                                           double* __restrict__ out) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t = tid; t < count; t += 256)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += partial[t * 4 + q];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4) out[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// Launch one form, in the tiled pair order where tiled_pair_grid takes it.  The tile height follows from the occupancy this
// kernel compiles to (2 workgroups per CU for the 1024-pixel forms: 8 rows where the forward kernel has 16), not from the
// forward kernel's.  *blocks_io: the grid asked for / launched (at most max_blocks, the size of the partials).
template <typename T, typename K>
int cgrad_launch_form(smn_ctx* ctx, K kern, CGradArgs<T> g, int64_t* blocks_io, int64_t max_blocks, size_t lds) {
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  tiled_pair_grid(resident_blocks(ctx, kern, lds), g.pa.npairs, max_blocks, blocks_io, &g.pa.tile_bn);
  ProfScope ps(ctx, PROF_MISC, ctx->stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)*blocks_io), dim3(256), lds, ctx->stream, g);
  return SMN_OK;
}

template <typename T, int ACT>
int cgrad_launch(smn_ctx* ctx, const CGradArgs<T>& g, int64_t* blocks_io, int64_t max_blocks, size_t lds, int64_t hw, bool multi) {
  const bool w64 = 64 % g.pa.prog.W == 0;
#define CGRAD_CASE(NP)                                                                                               \
  if (hw <= 64 * NP && multi) {                                                                                      \
    if (hw == 64 * NP && w64)                                                                                        \
      return cgrad_launch_form<T>(ctx, cgrad_pair_kernel<T, ACT, NP, true, true>, g, blocks_io, max_blocks, lds);    \
    return cgrad_launch_form<T>(ctx, cgrad_pair_kernel<T, ACT, NP, false, true>, g, blocks_io, max_blocks, lds);     \
  }                                                                                                                  \
  if (hw <= 64 * NP) {                                                                                               \
    if (hw == 64 * NP && w64)                                                                                        \
      return cgrad_launch_form<T>(ctx, cgrad_pair_kernel<T, ACT, NP, true>, g, blocks_io, max_blocks, lds);          \
    return cgrad_launch_form<T>(ctx, cgrad_pair_kernel<T, ACT, NP, false>, g, blocks_io, max_blocks, lds);           \
  }
  CGRAD_CASE(1)
  CGRAD_CASE(4)
  CGRAD_CASE(16)
#undef CGRAD_CASE
  return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_cnn_grad_terms: H*W > %d", kCgMaxHW);
}

template <typename T>
int cgrad_terms_t(smn_ctx* ctx, int act, int layers, double w_std, double b_std, double last_w_std, const void* x_d,
                  int64_t n, int64_t H, int64_t W, int64_t C, const void* nkinv, int64_t ldki, const void* alpha, double coef,
                  double out_h[4], int nc = 0) {   // nc > 0: the rank-C form, alpha [n, nc]
  const ConvProg p = make_prog(act, layers, H, W, C, w_std, b_std, last_w_std);
  const int64_t HW = H * W;
  const size_t psz = (size_t)(H + 2) * (W + 2);
  const size_t lds_q = (6 * psz + 3 * 256) * sizeof(double);
  const size_t lds_p = wave_map_lds_bytes<T>(H, W);
  if (lds_q > 160 * 1024 || lds_p > 160 * 1024)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_cnn_grad_terms: image %lldx%lld too large for the on-chip maps", (long long)H,
                    (long long)W);
  const int64_t npairs = n * (n + 1) / 2;
  int64_t blocks = (npairs + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  const int64_t max_blocks = std::max<int64_t>(256 * 8, (int64_t)ctx->num_cu * 8);
  // doubles first (8-byte aligned): dexact [n][3], partial [max_blocks * 4][4], out [4]; then the tables [n][L][3][HW] in T
  const size_t nd = (size_t)n * 3 + (size_t)max_blocks * 16 + 4;
  const size_t ntab = (size_t)n * (size_t)(layers > 0 ? layers : 1) * kCgFields * (size_t)HW;
  void* wsv = nullptr;
  SMN_TRY(smn_workspace(ctx, 4, sizeof(double) * nd + sizeof(T) * ntab, &wsv));
  double* dexact = static_cast<double*>(wsv);
  double* partial = dexact + (size_t)n * 3;
  double* out_d = partial + (size_t)max_blocks * 16;
  T* tab = reinterpret_cast<T*>(out_d + 4);
  {
    ProfScope ps(ctx, PROF_PREP, ctx->stream);
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(cgrad_q_kernel<T>), lds_q));
    hipLaunchKernelGGL(cgrad_q_kernel<T>, dim3((unsigned)n), dim3(256), lds_q, ctx->stream, static_cast<const T*>(x_d), p, tab,
                       dexact);
  }
  SMN_CHECK_LAUNCH(ctx);
  CGradArgs<T> g;
  g.pa.x1 = g.pa.x2 = static_cast<const T*>(x_d);
  g.pa.R1 = g.pa.R2 = tab;
  g.pa.diag = nullptr;
  g.pa.n1 = g.pa.n2 = n;
  g.pa.symmetric = 1; g.pa.mirror = 0;
  g.pa.prog = p;
  g.pa.out = nullptr; g.pa.ldo = 0;
  g.pa.npairs = npairs;
  g.pa.tile_bn = 0;
  g.dexact = dexact;
  g.nkinv = static_cast<const T*>(nkinv); g.ldki = ldki;
  g.alpha = static_cast<const T*>(alpha);
  g.nc = nc > 0 ? nc : 1;
  g.coef = coef;
  g.partial = partial;
  SMN_TRY(act == SMN_ACT_RELU ? (cgrad_launch<T, 0>(ctx, g, &blocks, max_blocks, lds_p, HW, nc > 0))
                              : (cgrad_launch<T, 1>(ctx, g, &blocks, max_blocks, lds_p, HW, nc > 0)));
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(cgrad_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, partial, blocks * 4, out_d);
  SMN_CHECK_LAUNCH(ctx);
  double s[4];
  SMN_HIP(ctx, hipMemcpyAsync(s, out_d, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out_h[0] = s[0] * 2.0 * w_std;                          // d/dw_std = 2 w d/dw^2
  out_h[1] = b_std == 0.0 ? 0.0 : s[1] * 2.0 * b_std;     // (the sum is finite by construction; 0 stays an exact 0)
  out_h[2] = s[2] * 2.0 / last_w_std;                     // K = lw^2 K_L  =>  dK/dlw = 2 K / lw
  out_h[3] = s[3];                                        // dK~/deps = I
  return SMN_OK;
}

int cgrad_check(smn_ctx* ctx, const char* who, int dtype, int act, int num_hiddens, double last_w_std, int64_t n, int64_t H,
                int64_t W, int64_t C) {
  SMN_TRY(conv_check(ctx, who, dtype, act, num_hiddens, n, H, W, C, kCgMaxHW));
  if (!(last_w_std != 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: bad hyper-parameters", who);
  return SMN_OK;
}

// smn_kernel_cnn_grad_terms (multi = false: alpha [n], the single-output kernel forms) / smn_kernel_cnn_grad_terms_multi (the
// rank-C contraction: alpha_d [n, c] row-major, G = coef A A^T - c K~^-1)
int cnn_grad_terms(smn_ctx* ctx, const char* who, bool multi, int dtype, int act, int num_hiddens, double w_std, double b_std,
                   double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, const void* neg_kinv_d,
                   int64_t ldkinv, const void* alpha_d, int64_t c, double coef, double terms_h[4]) {
  if (!ctx || !x_d || !neg_kinv_d || !alpha_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(cgrad_check(ctx, who, dtype, act, num_hiddens, last_w_std, n, H, W, C));
  if (c < 1) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes", who);
  SMN_CHECK_LD(ctx, who, ldkinv, n);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  const int nc = multi ? (int)c : 0;
  return by_dtype(dtype, [&](auto e) {
    return cgrad_terms_t<decltype(e)>(ctx, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, neg_kinv_d, ldkinv, alpha_d,
                                 coef, terms_h, nc);
  });
}

// smn_spr_cnn_loss_grad / smn_spr_cnn_loss_grad_multi.  Fused: the forward conv build of the lower triangle straight into the
// factorisation workspace (smn_kernel_cnn), one factorisation of [[K~], [I], [Y^T]] for the c target columns that share K~
// (heads.hip posterior_from_images: alpha, -K~^-1, quad, logdet), then the contraction above over the image pairs.
int spr_cnn_loss_grad(smn_ctx* ctx, const char* who, bool multi, int dtype, int act, int num_hiddens, double w_std, double b_std,
                      double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, const void* y_d, int64_t c,
                      double eps_abs, double df, double scale, double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h,
                      double terms_h[4]) {
  if (!ctx || !x_d || !y_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(cgrad_check(ctx, who, dtype, act, num_hiddens, last_w_std, n, H, W, C));
  if (c < 1) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes", who);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  if (df > 0.0 && !(scale > 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: scale must be > 0", who);
  const BuildSpec spec{dtype, SMN_NET_MLP, act, num_hiddens, w_std, b_std, last_w_std};   // (net: not read by the conv build)
  Posterior p;
  SMN_TRY(posterior_from_images(ctx, spec, x_d, n, H, W, C, y_d, c, eps_abs, &p));
  const double tot = publish_head(p, c, multi, n, df, scale, nullptr, quad_h, quad_cols_h, logdet_h, info_h, terms_h);
  if (p.info != 0) return SMN_OK;
  return cnn_grad_terms(ctx, multi ? "smn_kernel_cnn_grad_terms_multi" : "smn_kernel_cnn_grad_terms", multi, dtype, act,
                        num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, p.ninv, p.ldinv, p.alpha, c,
                        lml_coef(df, scale, tot, n, c), terms_h);
}

}  // namespace

extern "C" int smn_kernel_cnn_grad_terms(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                         double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                         const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, double coef,
                                         double terms_h[4]) {
  return cnn_grad_terms(ctx, "smn_kernel_cnn_grad_terms", false, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W,
                        C, neg_kinv_d, ldkinv, alpha_d, 1, coef, terms_h);
}

extern "C" int smn_spr_cnn_loss_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                     double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                     const void* y_d, double eps_abs, double df, double scale, double* quad_h,
                                     double* logdet_h, int* info_h, double terms_h[4]) {
  return spr_cnn_loss_grad(ctx, "smn_spr_cnn_loss_grad", false, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C,
                           y_d, 1, eps_abs, df, scale, quad_h, nullptr, logdet_h, info_h, terms_h);
}

extern "C" int smn_kernel_cnn_grad_terms_multi(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                               double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                               const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, int64_t c,
                                               double coef, double terms_h[4]) {
  return cnn_grad_terms(ctx, "smn_kernel_cnn_grad_terms_multi", true, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H,
                        W, C, neg_kinv_d, ldkinv, alpha_d, c, coef, terms_h);
}

extern "C" int smn_spr_cnn_loss_grad_multi(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                           double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                           const void* y_d, int64_t c, double eps_abs, double df, double scale, double* quad_h,
                                           double* quad_cols_h, double* logdet_h, int* info_h, double terms_h[4]) {
  return spr_cnn_loss_grad(ctx, "smn_spr_cnn_loss_grad_multi", true, dtype, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H,
                           W, C, y_d, c, eps_abs, df, scale, quad_h, quad_cols_h, logdet_h, info_h, terms_h);
}
