// cnn_input_grad.hip — reverse mode of the conv-NNGP kernel of cnn.hip with respect to its input images: what
// objax.GradValues(model.loss, model.vars()) supplies for SVSP.inducing_variable (spax/models.py:21,31;
// experiments/classification/train.py:205).  Given a symmetric seed g = d loss / d K over n images,
//     gx_i = sum_ab g_ab dK_ab / dx_i        for the first n_grad images (the rest are partners only).
//
// Notation of cnn_grad.hip (box = 3x3 zero-padded box sum, self-adjoint).  Forward, per layer l = 1..L and pair (n, m):
//   kt_l = w^2 box(k_{l-1})/9 + b^2,  k_l = phi(kt_l, qt_l^n, qt_l^m);   per image  qt_l = w^2 box(q_{l-1})/9 + b^2,  q_l = phi_diag(qt_l);
//   k_0 = x_n.x_m / C,  q_0 = |x_n|^2 / C per pixel;   K_nm = lw^2 mean k_L,  K_nn = lw^2 mean q_L (the exact diagonal).
// phi_A = d phi / d kt and phi_qi = [pair factor] * ra_i^2 are the factors cnn_grad.hip evaluates (act_factors of
// cnn_pairs.hpp; same zero-variance rule: ra = 0 gives no variance-side term, so 0 * inf never arises).
//
// Pair pass (cig_pair_kernel), owner i < n_grad against a partner m != i:
//   kbar_L = 2 g_im lw^2 / HW  (2: the mirror entry);  for l = L..1:  qtbar_i^l += phi_qi(l) kbar_l,  kbar_{l-1} = w^2 box(phi_A(l) kbar_l)/9;
//   gx_i[p,c] += kbar_0[p] x_m[p,c] / C.
// The partner's own variance-side term is not taken here: a pair of two differentiated images is visited once from each side.
// Per-image pass (cig_finish_kernel):  r = g_ii lw^2 / HW;  for l = L..1:  r = w^2 box(dq_l r + qtbar^l)/9;  gx_i += 2 x_i r / C.
//
// Work layout.  One wave per (owner, slice of its partner list); the partner list of an owner is cut into nsplit slices so
// that owners x nsplit fills the resident waves.  A lane owns NP pixels, with one padded LDS map per wave for the box sums
// (WaveMap of cnn_pairs.hpp).  The forward sweep of a pair leaves (phi_A, pair factor) per layer and pixel in the wave's own slab
// of global memory (2 L x 64 NP elements, written and read back by the same lane: no fence), the reverse sweep reads them back.
// The sums over partners (qtbar [L], gx [C] per pixel) are fp64 in the slice's own block of global memory, added to by the lane
// that owns the pixel in the fixed order of the partner list; the per-image pass adds the slices in order.  No floating-point
// atomics anywhere: two calls give the same bits.  Rows of the tables, the slab and the sums have 64 NP slots, one per lane and
// owned pixel whether the image has that pixel or not, so every global access of the pair kernel is unconditional and at
// lane + 64 i from a wave-uniform base (guarded accesses at computed offsets made the 16-pixel forms spill).  Memory beyond
// inputs and outputs: the per-image tables (n L 64 NP), one forward slab per resident wave, one sum block per slice -- nothing
// grows with n^2 HW.  DESIGN.md section 6d.
//
// The cross, multi-seed form for a fitted posterior's saliency maps (rows x1 against fixed partners x2, all seeds from one
// reverse sweep per pair) follows the symmetric one below and shares its per-image kernels; DESIGN.md section 6m.
#include <algorithm>
#include <cmath>

#include "cnn_pairs.hpp"
#include "internal.hpp"
#include "nngp_math.hpp"

namespace {

using namespace smn_cnn;

constexpr int kCigMaxHW = SMN_CNN_GRAD_MAX_PIXELS;

// One workgroup per image (fp64 arithmetic): ra[(img * L + l) * HWP + p] (1/sqrt(qt), 0 where qt <= 0; erf: 1/sqrt(1 + 2 qt))
// for all images -- rows of HWP = 64 NP entries, zero past the image, so that every lane of the pair kernel has a slot of its
// own for each of its NP pixels --, dq[(img * L + l) * HW + p] = d phi_diag / d qt for the differentiated ones.
template <typename T>
__global__ void __launch_bounds__(256) cig_q_kernel(const T* __restrict__ x, ConvProg p, int64_t n_grad, int HWP,
                                                    T* __restrict__ ra_tab, double* __restrict__ dq_tab) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, W = p.W, HW = H * W, PW = W + 2, PSZ = (H + 2) * PW;
  double* maps = reinterpret_cast<double*>(smem);   // two padded maps, ping-pong
  const int64_t img = blockIdx.x;
  for (int i = threadIdx.x; i < 2 * PSZ; i += blockDim.x) maps[i] = 0.0;
  __syncthreads();
  q0_into_map(x + img * HW * p.C, HW, W, PW, p.C, maps);
  __syncthreads();
  double* cur = maps;
  double* nxt = maps + PSZ;
  for (int l = 0; l < p.layers; ++l) {
    for (int px = threadIdx.x; px < HW; px += blockDim.x) {
      const int h = px / W, w = px % W;
      const DiagAct d = diag_act(p.act, p.w2 * box9(cur + h * PW + w, PW) / 9.0 + p.b2);
      ra_tab[(img * p.layers + l) * HWP + px] = (T)d.ra;
      if (img < n_grad) dq_tab[(img * p.layers + l) * HW + px] = d.dq;
      nxt[(h + 1) * PW + w + 1] = d.qa;
    }
    for (int px = HW + threadIdx.x; px < HWP; px += blockDim.x) ra_tab[(img * p.layers + l) * HWP + px] = T(0);
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
}

template <typename T>
struct CigArgs {
  const T* x;              // [n][HW][C]
  const T* ra;             // [n][L][HWP], HWP = 64 NP
  const T* g; int64_t ldg; // the seed; lower triangle read
  int64_t n, items;        // items = n_grad * nsplit
  int nsplit; int64_t per; // slices per owner, partners per slice
  ConvProg prog;
  T* fwd;                  // [gridDim.x * 4 waves][L][2][HWP]: (phi_A, pair factor) of the pair in flight
  double* part;            // [items][L + C][HWP]: qtbar per layer, then gx per channel
};

// Waves per SIMD a form is compiled for: the second __launch_bounds__ argument is the minimum number of waves per execution
// unit, and a workgroup of 256 threads puts one wave on each of a CU's four SIMDs, so here (and only for this block size) it
// is also the number of workgroups per CU.  The state is ONE value per owned pixel (the tangent kernel carries three), so the
// 1024-pixel form is 32 VGPRs of state in fp64; the LDS offsets and the temporaries of four pixels in flight come on top
// (170 VGPRs, no scratch: profiles/r10_cnn_input_grad.txt).
#ifndef SMN_CIG_OCC16
#define SMN_CIG_OCC16 2
#endif
#ifndef SMN_CIG_OCC4
#define SMN_CIG_OCC4 4
#endif
constexpr int cig_occ(int np) { return np <= 4 ? SMN_CIG_OCC4 : SMN_CIG_OCC16; }

template <typename T, int ACT, int NP>
__global__ void __launch_bounds__(256, cig_occ(NP)) cig_pair_kernel(CigArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvProg& p = a.prog;
  const int HW = p.H * p.W, L = p.layers, C = p.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int HWP = 64 * NP;                          // slots per row of the tables, the slab and the sums: lane + 64 i
  // one form per NP (never EXACT), and neither reread_lane() nor reread_off0(): either moves the 1024-pixel forms' registers
  WaveMap<T, NP, false> wm(smem, p.H, p.W, lane, wave);
  auto own = [&](int i) { return wm.own(i); };
  auto pix = [&](int i) { return wm.pix(i); };
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / C), lw2_hw2 = (T)(2.0 * p.lw2 / HW);
  constexpr int KB = NP < 4 ? NP : 4;
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave, nw = (int64_t)gridDim.x * 4;
  T* fwd = a.fwd + gw * (int64_t)(2 * L) * HWP + lane;   // this lane's slot of pixel i: + 64 i
  for (int64_t item = gw; item < a.items; item += nw) {
    const int64_t n = item / a.nsplit;
    const int64_t j0 = (item % a.nsplit) * a.per, j1 = min(j0 + a.per, a.n - 1);
    double* part = a.part + item * (int64_t)(L + C) * HWP + lane;
    for (int f = 0; f < L + C; ++f)
#pragma unroll
      for (int i = 0; i < NP; ++i) part[f * HWP + 64 * i] = 0.0;   // by the lane that adds to it below
    const T* xa = a.x + n * HW * C;
    for (int64_t j = j0; j < j1; ++j) {
      const int64_t m = j < n ? j : j + 1;   // the partner list of n: every image but n, in index order
      const T* xb = a.x + m * HW * C;
      const T gv = n > m ? a.g[n * a.ldg + m] : a.g[m * a.ldg + n];
      T k[NP];
      load_k0<KB, false>(xa, xb, C, inv_c, pix, k);
#pragma unroll
      for (int i = 0; i < NP; ++i) k[i] = own(i) ? k[i] : T(0);
      // forward sweep: (phi_A, pair factor) of every layer into the wave's slab
      for (int l = 0; l < L; ++l) {
        const T* t1 = a.ra + (n * L + l) * HWP + lane;
        const T* t2 = a.ra + (m * L + l) * HWP + lane;
        T* fl = fwd + l * 2 * HWP;
        wm.box(k);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const T rr = t1[64 * i] * t2[64 * i];
          T dA, tq;
          act_factors<T, ACT>(fma(w2_9, k[i], b2), rr, k[i], dA, tq);
          fl[64 * i] = dA;
          fl[HWP + 64 * i] = tq;
          if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // the table loads of four pixels in flight at a time
        }
      }
      // reverse sweep
      const T seed = gv * lw2_hw2;
#pragma unroll
      for (int i = 0; i < NP; ++i) k[i] = own(i) ? seed : T(0);
      for (int l = L - 1; l >= 0; --l) {
        const T* t1 = a.ra + (n * L + l) * HWP + lane;
        const T* fl = fwd + l * 2 * HWP;
        double* qb = part + l * HWP;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const T ra = t1[64 * i];
          qb[64 * i] += (double)(fl[HWP + 64 * i] * (ra * ra) * k[i]);
          k[i] *= fl[64 * i];
          if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        wm.box(k);
#pragma unroll
        for (int i = 0; i < NP; ++i) k[i] = own(i) ? k[i] * w2_9 : T(0);
      }
      for (int c = 0; c < C; ++c) {
        double* gp = part + (L + c) * HWP;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          gp[64 * i] += (double)(k[i] * xb[pix(i) * C + c] * inv_c);   // k is zero past the image
          if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
}

// Second stage and the per-image pass of one differentiated image by one workgroup: the slices of the pair pass (`mine`, one
// block of L + C rows of HWP sums per slice) added in slice order (bitwise reproducible), the reverse chain of the exact
// diagonal from r0 through two padded fp64 maps, the result in T.  dq_img [L][HW], x_img and gx_img [HW][C].
template <typename T>
__device__ __forceinline__ void cig_finish_image(const T* __restrict__ x_img, const ConvProg& p, double r0,
                                                 const double* __restrict__ dq_img, const double* __restrict__ mine, int nsplit,
                                                 int HWP, T* __restrict__ gx_img, char* smem) {
  const int H = p.H, W = p.W, HW = H * W, PW = W + 2, PSZ = (H + 2) * PW, L = p.layers, C = p.C;
  double* cur = reinterpret_cast<double*>(smem);
  double* nxt = cur + PSZ;
  const int64_t sstride = (int64_t)(L + C) * HWP;
  for (int i = threadIdx.x; i < 2 * PSZ; i += blockDim.x) cur[i] = 0.0;
  __syncthreads();
  for (int px = threadIdx.x; px < HW; px += blockDim.x) cur[(px / W + 1) * PW + px % W + 1] = r0;
  __syncthreads();
  for (int l = L - 1; l >= 0; --l) {
    for (int px = threadIdx.x; px < HW; px += blockDim.x) {
      double qs = 0.0;
      for (int s = 0; s < nsplit; ++s) qs += mine[s * sstride + (int64_t)l * HWP + px];
      const int o = (px / W + 1) * PW + px % W + 1;
      cur[o] = dq_img[l * HW + px] * cur[o] + qs;
    }
    __syncthreads();
    for (int px = threadIdx.x; px < HW; px += blockDim.x) {
      const int h = px / W, w = px % W;
      nxt[(h + 1) * PW + w + 1] = p.w2 * box9(cur + h * PW + w, PW) / 9.0;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  for (int e = threadIdx.x; e < HW * C; e += blockDim.x) {
    const int px = e / C, c = e % C;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += mine[k * sstride + (int64_t)(L + c) * HWP + px];
    const double r = cur[(px / W + 1) * PW + px % W + 1];
    gx_img[e] = (T)(s + 2.0 * (double)x_img[e] * r / C);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) cig_finish_kernel(const T* __restrict__ x, ConvProg p, const T* __restrict__ g, int64_t ldg,
                                                         const double* __restrict__ dq_tab, const double* __restrict__ part,
                                                         int nsplit, int HWP, T* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W, L = p.layers, C = p.C;
  const int64_t img = blockIdx.x;
  const double r0 = (double)g[img * ldg + img] * p.lw2 / HW;
  cig_finish_image<T>(x + img * HW * C, p, r0, dq_tab + img * L * HW, part + img * nsplit * (int64_t)(L + C) * HWP, nsplit, HWP,
                      gx + img * HW * C, smem);
}

template <typename T>
using CigKernel = void (*)(CigArgs<T>);

// The form for an image of hw pixels: 1, 4 or 16 pixels per lane.
template <typename T>
CigKernel<T> cig_form(int act, int64_t hw) {
  if (act == SMN_ACT_RELU) return hw <= 64 ? cig_pair_kernel<T, 0, 1> : hw <= 256 ? cig_pair_kernel<T, 0, 4> : cig_pair_kernel<T, 0, 16>;
  return hw <= 64 ? cig_pair_kernel<T, 1, 1> : hw <= 256 ? cig_pair_kernel<T, 1, 4> : cig_pair_kernel<T, 1, 16>;
}

template <typename T>
int cig_run(smn_ctx* ctx, int act, int layers, double w_std, double b_std, double last_w_std, const void* x_d, int64_t n,
            int64_t H, int64_t W, int64_t C, const void* g_d, int64_t ldg, int64_t n_grad, void* gx_d) {
  const ConvProg p = make_prog(act, layers, H, W, C, w_std, b_std, last_w_std);
  const int64_t HW = H * W;
  const int64_t HWP = HW <= 64 ? 64 : HW <= 256 ? 256 : 1024;   // 64 NP of the form cig_launch picks
  const size_t psz = (size_t)(H + 2) * (W + 2);
  const size_t lds_q = 2 * psz * sizeof(double);
  // H W <= 1024 bounds both: the padded map has at most 3 x 1026 elements (a 1 x 1024 image), so lds_p <= 4 x 4107 x 8 =
  // 128.3 KB and lds_q <= 48.1 KB of the CU's 160 KB, whatever the aspect ratio
  const size_t lds_p = wave_map_lds_bytes<T>(H, W);
  CigArgs<T> a;
  a.x = static_cast<const T*>(x_d);
  a.g = static_cast<const T*>(g_d); a.ldg = ldg;
  a.n = n;
  a.prog = p;
  const CigKernel<T> kern = cig_form<T>(act, HW);
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds_p));
  // the resident set this form compiles to decides how the partner lists are cut
  const int64_t resident = std::max<int64_t>(resident_blocks(ctx, kern, lds_p), ctx->num_cu) * 4;
  // owners x slices fills the resident waves once; never more slices than partners
  int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(resident / n_grad, n - 1));
  const int64_t per = n > 1 ? (n - 1 + nsplit - 1) / nsplit : 0;
  if (per > 0) nsplit = (n - 1 + per - 1) / per;   // no empty slice
  a.nsplit = (int)nsplit; a.per = per;
  a.items = n_grad * nsplit;
  const int64_t waves = std::min(resident, round_up(a.items, 4));
  // doubles first (8-byte aligned): dq [n_grad][L][HW], part [items][L + C][HWP]; then in T: ra [n][L][HWP], fwd [waves][L][2][HWP]
  const size_t lay = (size_t)(layers > 0 ? layers : 1);
  const size_t nd = (size_t)n_grad * lay * HW + (size_t)a.items * (size_t)(layers + C) * HWP;
  const size_t nt = (size_t)n * lay * HWP + (size_t)waves * 2 * lay * HWP;
  void* wsv = nullptr;
  SMN_TRY(smn_workspace(ctx, 4, sizeof(double) * nd + sizeof(T) * nt, &wsv));
  double* dq = static_cast<double*>(wsv);
  double* part = dq + (size_t)n_grad * lay * HW;
  T* ra = reinterpret_cast<T*>(part + (size_t)a.items * (size_t)(layers + C) * HWP);
  a.ra = ra;
  a.fwd = ra + (size_t)n * lay * HWP;
  a.part = part;
  {
    ProfScope ps(ctx, PROF_PREP, ctx->stream);
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(cig_q_kernel<T>), lds_q));
    hipLaunchKernelGGL(cig_q_kernel<T>, dim3((unsigned)n), dim3(256), lds_q, ctx->stream, a.x, p, n_grad, (int)HWP, ra, dq);
  }
  SMN_CHECK_LAUNCH(ctx);
  {
    ProfScope ps(ctx, PROF_MISC, ctx->stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)(waves / 4)), dim3(256), lds_p, ctx->stream, a);
  }
  SMN_CHECK_LAUNCH(ctx);
  {
    ProfScope ps(ctx, PROF_MISC, ctx->stream);
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(cig_finish_kernel<T>), lds_q));
    hipLaunchKernelGGL(cig_finish_kernel<T>, dim3((unsigned)n_grad), dim3(256), lds_q, ctx->stream, a.x, p, a.g, ldg, dq, part,
                       a.nsplit, (int)HWP, static_cast<T*>(gx_d));
  }
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}

// ---------------------------------------------------------------- the cross, multi-seed form (smn_kernel_cnn_input_grad_cross)
// Rows x1 [n1] against partners x2 [n2], which do not move, and S seeds at once: the c columns of alpha (mean seeds, g_s(r, j) =
// alpha[j, s], shared by all rows) and gbar (the variance seed, g(r, j) = gbar[r, j]).  The reverse sweep is linear in its seed, so
// a pair runs its forward sweep and ONE reverse sweep from the unit seed lw^2 / HW -- no mirror factor 2: a cross entry occurs
// once -- which yields khat_0[p] and, per layer, qhat_l[p] = pair factor ra_r^2 khat_l[p]; every seed then takes
//     qtbar_s^l += g_s qhat_l,      gx_s[p, ch] += g_s khat_0[p] x2_j[p, ch] / C
// in its own fp64 block of the slice (the product in T, the sum in fp64, in the order of the partner list).  The seed loop is
// the innermost one, inside groups of four pixels: the four values wait in registers while the seeds' blocks are read, added
// to and written back, so nothing of size S or NP x S lives in registers.  A seed's value is one wave-uniform load.
// Only the owner's variance-side term exists.  The per-image pass (cig_finish_image) runs once per row and seed; its r0 =
// gdiag[r] lw^2 / HW belongs to the variance seed alone.
// The cut of a row's partner list (nsplit, per) follows n1, n2, the form and the device, nothing else.  The sums are
// [seeds of the group][rows of the batch x nsplit][L + C][HWP] doubles, capped at min(256 MB, smn_debug_batch_bytes): above
// that the seeds go in groups -- one more pass over the pairs each, same cut, and a seed's sums never meet another seed's, so
// the bits do not depend on the budget or on which seeds share a call -- and, when one seed alone is too much, the rows in
// batches.  Rows computed alone need NOT carry the bits of the same rows in a larger call: n1 enters the cut.
template <typename T>
struct CigxArgs {
  const T* x1; const T* x2;       // [n1][HW][C], [n2][HW][C]
  const T* ra1; const T* ra2;     // [n1][L][HWP], [n2][L][HWP]
  const T* alpha; int c;          // mean seeds [n2][c]; c = 0 without them
  const T* gbar; int64_t ldg;     // variance seed [n1][ldg], or null: zero
  int64_t row0, n2, items;        // rows [row0, row0 + items / nsplit) of x1; items = rows * nsplit
  int nsplit; int64_t per;
  int s0, ns;                     // seeds s0 .. s0 + ns - 1 of the list: s < c the mean seed of output s, s == c the variance seed
  ConvProg prog;
  T* fwd;                         // [gridDim.x * 4 waves][L][2][HWP]
  double* part;                   // [ns][items][L + C][HWP]
};

template <typename T, int ACT, int NP>
__global__ void __launch_bounds__(256, cig_occ(NP)) cigx_pair_kernel(CigxArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvProg& p = a.prog;
  const int HW = p.H * p.W, L = p.layers, C = p.C;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int HWP = 64 * NP;
  WaveMap<T, NP, false> wm(smem, p.H, p.W, lane, wave);
  auto own = [&](int i) { return wm.own(i); };
  auto pix = [&](int i) { return wm.pix(i); };
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / C), lw2_hw = (T)(p.lw2 / HW);
  constexpr int KB = NP < 4 ? NP : 4;
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave, nw = (int64_t)gridDim.x * 4;
  const int64_t sstride = a.items * (int64_t)(L + C) * HWP;   // from one seed's blocks to the next seed's
  T* fwd = a.fwd + gw * (int64_t)(2 * L) * HWP + lane;
  for (int64_t item = gw; item < a.items; item += nw) {
    const int64_t r = a.row0 + item / a.nsplit;
    const int64_t j0 = (item % a.nsplit) * a.per, j1 = min(j0 + a.per, a.n2);
    double* part = a.part + item * (int64_t)(L + C) * HWP + lane;
    for (int s = 0; s < a.ns; ++s)
      for (int f = 0; f < L + C; ++f)
#pragma unroll
        for (int i = 0; i < NP; ++i) part[s * sstride + f * HWP + 64 * i] = 0.0;   // by the lane that adds to it below
    const T* xa = a.x1 + r * HW * C;
    for (int64_t j = j0; j < j1; ++j) {
      const T* xb = a.x2 + j * HW * C;
      auto seed = [&](int s) -> T {
        const int sid = a.s0 + s;
        return sid < a.c ? a.alpha[j * a.c + sid] : (a.gbar ? a.gbar[r * a.ldg + j] : T(0));
      };
      T k[NP];
      load_k0<KB, false>(xa, xb, C, inv_c, pix, k);
#pragma unroll
      for (int i = 0; i < NP; ++i) k[i] = own(i) ? k[i] : T(0);
      // forward sweep, as in cig_pair_kernel
      for (int l = 0; l < L; ++l) {
        const T* t1 = a.ra1 + (r * L + l) * HWP + lane;
        const T* t2 = a.ra2 + (j * L + l) * HWP + lane;
        T* fl = fwd + l * 2 * HWP;
        wm.box(k);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const T rr = t1[64 * i] * t2[64 * i];
          T dA, tq;
          act_factors<T, ACT>(fma(w2_9, k[i], b2), rr, k[i], dA, tq);
          fl[64 * i] = dA;
          fl[HWP + 64 * i] = tq;
          if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // one reverse sweep from the unit seed; every seed of the group takes its share of each group of four pixels
#pragma unroll
      for (int i = 0; i < NP; ++i) k[i] = own(i) ? lw2_hw : T(0);
      for (int l = L - 1; l >= 0; --l) {
        const T* t1 = a.ra1 + (r * L + l) * HWP + lane;
        const T* fl = fwd + l * 2 * HWP;
        double* qb = part + l * HWP;
#pragma unroll
        for (int i0 = 0; i0 < NP; i0 += KB) {
          T qh[KB];
#pragma unroll
          for (int u = 0; u < KB; ++u) {
            const int i = i0 + u;
            const T ra = t1[64 * i];
            qh[u] = fl[HWP + 64 * i] * (ra * ra) * k[i];
            k[i] *= fl[64 * i];
          }
          for (int s = 0; s < a.ns; ++s) {
            const T gv = seed(s);
            double* qs = qb + s * sstride;
#pragma unroll
            for (int u = 0; u < KB; ++u) qs[64 * (i0 + u)] += (double)(gv * qh[u]);
          }
          if (NP > 4) __builtin_amdgcn_sched_barrier(0);
        }
        wm.box(k);
#pragma unroll
        for (int i = 0; i < NP; ++i) k[i] = own(i) ? k[i] * w2_9 : T(0);
      }
      for (int c = 0; c < C; ++c) {
        double* gp = part + (L + c) * HWP;
#pragma unroll
        for (int i0 = 0; i0 < NP; i0 += KB) {
          T v[KB];
#pragma unroll
          for (int u = 0; u < KB; ++u) v[u] = k[i0 + u] * xb[pix(i0 + u) * C + c] * inv_c;   // k is zero past the image
          for (int s = 0; s < a.ns; ++s) {
            const T gv = seed(s);
            double* gs = gp + s * sstride;
#pragma unroll
            for (int u = 0; u < KB; ++u) gs[64 * (i0 + u)] += (double)(gv * v[u]);
          }
          if (NP > 4) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
}

// The per-image pass of row row0 + blockIdx.x and seed s0 + blockIdx.y of the group: mean seeds (sid < c) into gmean [n1][c],
// the variance seed into gvar [n1], which alone starts its chain from gdiag.
template <typename T>
__global__ void __launch_bounds__(256) cigx_finish_kernel(const T* __restrict__ x1, ConvProg p, const T* __restrict__ gdiag,
                                                          const double* __restrict__ dq_tab, const double* __restrict__ part,
                                                          int nsplit, int HWP, int64_t row0, int64_t items, int s0, int c,
                                                          T* __restrict__ gmean, T* __restrict__ gvar) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W, L = p.layers, C = p.C;
  const int64_t img = row0 + blockIdx.x;
  const int sid = s0 + (int)blockIdx.y;
  const double r0 = (sid >= c && gdiag) ? (double)gdiag[img] * p.lw2 / HW : 0.0;
  T* out = sid < c ? gmean + (img * c + sid) * HW * C : gvar + img * HW * C;
  const double* mine = part + ((int64_t)blockIdx.y * items + (int64_t)blockIdx.x * nsplit) * (int64_t)(L + C) * HWP;
  cig_finish_image<T>(x1 + img * HW * C, p, r0, dq_tab + img * L * HW, mine, nsplit, HWP, out, smem);
}

template <typename T>
using CigxKernel = void (*)(CigxArgs<T>);

template <typename T>
CigxKernel<T> cigx_form(int act, int64_t hw) {
  if (act == SMN_ACT_RELU) return hw <= 64 ? cigx_pair_kernel<T, 0, 1> : hw <= 256 ? cigx_pair_kernel<T, 0, 4> : cigx_pair_kernel<T, 0, 16>;
  return hw <= 64 ? cigx_pair_kernel<T, 1, 1> : hw <= 256 ? cigx_pair_kernel<T, 1, 4> : cigx_pair_kernel<T, 1, 16>;
}

constexpr size_t kCigxPartBytes = (size_t)256 << 20;   // the sums of one pass (or smn_debug_batch_bytes, if smaller)
constexpr int64_t kCigxMinPer = 8;                      // partners per slice, at least (fewer only when n2 is)

template <typename T>
int cigx_run(smn_ctx* ctx, int act, int layers, double w_std, double b_std, double last_w_std, const void* x1_d, int64_t n1,
             const void* x2_d, int64_t n2, int64_t H, int64_t W, int64_t C, const void* alpha_d, int64_t c, const void* gbar_d,
             int64_t ldg, const void* gdiag_d, void* gmean_d, void* gvar_d) {
  const ConvProg p = make_prog(act, layers, H, W, C, w_std, b_std, last_w_std);
  const int64_t HW = H * W;
  const int64_t HWP = HW <= 64 ? 64 : HW <= 256 ? 256 : 1024;
  const size_t lds_q = 2 * (size_t)(H + 2) * (W + 2) * sizeof(double);
  const size_t lds_p = wave_map_lds_bytes<T>(H, W);
  const CigxKernel<T> kern = cigx_form<T>(act, HW);
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds_p));
  const int64_t resident = std::max<int64_t>(resident_blocks(ctx, kern, lds_p), ctx->num_cu) * 4;
  // rows x slices fills the resident waves once, with slices of at least kCigxMinPer partners: every slice costs a block of
  // sums per seed that is cleared, added to and read back by the per-image pass, and at four partners per slice (16 rows of
  // 32 x 32 images against 1000 partners) that traffic, not the sweeps, was the call
  int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(resident / n1, (n2 + kCigxMinPer - 1) / kCigxMinPer));
  const int64_t per = (n2 + nsplit - 1) / nsplit;
  nsplit = (n2 + per - 1) / per;   // no empty slice
  // the seed list: mean seeds 0 .. cc - 1, the variance seed cc
  const int cc = alpha_d ? (int)c : 0;
  const int s_begin = gmean_d ? 0 : cc, s_end = gvar_d ? cc + 1 : cc;
  const size_t block = sizeof(double) * (size_t)(layers + C) * HWP;   // one seed's sums of one slice
  const size_t budget = std::max<size_t>(std::min(ctx->batch_bytes, kCigxPartBytes), block);
  const int64_t rows_b = std::max<int64_t>(1, std::min<int64_t>(n1, (int64_t)(budget / (block * (size_t)nsplit))));
  const int sg = (int)std::max<size_t>(1, std::min<size_t>((size_t)(s_end - s_begin), budget / (block * (size_t)(rows_b * nsplit))));
  const int64_t waves_max = std::min(resident, round_up(rows_b * nsplit, 4));
  // doubles first: dq [n1][L][HW], part [sg][rows_b nsplit][L + C][HWP]; then in T: ra1 [n1][L][HWP], ra2 [n2][L][HWP], fwd
  const size_t lay = (size_t)(layers > 0 ? layers : 1);
  const size_t n_part = (size_t)sg * (size_t)(rows_b * nsplit) * (size_t)(layers + C) * HWP;
  const size_t nd = (size_t)n1 * lay * HW + n_part;
  const size_t nt = (size_t)(n1 + n2) * lay * HWP + (size_t)waves_max * 2 * lay * HWP;
  void* wsv = nullptr;
  SMN_TRY(smn_workspace(ctx, 4, sizeof(double) * nd + sizeof(T) * nt, &wsv));
  double* dq = static_cast<double*>(wsv);
  double* part = dq + (size_t)n1 * lay * HW;
  T* ra1 = reinterpret_cast<T*>(part + n_part);
  T* ra2 = ra1 + (size_t)n1 * lay * HWP;
  CigxArgs<T> a;
  a.x1 = static_cast<const T*>(x1_d); a.x2 = static_cast<const T*>(x2_d);
  a.ra1 = ra1; a.ra2 = ra2;
  a.alpha = static_cast<const T*>(alpha_d); a.c = cc;
  a.gbar = static_cast<const T*>(gbar_d); a.ldg = ldg;
  a.n2 = n2; a.nsplit = (int)nsplit; a.per = per;
  a.prog = p;
  a.fwd = ra2 + (size_t)n2 * lay * HWP;
  a.part = part;
  {
    ProfScope ps(ctx, PROF_PREP, ctx->stream);
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(cig_q_kernel<T>), lds_q));
    hipLaunchKernelGGL(cig_q_kernel<T>, dim3((unsigned)n1), dim3(256), lds_q, ctx->stream, a.x1, p, n1, (int)HWP, ra1, dq);
    hipLaunchKernelGGL(cig_q_kernel<T>, dim3((unsigned)n2), dim3(256), lds_q, ctx->stream, a.x2, p, (int64_t)0, (int)HWP, ra2,
                       static_cast<double*>(nullptr));
  }
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(cigx_finish_kernel<T>), lds_q));
  for (int64_t row0 = 0; row0 < n1; row0 += rows_b) {
    const int64_t rows = std::min(rows_b, n1 - row0);
    a.row0 = row0; a.items = rows * nsplit;
    const int64_t waves = std::min(resident, round_up(a.items, 4));
    for (int s0 = s_begin; s0 < s_end; s0 += sg) {
      a.s0 = s0; a.ns = std::min(sg, s_end - s0);
      ProfScope ps(ctx, PROF_MISC, ctx->stream);
      hipLaunchKernelGGL(kern, dim3((unsigned)(waves / 4)), dim3(256), lds_p, ctx->stream, a);
      hipLaunchKernelGGL(cigx_finish_kernel<T>, dim3((unsigned)rows, (unsigned)a.ns), dim3(256), lds_q, ctx->stream, a.x1, p,
                         static_cast<const T*>(gdiag_d), dq, part, a.nsplit, (int)HWP, row0, a.items, s0, cc,
                         static_cast<T*>(gmean_d), static_cast<T*>(gvar_d));
      SMN_CHECK_LAUNCH(ctx);
    }
  }
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}

}  // namespace

extern "C" int smn_kernel_cnn_input_grad_cross(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                               double last_w_std, const void* x1_d, int64_t n1, const void* x2_d, int64_t n2,
                                               int64_t H, int64_t W, int64_t C, const void* alpha_d, int64_t c, const void* gbar_d,
                                               int64_t ldg, const void* gdiag_d, void* gmean_d, void* gvar_d) {
  if (!ctx) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_kernel_cnn_input_grad_cross";
  if (!x1_d || !x2_d) return smn_fail(ctx, SMN_EINVAL, "%s: x1_d or x2_d is NULL", who);
  if (!gmean_d && !gvar_d) return smn_fail(ctx, SMN_EINVAL, "%s: gmean_d and gvar_d are both NULL", who);
  if (gmean_d && !alpha_d) return smn_fail(ctx, SMN_EINVAL, "%s: gmean_d needs alpha_d", who);
  if (gvar_d && !gbar_d && !gdiag_d) return smn_fail(ctx, SMN_EINVAL, "%s: gvar_d needs gbar_d or gdiag_d", who);
  if (n1 < 1 || n2 < 1) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes (n1 = %lld, n2 = %lld)", who, (long long)n1, (long long)n2);
  SMN_TRY(conv_check(ctx, who, dtype, act, num_hiddens, n1, H, W, C, kCigMaxHW));
  SMN_CHECK_LD(ctx, who, ldg, n2);
  if (c < 0 || (alpha_d && c < 1)) return smn_fail(ctx, SMN_EINVAL, "%s: c = %lld (1 <= c <= 48 with alpha_d)", who, (long long)c);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: c = %lld: more than 48 mean seeds", who, (long long)c);
  return by_dtype(dtype, [&](auto e) {
    return cigx_run<decltype(e)>(ctx, act, num_hiddens, w_std, b_std, last_w_std, x1_d, n1, x2_d, n2, H, W, C, alpha_d, c, gbar_d, ldg,
                                 gdiag_d, gmean_d, gvar_d);
  });
}

extern "C" int smn_kernel_cnn_input_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                         double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                         const void* gbar_d, int64_t ldg, int64_t n_grad, void* gx_d) {
  if (!ctx || !x_d || !gbar_d || !gx_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_kernel_cnn_input_grad";
  SMN_TRY(conv_check(ctx, who, dtype, act, num_hiddens, n, H, W, C, kCigMaxHW));
  SMN_CHECK_LD(ctx, who, ldg, n);
  if (n_grad < 1 || n_grad > n)
    return smn_fail(ctx, SMN_EINVAL, "%s: n_grad = %lld outside [1, n = %lld]", who, (long long)n_grad, (long long)n);
  return by_dtype(dtype, [&](auto e) {
    return cig_run<decltype(e)>(ctx, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, H, W, C, gbar_d, ldg, n_grad, gx_d);
  });
}
