// grad.hip — analytic hyper-parameter gradients of the log-marginal likelihood.
//
// Replaces what objax.GradValues(model.loss, vars) provides to experiments/regression/train.py:61-67.
// With K~ = K(w, b, lw) + eps I,  alpha = K~^-1 y  and  log p = f(quad = y^T K~^-1 y, logdet K~):
//     d log p / d theta = 1/2 * sum_ij G_ij * dK~_ij/d theta,      G = coef * alpha alpha^T - K~^-1
// (coef = 1 for the Gaussian head, (nu+N)/((nu + quad/s) s) for the Student-t head with shape s K~).
// alpha and -K~^-1 come out of the SAME augmented factorisation the predictive head uses
// (smn_predict with K_td = I, K_tt = 0: mean = alpha, "covariance" = -K~^-1), so the only new device
// code is the contraction: one pass over the lower triangle of K0 = X X^T / d that carries
// (K, dK/dw^2, dK/db^2) through the layer stack in forward mode (in the arithmetic of the storage type,
// sums in fp64) and accumulates  sum G dK/dw_std,  sum G dK/db_std,  sum G dK/dlast_w_std,  tr G.
//
// Forward-mode rules (SURVEY.md Appendix A.1/A.2 differentiated; q_i, q_j = variances entering the map):
//   Dense:  A = w2 K + b2           dA/dw2 = K + w2 dK/dw2          dA/db2 = 1 + w2 dK/db2
//   ReLU:   phi   = sqrt(q_i q_j)/(2 pi) * (sqrt(1-c^2) + (pi - acos c) c),   c = A / sqrt(q_i q_j)
//           phi_A = (pi - acos c)/(2 pi)        phi_qi = sqrt(1-c^2) sqrt(q_i q_j) / (4 pi q_i)
//   Erf:    phi   = (2/pi) asin s,   s = 2A / sqrt(P),  P = (1+2q_i)(1+2q_j)
//           phi_A = 4 / (pi sqrt(P) sqrt(1-s^2))     phi_qi = -(2/pi) s / (sqrt(1-s^2) (1+2q_i))
#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#include "act_tangent.hpp"
#include "gemm_nt.hpp"
#include "grad_rules.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

// the maps, their per-element form and the per-row tables: grad_rules.hpp (shared with lowrank_grad.hip)
using grad_rules::act_d;
using grad_rules::act_r;
using grad_rules::ActD;
using grad_rules::ActR;
using grad_rules::grad_tables_row;
constexpr int kTabFields = grad_rules::kGradTabFields;

template <int NET, int ACT, typename R>
__global__ void grad_tables_kernel(const double* __restrict__ q0, int64_t n, int nsets, double w2, double b2,
                                   R* __restrict__ tab) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  grad_tables_row<NET, ACT, R>(q0, n, nsets, w2, b2, tab, i);
}

template <typename T>
struct GradArgs {
  using R = T;                       // arithmetic of the per-element chain
  const T* k0; int64_t ldk0;
  const T* nkinv; int64_t ldki;      // -K~^-1
  const T* alpha;
  int nc;                            // MULTI forms: alpha is [n, nc] row-major (one row of coefficients per point)
  int64_t n;
  const R* tab;                      // grad_tables_kernel output
  int nsets;
  double w2, b2, lw2, coef;
  double* partial;                   // [gridDim.x][4]
};

constexpr int GT = 64;               // tile edge of the contraction

// One 64 x 64 tile of the lower triangle per workgroup; a thread owns one column and 16 rows (wave w: rows w, w+4, ...)
// and carries their (K, dK/dw2, dK/db2) through the layers together: the column-side table entries are loaded once per
// layer, the row-side ones are wave-uniform (scalar loads).  Products in R, the four sums in double.
// INPLACE (the batched form): -K~^-1 and alpha are read where the joint factorisation left them -- the lower triangle of the
// Schur block (what extract_posterior mirrors into the serial call's copy) and the NEGATED right-hand-side row.
// MULTI (the rank-C form, MultiSPR): g = coef sum_c A_ic A_jc + C (-K~^-1)_ij with A = alpha [n, nc], formed once per entry
// BEHIND the layer loop, so the loop's live state is the single-column form's; the sums and the reduction tree are the same, and
// nc = 1 gives the single-column form's bits.
template <typename T, int NET, int ACT, bool INPLACE, bool MULTI = false>
__device__ __forceinline__ void grad_contract_tile(const GradArgs<T>& a, double* __restrict__ partial) {
  using R = typename GradArgs<T>::R;
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  const int64_t row0 = (int64_t)tr * GT, col0 = (int64_t)tc * GT, n = a.n;
  const int tid = threadIdx.x;
  const int lc = tid % GT;
  const int w = __builtin_amdgcn_readfirstlane(tid / GT);
  constexpr int NR = GT / 4;
  const int64_t j = col0 + lc, jc = j < n ? j : n - 1;
  const R w2 = (R)a.w2, b2 = (R)a.b2;
  R k[NR], dw[NR], db[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t i = row0 + w + 4 * r, ic = i < n ? i : n - 1;
    k[r] = (R)a.k0[ic * a.ldk0 + jc];
    dw[r] = R(0);
    db[r] = R(0);
    if (NET == NET_RESNET) {
      dw[r] = k[r];
      db[r] = R(1);
      k[r] = fma(w2, k[r], b2);
    }
  }
  for (int s = 0; s < a.nsets; ++s) {
    const R* ts = a.tab + (int64_t)s * kTabFields * n;
    const R cdw = ts[n + jc], cdb = ts[2 * n + jc], cra = ts[3 * n + jc], crb = ts[4 * n + jc];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = row0 + w + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
      const R rq = ts[ic], rdw = ts[n + ic], rdb = ts[2 * n + ic], rra = ts[3 * n + ic], rrb = ts[4 * n + ic];
      R kk = k[r], kw = dw[r], kb = db[r];
      if (NET == NET_MLP) {
        kw = fma(w2, kw, kk);
        kb = fma(w2, kb, R(1));
        kk = fma(w2, kk, b2);
      }
      if (i == j) kk = rq;                        // exact diagonal
      const ActR<R> q = act_r<ACT, R>(kk, rra, rrb, cra, crb);
      R o = q.o;
      R ow = fma(q.dA, kw, fma(q.d1, rdw, q.d2 * cdw));
      R ob = fma(q.dA, kb, fma(q.d1, rdb, q.d2 * cdb));
      if (NET == NET_RESNET && s != a.nsets - 1) {
        const R ka = fma(w2, o, b2);
        const R aw = fma(w2, ow, o), ab = fma(w2, ob, R(1));
        o = kk + ka;
        ow = kw + aw;
        ob = kb + ab;
      }
      k[r] = o; dw[r] = ow; db[r] = ob;
    }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum G dK/dw2, sum G dK/db2, sum G K, tr G
  const R coef_r = (R)a.coef;
  R gc[MULTI ? NR : 1];   // MULTI: C (-K~^-1)_ij + coef sum_c A_ic A_jc, column by column (the thread's row of A is read once)
  if (MULTI) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = row0 + w + 4 * r, ic = i < n ? i : n - 1;
      gc[r] = R(a.nc) * (R)a.nkinv[ic * a.ldki + jc];
    }
    const T* rj = a.alpha + jc * a.nc;
    for (int c = 0; c < a.nc; ++c) {
      const R ajc = (R)rj[c];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t i = row0 + w + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
        gc[r] = fma(coef_r * (R)a.alpha[ic * a.nc + c], ajc, gc[r]);
      }
    }
  }
  const R aj = MULTI ? R(0) : (INPLACE ? -(R)a.alpha[jc] : (R)a.alpha[jc]), coef = (R)a.coef, lw2 = (R)a.lw2;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t i = row0 + w + 4 * r, ic = i < n ? i : n - 1;
    const bool valid = i < n && j < n && j <= i;
    const R ai = MULTI ? R(0) : (INPLACE ? -(R)a.alpha[ic] : (R)a.alpha[ic]);
    const int64_t hi = ic > jc ? ic : jc, lo = ic > jc ? jc : ic;
    const R ninv = INPLACE ? (R)a.nkinv[hi * a.ldki + lo] : (R)a.nkinv[ic * a.ldki + jc];
    const R g = MULTI ? gc[r] : fma(coef * ai, aj, ninv);
    const R m = !valid ? R(0) : (i == j ? R(1) : R(2));   // the upper triangle is the mirror image
    const R gm = m * g * lw2;
    acc[0] += (double)(gm * dw[r]);
    acc[1] += (double)(gm * db[r]);
    acc[2] += (double)(gm * k[r]);
    if (valid && i == j) acc[3] += (double)g;
  }
  __shared__ double red[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

template <typename T, int NET, int ACT>
__global__ void __launch_bounds__(256) grad_contract_kernel(GradArgs<T> a) {
  grad_contract_tile<T, NET, ACT, false>(a, a.partial);
}

template <typename T, int NET, int ACT>
__global__ void __launch_bounds__(256) grad_contract_multi_kernel(GradArgs<T> a) {
  grad_contract_tile<T, NET, ACT, false, true>(a, a.partial);
}

// NTK form (SMN_NET_NTK): the covariance is Theta_out = lw2 (K + Theta), so the thread carries SIX values per entry,
// (K, K_w, K_b, Theta, Theta_w, Theta_b) with subscripts d/dw2, d/db2 -- Theta the tangent kernel behind an activation, T the one
// in front of it (the dense ResNet keeps T in the Theta slots between blocks):
//   Dense:       A = w2 K + b2,  A_w = K + w2 K_w,  A_b = 1 + w2 K_b;   T = A + w2 Theta,  T_w = A_w + Theta + w2 Theta_w,
//                T_b = A_b + w2 Theta_b
//   activation:  K <- phi(A), K_t = D A_t + phi_1 q_i,t + phi_2 q_j,t  (as above);   D = phi_A,  D_t = D_A A_t + D_1 q_i,t + D_2 q_j,t;
//                Theta <- T D,  Theta_t = T_t D + T D_t
//   dense ResNet: every state of a block is Dense(act(S)) + S with the same rules (layer_prog.hpp ElemProg::step).
// Six values x 16 rows do not fit the f64 register budget: the thread takes 8 rows at a time and the tile is covered in two
// passes (rows w + 4 r of each 32-row half), the sums running on in the same fixed order.  The sums, the reduction tree and
// the MULTI seed (formed behind the layer loop) are those of grad_contract_tile.
template <typename T, int NET, int ACT, bool MULTI>
__device__ __forceinline__ void grad_contract_tile_ntk(const GradArgs<T>& a, double* __restrict__ partial) {
  using R = typename GradArgs<T>::R;
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  const int64_t row0 = (int64_t)tr * GT, col0 = (int64_t)tc * GT, n = a.n;
  const int tid = threadIdx.x;
  const int lc = tid % GT;
  const int w = __builtin_amdgcn_readfirstlane(tid / GT);
  constexpr int NR = GT / 8, NPASS = 2;
  const int64_t j = col0 + lc, jc = j < n ? j : n - 1;
  const R w2 = (R)a.w2, b2 = (R)a.b2;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum G dTheta_out/dw2, sum G dTheta_out/db2, sum G Theta_out, tr G
  const R coef = (R)a.coef, lw2 = (R)a.lw2;
  const R aj = MULTI ? R(0) : (R)a.alpha[jc];
#pragma unroll 1
  for (int p = 0; p < NPASS; ++p) {
    const int64_t rowp = row0 + w + 4 * NR * p;
    R k[NR], kw[NR], kb[NR], th[NR], tw[NR], tb[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = rowp + 4 * r, ic = i < n ? i : n - 1;
      k[r] = (R)a.k0[ic * a.ldk0 + jc];
      kw[r] = kb[r] = th[r] = tw[r] = tb[r] = R(0);
      if (NET == NET_RESNET) {   // the Dense in front of the first block: A and T = A (Theta = 0)
        kw[r] = k[r];
        kb[r] = R(1);
        k[r] = fma(w2, k[r], b2);
        th[r] = k[r]; tw[r] = kw[r]; tb[r] = kb[r];
      }
    }
    for (int s = 0; s < a.nsets; ++s) {
      const R* ts = a.tab + (int64_t)s * kTabFields * n;
      const R cdw = ts[n + jc], cdb = ts[2 * n + jc], cra = ts[3 * n + jc], crb = ts[4 * n + jc];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t i = rowp + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
        const R rq = ts[ic], rdw = ts[n + ic], rdb = ts[2 * n + ic], rra = ts[3 * n + ic], rrb = ts[4 * n + ic];
        R aa = k[r], aw = kw[r], ab = kb[r], tt = th[r], ttw = tw[r], ttb = tb[r];
        if (NET == NET_MLP) {
          ttw = fma(w2, ttw, tt);          // Theta + w2 Theta_w (+ A_w below)
          ttb = w2 * ttb;
          aw = fma(w2, aw, aa);
          ab = fma(w2, ab, R(1));
          aa = fma(w2, aa, b2);
          if (i == j) aa = rq;             // exact diagonal
          tt = fma(w2, tt, aa);
          ttw += aw;
          ttb += ab;
        } else if (i == j) {
          aa = rq;                         // exact diagonal
        }
        const ActR2<R> q = act_r2<ACT, R>(aa, rra, rrb, cra, crb, i == j);
        R o = q.o;
        R ow = fma(q.dA, aw, fma(q.d1, rdw, q.d2 * cdw));
        R ob = fma(q.dA, ab, fma(q.d1, rdb, q.d2 * cdb));
        const R dw_ = fma(q.hA, aw, fma(q.h1, rdw, q.h2 * cdw));
        const R db_ = fma(q.hA, ab, fma(q.h1, rdb, q.h2 * cdb));
        R to = tt * q.dA;
        R tow = fma(ttw, q.dA, tt * dw_);
        R tob = fma(ttb, q.dA, tt * db_);
        if (NET == NET_RESNET && s != a.nsets - 1) {   // S <- Dense(act(S)) + S, the Theta slots holding T
          const R a2 = fma(w2, o, b2), a2w = fma(w2, ow, o), a2b = fma(w2, ob, R(1));
          const R t2 = fma(w2, to, a2), t2w = fma(w2, tow, to) + a2w, t2b = fma(w2, tob, a2b);
          o = aa + a2; ow = aw + a2w; ob = ab + a2b;
          to = tt + t2; tow = ttw + t2w; tob = ttb + t2b;
        }
        k[r] = o; kw[r] = ow; kb[r] = ob; th[r] = to; tw[r] = tow; tb[r] = tob;
      }
    }
    R gc[MULTI ? NR : 1];
    if (MULTI) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t i = rowp + 4 * r, ic = i < n ? i : n - 1;
        gc[r] = R(a.nc) * (R)a.nkinv[ic * a.ldki + jc];
      }
      const T* rj = a.alpha + jc * a.nc;
      for (int c = 0; c < a.nc; ++c) {
        const R ajc = (R)rj[c];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int64_t i = rowp + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
          gc[r] = fma(coef * (R)a.alpha[ic * a.nc + c], ajc, gc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = rowp + 4 * r, ic = i < n ? i : n - 1;
      const bool valid = i < n && j < n && j <= i;
      const R ai = MULTI ? R(0) : (R)a.alpha[ic];
      const R g = MULTI ? gc[r] : fma(coef * ai, aj, (R)a.nkinv[ic * a.ldki + jc]);
      const R m = !valid ? R(0) : (i == j ? R(1) : R(2));   // the upper triangle is the mirror image
      const R gm = m * g * lw2;
      // the last activation leaves (K, Theta); the last Dense adds them
      acc[0] += (double)(gm * (kw[r] + tw[r]));
      acc[1] += (double)(gm * (kb[r] + tb[r]));
      acc[2] += (double)(gm * (k[r] + th[r]));
      if (valid && i == j) acc[3] += (double)g;
    }
  }
  __shared__ double red[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4) partial[(int64_t)blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

template <typename T, int NET, int ACT, bool MULTI>
__global__ void __launch_bounds__(256) grad_contract_ntk_kernel(GradArgs<T> a) {
  grad_contract_tile_ntk<T, NET, ACT, MULTI>(a, a.partial);
}

// Second stage: fixed-order sum of the per-tile partials (bitwise reproducible).
__device__ __forceinline__ void grad_reduce_block(const double* __restrict__ partial, int64_t ntiles, double* __restrict__ out) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t = tid; t < ntiles; t += 256)
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

__global__ void __launch_bounds__(256) grad_reduce_kernel(const double* __restrict__ partial, int64_t ntiles,
                                                          double* __restrict__ out) {
  grad_reduce_block(partial, ntiles, out);
}

// ---- batched forms (smn_spr_loss_grad_batch): grid.y = the problem.  Each runs the text of the serial kernels above on its
// own hyper-parameters, tables and Schur block, so every problem's sums carry the bits of its serial call.
struct GradProb {
  double w2, b2, lw2, df, scale;   // df <= 0: Gaussian head
  double shift;                    // absolute shift of K's diagonal
};
constexpr int kBatchRes = 8;       // per problem: the four sums, quad, logdet, info, (pad)

template <int NET, int ACT, typename R>
__global__ void grad_tables_batch_kernel(const double* __restrict__ q0, int64_t n, int nsets,
                                         const GradProb* __restrict__ prob, R* __restrict__ tab, int64_t tab_bs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const GradProb p = prob[blockIdx.y];
  grad_tables_row<NET, ACT, R>(q0, n, nsets, p.w2, p.b2, tab + (int64_t)blockIdx.y * tab_bs, i);
}

// coef of the Student-t head from the problem's own quadratic form: the host expression of smn_spr_loss_grad, operation by
// operation (IEEE double add / multiply / divide; nothing here can contract into an FMA)
__device__ __forceinline__ double grad_coef(double df, double scale, double quad, int64_t n) {
#pragma clang fp contract(off)
  if (!(df > 0.0)) return 1.0;
  const double num = df + (double)n;
  const double qs = quad / scale;
  const double den = (df + qs) * scale;
  return num / den;
}

template <typename T>
struct GradBatchArgs {
  const T* k0; int64_t ldk0;
  const T* aug; int64_t lda, bstride, aug0;   // problem b's factored joint matrix at aug + b * bstride; Schur block from (aug0, aug0)
  int64_t n;
  const T* tab; int64_t tab_bs;
  int nsets;
  const GradProb* prob;
  double* partial; int64_t ntiles;            // [batch][ntiles][4]
};

template <typename T, int NET, int ACT>
__global__ void __launch_bounds__(256) grad_contract_batch_kernel(GradBatchArgs<T> b) {
  const int64_t y = blockIdx.y;
  const GradProb p = b.prob[y];
  const T* m = b.aug + y * b.bstride;
  GradArgs<T> a;
  a.k0 = b.k0; a.ldk0 = b.ldk0;
  a.nkinv = m + b.aug0 * b.lda + b.aug0; a.ldki = b.lda;
  a.alpha = m + (b.aug0 + b.n) * b.lda + b.aug0;
  a.nc = 1; a.n = b.n; a.tab = b.tab + y * b.tab_bs; a.nsets = b.nsets;
  a.w2 = p.w2; a.b2 = p.b2; a.lw2 = p.lw2;
  a.coef = grad_coef(p.df, p.scale, -(double)m[(b.aug0 + b.n) * b.lda + b.aug0 + b.n], b.n);
  a.partial = nullptr;
  grad_contract_tile<T, NET, ACT, true>(a, b.partial + y * b.ntiles * 4);
}

// one block per problem: its four sums, and beside them quad, logdet and info, so that ONE copy brings a chunk home
template <typename T>
__global__ void __launch_bounds__(256) grad_reduce_batch_kernel(const double* __restrict__ partial, int64_t ntiles,
                                                                const T* __restrict__ aug, int64_t lda, int64_t bstride,
                                                                int64_t qrow, const double* __restrict__ logdet,
                                                                const int* __restrict__ info, double* __restrict__ res) {
  const int64_t y = blockIdx.x;
  double* r = res + y * kBatchRes;
  grad_reduce_block(partial + y * ntiles * 4, ntiles, r);
  if (threadIdx.x == 4) r[4] = -(double)aug[y * bstride + qrow * lda + qrow];
  if (threadIdx.x == 5) r[5] = logdet[y];
  if (threadIdx.x == 6) r[6] = (double)info[y];
}

// Everything of the joint matrices but K itself, all problems in one launch: rows [n, n_total) cleared, the identity padding,
// the identity block under K, y^T behind it, the problem's absolute shift on K's diagonal (the arithmetic of aug_prep_kernel)
// and the logdet / info reset.  16-byte stores; the shift touches K's rows only, the fill the rows under them.
template <typename T>
__global__ void __launch_bounds__(256) grad_assemble_batch_kernel(T* __restrict__ aug, int64_t lda, int64_t bstride, int64_t n,
                                                                  int64_t n_pad, int64_t n_total, const T* __restrict__ y,
                                                                  const GradProb* __restrict__ prob, double* __restrict__ logdet,
                                                                  int* __restrict__ info) {
  constexpr int VEC = 16 / sizeof(T);
  using vec_t = typename Mfma<T>::vec_t;
  T* a = aug + (int64_t)blockIdx.z * bstride;
  const int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (c0 >= n_total) return;
  if (blockIdx.y == 0) {
    const double sh = prob[blockIdx.z].shift;
    if (sh != 0.0)
      for (int e = 0; e < VEC; ++e) {
        const int64_t c = c0 + e;
        if (c < n) a[c * lda + c] = (T)((double)a[c * lda + c] + sh);
      }
  }
  for (int64_t r = n + blockIdx.y; r < n_total; r += gridDim.y) {
    vec_t v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int64_t c = c0 + e;
      T x = T(0);
      if (r < n_pad) x = c == r ? T(1) : T(0);                      // identity padding
      else if (r < n_pad + n) x = c == r - n_pad ? T(1) : T(0);     // identity block
      else if (r == n_pad + n) x = c < n ? y[c] : T(0);             // y^T
      v[e] = x;
    }
    *reinterpret_cast<vec_t*>(a + r * lda + c0) = v;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    logdet[blockIdx.z] = 0.0;
    info[blockIdx.z] = INT_MAX;
  }
}

template <typename T>
__global__ void cast_q_kernel(const T* __restrict__ s, double* __restrict__ d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = (double)s[i];
}

// f(NET, ACT) with the (net, act) pair of a validated call as compile-time constants: the one place the host code of this file
// picks a kernel instantiation
template <typename F>
int with_net_act(int net, int act, F&& f) {
  using std::integral_constant;
  if (net == SMN_NET_MLP && act == SMN_ACT_RELU) return f(integral_constant<int, NET_MLP>{}, integral_constant<int, ACT_RELU>{});
  if (net == SMN_NET_MLP) return f(integral_constant<int, NET_MLP>{}, integral_constant<int, ACT_ERF>{});
  if (act == SMN_ACT_RELU) return f(integral_constant<int, NET_RESNET>{}, integral_constant<int, ACT_RELU>{});
  return f(integral_constant<int, NET_RESNET>{}, integral_constant<int, ACT_ERF>{});
}

template <typename T, int NET, int ACT>
int grad_terms_na(smn_ctx* ctx, const GradArgs<T>& a, const double* q64, int64_t ntiles, double* out_d, bool multi, bool ntk) {
  hipLaunchKernelGGL((grad_tables_kernel<NET, ACT, T>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, ctx->stream,
                     q64, a.n, a.nsets, a.w2, a.b2, const_cast<T*>(a.tab));
  SMN_CHECK_LAUNCH(ctx);
  {
    ProfScope ps(ctx, PROF_MISC, ctx->stream);
    if (ntk && multi) hipLaunchKernelGGL((grad_contract_ntk_kernel<T, NET, ACT, true>), dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
    else if (ntk) hipLaunchKernelGGL((grad_contract_ntk_kernel<T, NET, ACT, false>), dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
    else if (multi) hipLaunchKernelGGL((grad_contract_multi_kernel<T, NET, ACT>), dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((grad_contract_kernel<T, NET, ACT>), dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
  }
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(grad_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, a.partial, ntiles, out_d);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

template <typename T>
int grad_terms_t(smn_ctx* ctx, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                 const void* k0, int64_t n, int64_t ldk0, const void* q, const void* nkinv, int64_t ldki,
                 const void* alpha, double coef, double out_h[4], int nc = 0,   // nc > 0: the rank-C form, alpha [n, nc]
                 bool ntk = false) {                                              // the tangent of Theta instead of K
  const bool multi = nc > 0;
  const int nsets = net == SMN_NET_MLP ? num_hiddens : num_hiddens + 1;
  if (nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "num_hiddens too large (max %d activation layers)", kMaxSets);
  const int64_t t = (n + GT - 1) / GT, ntiles = t * (t + 1) / 2;
  void* wsv = nullptr;
  const size_t ntab = (size_t)n * kTabFields * (size_t)(nsets > 0 ? nsets : 1);   // T-typed; sized as doubles
  const size_t nd = (size_t)n + ntab + (size_t)ntiles * 4 + 4;
  SMN_TRY(smn_workspace(ctx, 4, sizeof(double) * nd, &wsv));
  double* q64 = static_cast<double*>(wsv);
  double* tabd = q64 + n;
  double* partial = tabd + ntab;
  double* out_d = partial + (size_t)ntiles * 4;
  hipLaunchKernelGGL(cast_q_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     static_cast<const T*>(q), q64, n);
  SMN_CHECK_LAUNCH(ctx);
  GradArgs<T> a;
  a.k0 = static_cast<const T*>(k0); a.ldk0 = ldk0;
  a.nkinv = static_cast<const T*>(nkinv); a.ldki = ldki;
  a.alpha = static_cast<const T*>(alpha);
  a.nc = multi ? nc : 1;
  a.n = n; a.tab = reinterpret_cast<const T*>(tabd); a.nsets = nsets;
  a.w2 = w_std * w_std; a.b2 = b_std * b_std; a.lw2 = last_w_std * last_w_std; a.coef = coef;
  a.partial = partial;
  SMN_TRY(with_net_act(net, act, [&](auto NET, auto ACT) {
    return grad_terms_na<T, decltype(NET)::value, decltype(ACT)::value>(ctx, a, q64, ntiles, out_d, multi, ntk);
  }));
  double s[4];
  SMN_HIP(ctx, hipMemcpyAsync(s, out_d, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out_h[0] = s[0] * 2.0 * w_std;                  // d/dw_std  = 2 w  d/dw^2
  out_h[1] = s[1] * 2.0 * b_std;
  out_h[2] = s[2] * 2.0 / last_w_std;             // K = lw^2 K_L  =>  dK/dlw = 2 K / lw  (NTK form: lw^2 (K_L + Theta_L))
  out_h[3] = s[3];                                // dK~/deps = I
  return SMN_OK;
}

// The batched launches of one chunk behind its factorisation: tables, contraction, reduction (+ quad / logdet / info).
template <typename T, int NET, int ACT>
int grad_batch_launch(smn_ctx* ctx, const GradBatchArgs<T>& b, int nb, const double* q64, const double* logdet_d,
                      const int* info_d, double* res_d) {
  hipLaunchKernelGGL((grad_tables_batch_kernel<NET, ACT, T>), dim3((unsigned)((b.n + 255) / 256), (unsigned)nb), dim3(256), 0,
                     ctx->stream, q64, b.n, b.nsets, b.prob, const_cast<T*>(b.tab), b.tab_bs);
  SMN_CHECK_LAUNCH(ctx);
  {
    ProfScope ps(ctx, PROF_MISC, ctx->stream);
    hipLaunchKernelGGL((grad_contract_batch_kernel<T, NET, ACT>), dim3((unsigned)b.ntiles, (unsigned)nb), dim3(256), 0,
                       ctx->stream, b);
  }
  SMN_CHECK_LAUNCH(ctx);
  const int64_t qrow = b.aug0 + b.n;
  hipLaunchKernelGGL(grad_reduce_batch_kernel<T>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, b.partial, b.ntiles, b.aug,
                     b.lda, b.bstride, qrow, logdet_d, info_d, res_d);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

// The joint route of smn_spr_loss_grad for nprob problems at once (heads.hip posterior_from_x, batched the way
// spr_batch batches the loss): K0 and its diagonal once; per chunk the G joint matrices [[K~, .], [I, 0], [y^T, 0, 0]] side by
// side in workspace slot 2, ONE factorisation with grid.y = G, and the contraction reading -K~^-1 and alpha where it left them.
template <typename T>
int grad_batch_t(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, int nprob, const double* w_std, const double* b_std,
                 const double* last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                 const double* eps_abs, const double* df, const double* scale, double* quad_h, double* logdet_h, int* info_h,
                 double* terms_h) {
  const int nsets = net == SMN_NET_MLP ? num_hiddens : num_hiddens + 1;
  if (nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "num_hiddens too large (max %d activation layers)", kMaxSets);
  const size_t es = sizeof(T);
  const int64_t ld0 = round_up(n, 16 / (int64_t)es);
  void* k0 = nullptr;
  SMN_TRY(smn_workspace(ctx, 5, es * ((size_t)n * ld0 + (size_t)n), &k0));
  void* q = static_cast<char*>(k0) + es * (size_t)n * ld0;
  SMN_TRY(gram_lower(ctx, dtype, x_d, n, ldx, d, k0, ld0, q));
  const int64_t n_pad = round_up(n, kTile), n_total = n_pad + round_up(n + 1, kTile), lda = n_total, bstride = n_total * lda;
  const size_t per = es * (size_t)bstride;
  int chunk = (int)std::min<size_t>((size_t)nprob, std::max<size_t>(1, ctx->batch_bytes / per));
  if (chunk > 65535) chunk = 65535;   // grid.y / grid.z
  void *av = nullptr, *gv = nullptr, *sv = nullptr;
  SMN_TRY(smn_workspace(ctx, 2, per * (size_t)chunk, &av));
  const int64_t t64 = (n + GT - 1) / GT, ntiles = t64 * (t64 + 1) / 2;
  const size_t ntab = (size_t)n * kTabFields * (size_t)(nsets > 0 ? nsets : 1);   // T-typed; sized as doubles, per problem
  SMN_TRY(smn_workspace(ctx, 4, sizeof(double) * ((size_t)n + (size_t)chunk * (ntab + (size_t)ntiles * 4 + kBatchRes)), &gv));
  double* q64 = static_cast<double*>(gv);
  double* tabd = q64 + n;
  double* partial = tabd + (size_t)chunk * ntab;
  double* res_d = partial + (size_t)chunk * (size_t)ntiles * 4;
  // per-problem scalars: GradProb and logdet (doubles), info (ints)
  SMN_TRY(smn_workspace(ctx, 8, (sizeof(GradProb) + sizeof(double) + sizeof(int)) * (size_t)chunk, &sv));
  GradProb* prob_d = static_cast<GradProb*>(sv);
  double* ld_d = reinterpret_cast<double*>(prob_d + chunk);
  int* info_d = reinterpret_cast<int*>(ld_d + chunk);
  hipLaunchKernelGGL(cast_q_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<const T*>(q), q64, n);
  SMN_CHECK_LAUNCH(ctx);
  // host sources of the two parameter uploads of a chunk: they live until the chunk's synchronisation (and a failed call
  // drains the stream before they go, below), so neither upload needs a synchronisation of its own
  std::vector<GradProb> prob_h((size_t)chunk);
  std::vector<char> progs_h;
  const BuildSpec spec{dtype, net, act, num_hiddens, w_std[0], b_std[0], last_w_std[0]};
  std::vector<double> res_h((size_t)chunk * kBatchRes);
  struct Drain {   // an error return: nothing in flight may still read the vectors above
    smn_ctx* c; bool armed = true;
    ~Drain() { if (armed) (void)hipStreamSynchronize(c->stream); }
  } drain{ctx};
  for (int p0 = 0; p0 < nprob; p0 += chunk) {
    const int nb = std::min(chunk, nprob - p0);
    SMN_TRY(recursion_lower_batch(ctx, spec, nb, w_std + p0, b_std + p0, last_w_std + p0, k0, n, ld0, q, av, lda, bstride, progs_h));
    for (int b = 0; b < nb; ++b) {
      const int g = p0 + b;
      prob_h[(size_t)b] = GradProb{w_std[g] * w_std[g], b_std[g] * b_std[g], last_w_std[g] * last_w_std[g], df ? df[g] : 0.0,
                                   scale ? scale[g] : 1.0, eps_abs[g]};
    }
    SMN_HIP(ctx, hipMemcpyAsync(prob_d, prob_h.data(), sizeof(GradProb) * (size_t)nb, hipMemcpyHostToDevice, ctx->stream));
    {
      constexpr int VEC = 16 / (int)sizeof(T);
      dim3 ga((unsigned)((n_total / VEC + 255) / 256), (unsigned)std::min<int64_t>(n_total - n, 1024), (unsigned)nb);
      hipLaunchKernelGGL(grad_assemble_batch_kernel<T>, ga, dim3(256), 0, ctx->stream, static_cast<T*>(av), lda, bstride, n, n_pad,
                         n_total, static_cast<const T*>(y_d), prob_d, ld_d, info_d);
    }
    SMN_CHECK_LAUNCH(ctx);
    FactorCall f{dtype, av, n_total, n_pad, lda, n, 0.0, 0.0, false};
    f.id0 = n_pad;
    f.id1 = n_pad + n / kTile * kTile;
    f.prepped = true;
    f.batch = nb; f.batch_stride = bstride; f.batch_logdet = ld_d; f.batch_info = info_d;
    SMN_TRY(cholesky_padded(ctx, f));
    GradBatchArgs<T> ba;
    ba.k0 = static_cast<const T*>(k0); ba.ldk0 = ld0;
    ba.aug = static_cast<const T*>(av); ba.lda = lda; ba.bstride = bstride; ba.aug0 = n_pad;
    ba.n = n; ba.tab = reinterpret_cast<const T*>(tabd); ba.tab_bs = (int64_t)ntab; ba.nsets = nsets;
    ba.prob = prob_d; ba.partial = partial; ba.ntiles = ntiles;
    // a chunk of up to eight problems (a single start above all) publishes straight into the pinned mailbox, as the serial
    // call's read-out does: one synchronisation, no copy
    const bool mail = (size_t)nb * kBatchRes <= (size_t)smn_ctx::kMailGram;
    double* out_d = mail ? ctx->d_mail : res_d;
    SMN_TRY(with_net_act(net, act, [&](auto NET, auto ACT) {
      return grad_batch_launch<T, decltype(NET)::value, decltype(ACT)::value>(ctx, ba, nb, q64, ld_d, info_d, out_d);
    }));
    if (!mail)
      SMN_HIP(ctx, hipMemcpyAsync(res_h.data(), res_d, sizeof(double) * (size_t)nb * kBatchRes, hipMemcpyDeviceToHost, ctx->stream));
    SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double* res = mail ? ctx->h_mail : res_h.data();
    for (int b = 0; b < nb; ++b) {
      const int g = p0 + b;
      const double* r = res + (size_t)b * kBatchRes;
      int info = (int)r[6];
      if (info == INT_MAX) info = 0;
      if (info_h) info_h[g] = info;
      if (quad_h) quad_h[g] = info ? std::nan("") : r[4];
      if (logdet_h) logdet_h[g] = info ? std::nan("") : r[5];
      double* t = terms_h + (size_t)g * 4;
      if (info != 0) {
        for (int i = 0; i < 4; ++i) t[i] = std::nan("");
        continue;
      }
      t[0] = r[0] * 2.0 * w_std[g];
      t[1] = r[1] * 2.0 * b_std[g];
      t[2] = r[2] * 2.0 / last_w_std[g];
      t[3] = r[3];
    }
  }
  drain.armed = false;   // the last chunk's synchronisation has passed
  return SMN_OK;
}

// smn_lml_grad_terms (multi = false: alpha [n], the single-output kernel form) / smn_lml_grad_terms_multi (the rank-C
// contraction: alpha_d [n, c] row-major, G = coef A A^T - c K~^-1)
int lml_grad_terms(smn_ctx* ctx, const char* who, bool multi, int dtype, int net, int act, int num_hiddens, double w_std,
                   double b_std, double last_w_std, const void* k0_d, int64_t n, int64_t ldk0, const void* q_d,
                   const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, int64_t c, double coef, double terms_h[4]) {
  if (!ctx || !k0_d || !q_d || !neg_kinv_d || !alpha_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (n <= 0 || c < 1) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes", who);
  SMN_CHECK_LD(ctx, who, ldk0, n);
  SMN_CHECK_LD(ctx, who, ldkinv, n);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  bool ntk = false;
  SMN_TRY(split_net(ctx, &net, &ntk));
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "Unsupported act %d", act);
  if (num_hiddens < 0 || !(last_w_std != 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: bad hyper-parameters", who);
  const int nc = multi ? (int)c : 0;
  return by_dtype(dtype, [&](auto e) {
    return grad_terms_t<decltype(e)>(ctx, net, act, num_hiddens, w_std, b_std, last_w_std, k0_d, n, ldk0, q_d, neg_kinv_d,
                                ldkinv, alpha_d, coef, terms_h, nc, ntk);
  });
}

// smn_spr_loss_grad / smn_spr_loss_grad_multi.  Fused: K0 = X X^T / d and its diagonal, K by the stand-alone recursion straight
// into the factorisation workspace laid out as the rectangle [[K~], [I], [Y^T]] for the c target columns that share K~, a
// no-Schur factorisation (L, L^-T, L^-1 Y), -K~^-1 = -L^-T L^-1 as one full-rate launch, alpha = L^-T (L^-1 Y) (heads.hip
// posterior_from_x), then the contraction under the coef of the joint Student-t head (lml_coef).
int spr_loss_grad(smn_ctx* ctx, const char* who, bool multi, int dtype, int net, int act, int num_hiddens, double w_std,
                  double b_std, double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                  double eps_abs, double df, double scale, double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h,
                  double terms_h[4]) {
  if (!ctx || !x_d || !y_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (n <= 0 || d <= 0 || c < 1) return smn_fail(ctx, SMN_EINVAL, "%s: empty", who);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  if (df > 0.0 && !(scale > 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: scale must be > 0", who);
  SMN_CHECK_LD(ctx, who, ldx, d);
  const BuildSpec spec{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};
  Posterior p;
  SMN_TRY(posterior_from_x(ctx, spec, x_d, n, ldx, d, y_d, c, eps_abs, &p));
  const double tot = publish_head(p, c, multi, n, df, scale, nullptr, quad_h, quad_cols_h, logdet_h, info_h, terms_h);
  if (p.info != 0) return SMN_OK;
  return lml_grad_terms(ctx, multi ? "smn_lml_grad_terms_multi" : "smn_lml_grad_terms", multi, dtype, net, act, num_hiddens, w_std,
                        b_std, last_w_std, p.k0, n, p.ld0, p.q, p.ninv, p.ldinv, p.alpha, c, lml_coef(df, scale, tot, n, c),
                        terms_h);
}

}  // namespace

extern "C" int smn_lml_grad_terms(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std,
                                  double b_std, double last_w_std, const void* k0_d, int64_t n, int64_t ldk0,
                                  const void* q_d, const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d,
                                  double coef, double terms_h[4]) {
  return lml_grad_terms(ctx, "smn_lml_grad_terms", false, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, k0_d, n, ldk0,
                        q_d, neg_kinv_d, ldkinv, alpha_d, 1, coef, terms_h);
}

extern "C" int smn_lml_grad_terms_multi(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std,
                                        double b_std, double last_w_std, const void* k0_d, int64_t n, int64_t ldk0,
                                        const void* q_d, const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d,
                                        int64_t c, double coef, double terms_h[4]) {
  return lml_grad_terms(ctx, "smn_lml_grad_terms_multi", true, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, k0_d, n,
                        ldk0, q_d, neg_kinv_d, ldkinv, alpha_d, c, coef, terms_h);
}

extern "C" int smn_spr_loss_grad_multi(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std,
                                       double b_std, double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d,
                                       const void* y_d, int64_t c, double eps_abs, double df, double scale, double* quad_h,
                                       double* quad_cols_h, double* logdet_h, int* info_h, double terms_h[4]) {
  return spr_loss_grad(ctx, "smn_spr_loss_grad_multi", true, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx,
                       d, y_d, c, eps_abs, df, scale, quad_h, quad_cols_h, logdet_h, info_h, terms_h);
}

extern "C" int smn_spr_loss_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std,
                                 double b_std, double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d,
                                 const void* y_d, double eps_abs, double df, double scale, double* quad_h,
                                 double* logdet_h, int* info_h, double terms_h[4]) {
  return spr_loss_grad(ctx, "smn_spr_loss_grad", false, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, d,
                       y_d, 1, eps_abs, df, scale, quad_h, nullptr, logdet_h, info_h, terms_h);
}

// nprob x smn_spr_loss_grad on one data set (their own w_std, b_std, last_w_std, shift and head) as ONE sequence of launches
// with grid.y = the problem; below the rectangle route's size only -- from there on one problem fills the chip, and the
// problems run one after another through the serial call.
extern "C" int smn_spr_loss_grad_batch(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, int nprob,
                                       const double* w_std, const double* b_std, const double* last_w_std, const void* x_d,
                                       int64_t n, int64_t ldx, int64_t d, const void* y_d, const double* eps_abs,
                                       const double* df, const double* scale, double* quad_h, double* logdet_h, int* info_h,
                                       double* terms_h) {
  if (!ctx || !x_d || !y_d || !terms_h) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype");
  if (nprob <= 0 || !w_std || !b_std || !last_w_std || !eps_abs)
    return smn_fail(ctx, SMN_EINVAL, "smn_spr_loss_grad_batch: empty batch or null parameter array");
  if (n <= 0 || d <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_spr_loss_grad_batch: empty");
  SMN_CHECK_LD(ctx, "smn_spr_loss_grad_batch", ldx, d);
  SMN_TRY(no_ntk_net(ctx, "smn_spr_loss_grad_batch", net));
  if (net != SMN_NET_MLP && net != SMN_NET_DENSE_RESNET) return smn_fail(ctx, SMN_EINVAL, "unknown net %d", net);
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "Unsupported act %d", act);
  if (num_hiddens < 0) return smn_fail(ctx, SMN_EINVAL, "num_hiddens < 0");
  for (int b = 0; b < nprob; ++b) {
    if (df && df[b] > 0.0 && !(scale && scale[b] > 0.0)) return smn_fail(ctx, SMN_EINVAL, "smn_spr_loss_grad_batch: scale must be > 0");
    if (!(last_w_std[b] != 0.0)) return smn_fail(ctx, SMN_EINVAL, "smn_spr_loss_grad_batch: bad hyper-parameters");
  }
  if (grad_uses_rectangle(n)) {
    for (int b = 0; b < nprob; ++b)
      SMN_TRY(smn_spr_loss_grad(ctx, dtype, net, act, num_hiddens, w_std[b], b_std[b], last_w_std[b], x_d, n, ldx, d, y_d, eps_abs[b],
                                df ? df[b] : 0.0, scale ? scale[b] : 1.0, quad_h ? quad_h + b : nullptr,
                                logdet_h ? logdet_h + b : nullptr, info_h ? info_h + b : nullptr, terms_h + (size_t)b * 4));
    return SMN_OK;
  }
  return by_dtype(dtype, [&](auto e) {
    return grad_batch_t<decltype(e)>(ctx, dtype, net, act, num_hiddens, nprob, w_std, b_std, last_w_std, x_d, n, ldx, d, y_d, eps_abs, df,
                                scale, quad_h, logdet_h, info_h, terms_h);
  });
}
