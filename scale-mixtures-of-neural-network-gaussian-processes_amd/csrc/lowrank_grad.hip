// lowrank_grad.hip — analytic hyper-parameter gradient of the log-marginal likelihood of the low-rank model of lowrank.hip at
// FIXED pivots P (inducing inputs Z = X[P]):  K^ = Q + diag(mu o (k - q)) + lambda I,  Q = K_nP K_PP^-1 K_Pn = L L^T.
//
// With W = diag(1 / d), A = I + L^T W L = C C^T, beta = A^-1 L^T W Y, alpha = W (Y - L beta) = K^^-1 Y, R = L[P, :]:
//     h_i = |C^-1 L_i^T|^2,  kappa_i = (K^^-1)_ii = w_i - w_i^2 h_i,  g_i = coef |alpha_i|^2 - c kappa_i,  mu_i = fitc [resid_i > 0]
//     U = [coef alpha beta^T - c W L A^-1 - diag(mu o g) L] R^-1                                   [n, m]
//     T = R^-T [coef beta beta^T - c (I - A^-1) - L^T diag(mu o g) L] R^-1                         [m, m]
//     terms_theta = 2 sum_ia U_ia dK(x_i, z_a) - sum_ab T_ab dK(z_a, z_b) + sum_i mu_i g_i dK(x_i, x_i),   terms_eps = sum_i g_i
// in the convention of smn_lml_grad_terms (d logpdf / d theta = terms / 2).  O(n m^2 + n m d) work, O(n m) memory.
//
// Stages
//   m x m side (fp64 for both storage types, as everything m x m in lowrank.hip): C^-1, A^-1 = C^-T C^-1, R^-1, A^-1 R^-1,
//     R^-T beta and the two solves of T, all through smn_trsm on the device; nothing of it comes to the host.
//   row pass (lrg_row_kernel): a workgroup takes 16 rows of L, read in place (16-byte loads when the base and ldl allow, element
//     loads into the same registers otherwise) and staged in LDS as fp64 in tiles of 64 columns; thread a carries column a of
//     L C^-T for the 16 rows (the triangle of C^-T is skipped by whole column blocks), squares it into h, then the threads
//     k < c carry L beta.  Every sum is fp64 in a fixed order (t ascending; the column blocks ascending; a butterfly; the four
//     waves): the bits depend neither on ldl nor on the alignment nor on a grid.
//   L^T diag(mu o g) L: smn_lowrank_gram with the weights mu o g (any sign: the weight only multiplies).
//   U (lrg_u_kernel): the same product against A^-1 R^-1 and R^-1 side by side, fp64 accumulation, U stored in the storage type.
//   K0 = X Z^T / d [n, m]: ONE rectangular smn_gram into a workspace of the size of L, not fused into the contraction.  The
//     tile engine already has the NT product with its staging, padding and alignment paths, and it leaves the per-row variances
//     q_i the tables need; the product is 2 n m d flop on the MFMAs against an [n, m] round trip through HBM that is 1 / d of
//     its operand traffic.  A fused form would keep K0 in registers and save that round trip ("Not done").
//   contraction (lrg_contract_kernel): grad.hip's grad_contract_tile on a rectangle -- one 64 x 64 tile per workgroup, a thread
//     owns a column and 16 rows and carries (K, dK/dw2, dK/db2) through the layer stack by the rules of grad_rules.hpp in the
//     storage arithmetic; row- and column-side tables are the per-row tables of X, the column side indexed through the
//     pivots; the exact-diagonal rule applies where i == P[a].  The same kernel takes the m x m square of Z against itself with
//     the rows mapped through P as well (weights -T).  The four sums are fp64; per-workgroup partials go to one fixed-tree
//     reduction.  No floating-point atomics anywhere.
//   diagonal term: sum_i mu_i g_i dK_ii from the fp64 end of the tables' own chain.
#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#include "grad_rules.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

using grad_rules::act_r;
using grad_rules::ActR;
using grad_rules::DiagEnd;
using grad_rules::grad_tables_row;
constexpr int kTabFields = grad_rules::kGradTabFields;

constexpr int kRows = 16;    // rows of L per workgroup of the row kernels
constexpr int kTT = 64;      // columns of L staged per LDS tile
constexpr int kMaxC = 48;
constexpr int GT = 64;       // tile edge of the contraction

__device__ __forceinline__ double lrg_weight(const double* __restrict__ resid, int64_t i, double lambda, int fitc) {
  return 1.0 / ((fitc && resid ? fmax(resid[i], 0.0) : 0.0) + lambda);   // (the expression of lowrank_weights_kernel)
}

// sh[t][r] <- (double) L[row0 + r][t0 + t], t < 64, r < 16; zero behind m; a row past the end repeats the last one
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ L, int64_t n, int m, int64_t ldl, bool vec_ok, int64_t row0, int t0,
                                           double (*sh)[kRows]) {
  constexpr int V = Vec16<T>::N;
  const int r = threadIdx.x >> 4, tq = (threadIdx.x & 15) * 4;
  const int64_t i = row0 + r < n ? row0 + r : n - 1;
  const T* src = L + i * ldl;
  T v[4];
#pragma unroll
  for (int u = 0; u < 4; u += V) {
    const int t = t0 + tq + u;
    if (vec_ok && t + V <= m) {
      const typename Vec16<T>::type x = *reinterpret_cast<const typename Vec16<T>::type*>(src + t);
#pragma unroll
      for (int k = 0; k < V; ++k) v[u + k] = x[k];
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) v[u + k] = t + k < m ? src[t + k] : T(0);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[tq + k][r] = (double)v[k];
}

// a0[r] += sum_{t < t_hi} L[row0 + r][t] M0[t][col] (and a1 with M1 when NM == 2), t ascending.  The whole workgroup stages the
// tiles: every thread calls this with the same row0 and t_hi <= m; col_ok == false: the thread only helps staging.
template <typename T, int NM>
__device__ __forceinline__ void row_product(const T* __restrict__ L, int64_t n, int m, int64_t ldl, bool vec_ok, int64_t row0,
                                            const double* __restrict__ M0, const double* __restrict__ M1, int64_t ldm, int col,
                                            bool col_ok, int t_hi, double (*sh)[kRows], double (&a0)[kRows], double (&a1)[kRows]) {
  for (int t0 = 0; t0 < t_hi; t0 += kTT) {
    __syncthreads();   // the readers of the tile before this one are done
    stage_rows<T>(L, n, m, ldl, vec_ok, row0, t0, sh);
    __syncthreads();
    if (col_ok) {
      const int te = t_hi - t0 < kTT ? t_hi - t0 : kTT;
      for (int t = 0; t < te; ++t) {
        const double m0 = M0[(int64_t)(t0 + t) * ldm + col];
        const double m1 = NM == 2 ? M1[(int64_t)(t0 + t) * ldm + col] : 0.0;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const double l = sh[t][r];
          a0[r] = fma(l, m0, a0[r]);
          if (NM == 2) a1[r] = fma(l, m1, a1[r]);
        }
      }
    }
  }
}

template <typename T>
struct RowArgs {
  const T* L; int64_t n; int m; int64_t ldl; int vec_ok;
  const double* resid; double lambda; int fitc;
  const T* y; int64_t ldy; int c; double coef;
  const double* cinvt;   // C^-T [m, m] (upper triangular)
  const double* beta;    // [m, c]
  const double* m1;      // A^-1 R^-1 [m, m]
  const double* m2;      // R^-1 [m, m]
  const double* bt;      // R^-T beta [m, c]
  double* alpha;         // [n, c]
  double* g;             // [n]
  double* mg;            // [n]: mu o g
  T* U; int64_t ldu;
};

template <typename T>
__global__ void __launch_bounds__(256) lrg_row_kernel(RowArgs<T> a) {
  __shared__ double sh[kTT][kRows];
  __shared__ double hs[4][kRows];
  __shared__ double a2[kRows][kMaxC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  double hacc[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) hacc[r] = 0.0;
  for (int c0 = 0; c0 < a.m; c0 += 256) {
    const int col = c0 + tid;
    const bool ok = col < a.m;
    double q[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) q[r] = 0.0;
    const int t_hi = c0 + 256 < a.m ? c0 + 256 : a.m;   // (C^-T)[t][col] = 0 for t > col
    row_product<T, 1>(a.L, a.n, a.m, a.ldl, a.vec_ok != 0, row0, a.cinvt, nullptr, a.m, col, ok, t_hi, sh, q, q);
    if (ok) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) hacc[r] = fma(q[r], q[r], hacc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    double v = hacc[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) hs[wave][r] = v;
  }
  double lb[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) lb[r] = 0.0;
  const bool kok = tid < a.c;
  row_product<T, 1>(a.L, a.n, a.m, a.ldl, a.vec_ok != 0, row0, a.beta, nullptr, a.c, tid, kok, a.m, sh, lb, lb);
  if (kok) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int64_t i = row0 + r;
      double al = 0.0;
      if (i < a.n) {
        al = lrg_weight(a.resid, i, a.lambda, a.fitc) * ((double)a.y[i * a.ldy + tid] - lb[r]);
        a.alpha[i * a.c + tid] = al;
      }
      a2[r][tid] = al * al;
    }
  }
  __syncthreads();
  if (tid < kRows && row0 + tid < a.n) {
    const int64_t i = row0 + tid;
    const double h = (hs[0][tid] + hs[1][tid]) + (hs[2][tid] + hs[3][tid]);
    double s = 0.0;
    for (int k = 0; k < a.c; ++k) s += a2[tid][k];
    const double w = lrg_weight(a.resid, i, a.lambda, a.fitc);
    const double kappa = w - w * w * h;
    const double g = a.coef * s - (double)a.c * kappa;
    a.g[i] = g;
    a.mg[i] = (a.fitc && a.resid && a.resid[i] > 0.0) ? g : 0.0;   // the clamp's derivative is 0 where it is active
  }
}

// U[i][col] = -c w_i (L_i A^-1 R^-1)[col] - mu_i g_i (L_i R^-1)[col] + coef sum_k alpha_ik (R^-T beta)[col][k]
template <typename T>
__global__ void __launch_bounds__(256) lrg_u_kernel(RowArgs<T> a) {
  __shared__ double sh[kTT][kRows];
  __shared__ double as[kRows][kMaxC];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int col = blockIdx.y * 256 + tid;
  const bool ok = col < a.m;
  double u1[kRows], u2[kRows], u3[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    u1[r] = 0.0; u2[r] = 0.0; u3[r] = 0.0;
  }
  for (int e = tid; e < kRows * a.c; e += 256) {
    const int r = e / a.c, k = e - r * a.c;
    as[r][k] = row0 + r < a.n ? a.alpha[(row0 + r) * a.c + k] : 0.0;
  }
  row_product<T, 2>(a.L, a.n, a.m, a.ldl, a.vec_ok != 0, row0, a.m1, a.m2, a.m, col, ok, a.m, sh, u1, u2);
  if (!ok) return;   // (behind the last barrier)
  for (int k = 0; k < a.c; ++k) {
    const double b = a.bt[(int64_t)col * a.c + k];
#pragma unroll
    for (int r = 0; r < kRows; ++r) u3[r] = fma(as[r][k], b, u3[r]);
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int64_t i = row0 + r;
    if (i < a.n) {
      const double w = lrg_weight(a.resid, i, a.lambda, a.fitc);
      a.U[i * a.ldu + col] = (T)(fma(-(double)a.c * w, u1[r], a.coef * u3[r]) - a.mg[i] * u2[r]);
    }
  }
}

// ---- small kernels of the m x m side
__global__ void lrg_identity_kernel(double* __restrict__ a, int m) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * m) return;
  a[e] = (e / m == e % m) ? 1.0 : 0.0;
}

// B[a][b] = coef sum_k beta_ak beta_bk - c (delta_ab - Ainv_ab) - G2_ab, in place of G2
__global__ void lrg_bracket_kernel(double* __restrict__ g2, const double* __restrict__ ainv, const double* __restrict__ beta, int m,
                                   int c, double coef) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * m) return;
  const int ia = (int)(e / m), ib = (int)(e % m);
  double s = 0.0;
  for (int k = 0; k < c; ++k) s = fma(beta[(int64_t)ia * c + k], beta[(int64_t)ib * c + k], s);
  g2[e] = coef * s - (double)c * ((ia == ib ? 1.0 : 0.0) - ainv[e]) - g2[e];
}

template <typename T>
__global__ void lrg_cast_matrix_kernel(const double* __restrict__ src, int m, T* __restrict__ dst, int64_t ldd) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * m) return;
  dst[(e / m) * ldd + e % m] = (T)src[e];
}

template <typename T>
__global__ void lrg_gather_kernel(const T* __restrict__ x, int64_t ldx, int64_t d, const int64_t* __restrict__ piv, int m,
                                  T* __restrict__ z, int64_t ldz) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * ldz) return;
  const int64_t a = e / ldz, k = e % ldz;
  z[e] = k < d ? x[piv[a] * ldx + k] : T(0);
}

template <typename T>
__global__ void lrg_cast_q_kernel(const T* __restrict__ s, double* __restrict__ d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = (double)s[i];
}

template <int NET, int ACT, typename R>
__global__ void lrg_tables_kernel(const double* __restrict__ q0, int64_t n, int nsets, double w2, double b2, R* __restrict__ tab,
                                  double* __restrict__ dend) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DiagEnd e = grad_tables_row<NET, ACT, R>(q0, n, nsets, w2, b2, tab, i);
  dend[i] = e.dw; dend[n + i] = e.db; dend[2 * n + i] = e.k;
}

// ---- the contraction on a rectangle
template <typename T>
struct XArgs {
  const T* k0; int64_t ldk0;      // X Z^T / d [n, ldk0]; its row is the point's index in X
  const T* wgt; int64_t ldw;      // [rows, ldw] weights; its row is the tile's own row index
  const int64_t* rowmap;          // nullptr: row r is point r; else point rowmap[r] (the square of Z against itself)
  const int64_t* piv;             // [m]: column a is point piv[a]
  int64_t rows, n; int m; int tcols;
  const T* tab; int nsets;
  double w2, b2, lw2, scale;
  double* partial;                // [gridDim.x][4]
};

template <typename T, int NET, int ACT>
__global__ void __launch_bounds__(256) lrg_contract_kernel(XArgs<T> a) {
  using R = T;
  const int tr = blockIdx.x / a.tcols, tc = blockIdx.x - tr * a.tcols;
  const int64_t row0 = (int64_t)tr * GT, n = a.n;
  const int col0 = tc * GT;
  const int tid = threadIdx.x;
  const int lc = tid % GT;
  const int w = __builtin_amdgcn_readfirstlane(tid / GT);
  constexpr int NR = GT / 4;
  const int ja = col0 + lc, jac = ja < a.m ? ja : a.m - 1;
  const int64_t j = a.piv[jac];
  const R w2 = (R)a.w2, b2 = (R)a.b2;
  R k[NR], dw[NR], db[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t iw = row0 + w + 4 * r, iwc = iw < a.rows ? iw : a.rows - 1;
    const int64_t i = a.rowmap ? a.rowmap[iwc] : iwc;
    k[r] = (R)a.k0[i * a.ldk0 + jac];
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
    const R cdw = ts[n + j], cdb = ts[2 * n + j], cra = ts[3 * n + j], crb = ts[4 * n + j];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t iw = row0 + w + 4 * r, iwc = iw < a.rows ? iw : a.rows - 1;   // wave-uniform
      const int64_t i = a.rowmap ? a.rowmap[iwc] : iwc;
      const R rq = ts[i], rdw = ts[n + i], rdb = ts[2 * n + i], rra = ts[3 * n + i], rrb = ts[4 * n + i];
      R kk = k[r], kw = dw[r], kb = db[r];
      if (NET == NET_MLP) {
        kw = fma(w2, kw, kk);
        kb = fma(w2, kb, R(1));
        kk = fma(w2, kk, b2);
      }
      if (i == j) kk = rq;                        // exact diagonal: the row's point is the column's pivot
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
  double acc[3] = {0.0, 0.0, 0.0};   // sum W dK/dw2, sum W dK/db2, sum W K
  const R lw2 = (R)a.lw2, scale = (R)a.scale;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t iw = row0 + w + 4 * r, iwc = iw < a.rows ? iw : a.rows - 1;
    const bool valid = iw < a.rows && ja < a.m;
    const R gm = valid ? scale * (R)a.wgt[iwc * a.ldw + jac] * lw2 : R(0);
    acc[0] += (double)(gm * dw[r]);
    acc[1] += (double)(gm * db[r]);
    acc[2] += (double)(gm * k[r]);
  }
  __shared__ double red[3][4];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 4) a.partial[(int64_t)blockIdx.x * 4 + tid] = tid < 3 ? (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]) : 0.0;
}

// per 256 rows: sum mu_i g_i lw2 (dK_ii/dw2, dK_ii/db2, K_ii) and sum g_i
__global__ void __launch_bounds__(256) lrg_diag_kernel(const double* __restrict__ g, const double* __restrict__ mg,
                                                       const double* __restrict__ dend, int64_t n, double lw2,
                                                       double* __restrict__ partial) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const double v = mg[i] * lw2;
    acc[0] = v * dend[i]; acc[1] = v * dend[n + i]; acc[2] = v * dend[2 * n + i]; acc[3] = g[i];
  }
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

// workgroup b: out[4 b + q] = the sum of its set of partials (thread t takes t, t + 256, ...; a butterfly; the four waves)
struct ReduceSets {
  const double* p[3]; int64_t cnt[3];
};
__global__ void __launch_bounds__(256) lrg_reduce_kernel(ReduceSets s, double* __restrict__ out) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x;
  const double* partial = s.p[blockIdx.x];
  const int64_t cnt = s.cnt[blockIdx.x];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t = tid; t < cnt; t += 256)
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
  if (tid < 4) out[blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// ------------------------------------------------------------------ host side
bool aligned16(const void* p, int64_t ld, size_t es) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * (int64_t)es) % 16 == 0; }

template <typename F>
int with_net_act(int net, int act, F&& f) {
  using std::integral_constant;
  if (net == SMN_NET_MLP && act == SMN_ACT_RELU) return f(integral_constant<int, NET_MLP>{}, integral_constant<int, ACT_RELU>{});
  if (net == SMN_NET_MLP) return f(integral_constant<int, NET_MLP>{}, integral_constant<int, ACT_ERF>{});
  if (act == SMN_ACT_RELU) return f(integral_constant<int, NET_RESNET>{}, integral_constant<int, ACT_RELU>{});
  return f(integral_constant<int, NET_RESNET>{}, integral_constant<int, ACT_ERF>{});
}

struct Carver {
  char* p;
  template <typename U>
  U* take(size_t count) {
    U* r = reinterpret_cast<U*>(p);
    p += al256(sizeof(U) * count);
    return r;
  }
};

template <typename T>
int lowrank_grad_t(smn_ctx* ctx, int dtype, int net, int act, int nsets, double w_std, double b_std, double last_w_std, const void* x_d,
                   int64_t n, int64_t ldx, int64_t d, const int64_t* pivots_h, const void* L_d, int64_t m, int64_t ldl,
                   const double* resid_d, double lambda, int fitc, const void* y_d, int64_t c, int64_t ldy, const double* C_d,
                   const double* beta_d, const double* R_d, int64_t ldr, double coef, double* terms_h) {
  const int64_t per16 = 16 / (int64_t)sizeof(T);
  const int64_t ldk = round_up(m, per16), ldz = round_up(d, per16);
  const int64_t trows = (n + GT - 1) / GT, tcols = (m + GT - 1) / GT, tsq = tcols;
  const int64_t nx = trows * tcols, nsq = tsq * tcols, ndg = (n + 255) / 256;
  if (nx > (int64_t)INT_MAX || (n + kRows - 1) / kRows > (int64_t)INT_MAX)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_lowrank_grad: n = %lld, m = %lld is too large", (long long)n, (long long)m);
  const size_t ntab = (size_t)n * kTabFields * (size_t)(nsets > 0 ? nsets : 1);
  // slot 9: the m x m side, fp64
  const size_t mm = (size_t)m * (size_t)m;
  void* sv = nullptr;
  SMN_TRY(smn_workspace(ctx, 9, 5 * al256(8 * mm) + al256(8 * (size_t)m * (size_t)c) + al256(8 * (size_t)m), &sv));
  Carver sc{static_cast<char*>(sv)};
  double* cinv = sc.take<double>(mm);    // C^-1, then A^-1
  double* cinvt = sc.take<double>(mm);   // C^-T
  double* rinv = sc.take<double>(mm);    // R^-1
  double* m1 = sc.take<double>(mm);      // A^-1 R^-1
  double* g2 = sc.take<double>(mm);      // L^T diag(mu g) L, the bracket, T
  double* bt = sc.take<double>((size_t)m * (size_t)c);
  int64_t* piv_d = sc.take<int64_t>((size_t)m);
  // slot 7: everything of size n
  const size_t big = 2 * al256(sizeof(T) * (size_t)n * (size_t)ldk) + al256(sizeof(T) * (size_t)m * (size_t)ldz) +
                     al256(sizeof(T) * (size_t)m * (size_t)ldk) + al256(8 * (size_t)n * (size_t)c) + 7 * al256(8 * (size_t)n) +
                     2 * al256(sizeof(T) * (size_t)(n > m ? n : m)) + al256(8 * ntab) + al256(32 * (size_t)nx) +
                     al256(32 * (size_t)nsq) + al256(32 * (size_t)ndg) + 256 + al256(8 * mm);
  void* bv = nullptr;
  SMN_TRY(smn_workspace(ctx, 7, big, &bv));
  Carver bc{static_cast<char*>(bv)};
  T* k0 = bc.take<T>((size_t)n * (size_t)ldk);
  T* U = bc.take<T>((size_t)n * (size_t)ldk);
  T* z = bc.take<T>((size_t)m * (size_t)ldz);
  T* tm = bc.take<T>((size_t)m * (size_t)ldk);
  double* alpha = bc.take<double>((size_t)n * (size_t)c);
  double* g = bc.take<double>((size_t)n);
  double* mg = bc.take<double>((size_t)n);
  double* q64 = bc.take<double>((size_t)n);
  double* dend = bc.take<double>(3 * (size_t)n);
  T* q1 = bc.take<T>((size_t)n);
  T* q2 = bc.take<T>((size_t)m);
  T* tab = reinterpret_cast<T*>(bc.take<double>(ntab));
  double* px = bc.take<double>(4 * (size_t)nx);
  double* psq = bc.take<double>(4 * (size_t)nsq);
  double* pdg = bc.take<double>(4 * (size_t)ndg);
  double* out_d = bc.take<double>(16);
  double* xt = bc.take<double>(mm);      // the transpose between the two solves of T
  hipStream_t st = ctx->stream;
  const unsigned gmm = (unsigned)((mm + 255) / 256);

  SMN_HIP(ctx, hipMemcpyAsync(piv_d, pivots_h, 8 * (size_t)m, hipMemcpyHostToDevice, st));
  // ---- the m x m side
  hipLaunchKernelGGL(lrg_identity_kernel, dim3(gmm), dim3(256), 0, st, cinv, (int)m);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_trsm(ctx, SMN_F64, C_d, m, m, cinv, m, m, 0));                        // C^-1
  SMN_TRY(smn_transpose(ctx, SMN_F64, cinvt, m, cinv, m, m, m));                    // C^-T
  SMN_TRY(smn_trsm(ctx, SMN_F64, C_d, m, m, cinv, m, m, 1));                        // A^-1 = C^-T C^-1
  hipLaunchKernelGGL(lrg_identity_kernel, dim3(gmm), dim3(256), 0, st, rinv, (int)m);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_trsm(ctx, SMN_F64, R_d, m, ldr, rinv, m, m, 0));                      // R^-1
  SMN_HIP(ctx, hipMemcpyAsync(m1, rinv, 8 * mm, hipMemcpyDeviceToDevice, st));
  SMN_TRY(smn_trsm(ctx, SMN_F64, C_d, m, m, m1, m, m, 0));
  SMN_TRY(smn_trsm(ctx, SMN_F64, C_d, m, m, m1, m, m, 1));                          // A^-1 R^-1
  SMN_HIP(ctx, hipMemcpyAsync(bt, beta_d, 8 * (size_t)m * (size_t)c, hipMemcpyDeviceToDevice, st));
  SMN_TRY(smn_trsm(ctx, SMN_F64, R_d, m, ldr, bt, c, c, 1));                        // R^-T beta
  // ---- row pass, Gram with the weights mu o g, U
  RowArgs<T> ra{};
  ra.L = static_cast<const T*>(L_d); ra.n = n; ra.m = (int)m; ra.ldl = ldl; ra.vec_ok = aligned16(L_d, ldl, sizeof(T)) ? 1 : 0;
  ra.resid = resid_d; ra.lambda = lambda; ra.fitc = fitc;
  ra.y = static_cast<const T*>(y_d); ra.ldy = ldy; ra.c = (int)c; ra.coef = coef;
  ra.cinvt = cinvt; ra.beta = beta_d; ra.m1 = m1; ra.m2 = rinv; ra.bt = bt;
  ra.alpha = alpha; ra.g = g; ra.mg = mg; ra.U = U; ra.ldu = ldk;
  const unsigned grows = (unsigned)((n + kRows - 1) / kRows);
  hipLaunchKernelGGL(lrg_row_kernel<T>, dim3(grows), dim3(256), 0, st, ra);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_lowrank_gram(ctx, dtype, L_d, n, m, ldl, mg, nullptr, 0, 0, g2, m, nullptr, nullptr));
  hipLaunchKernelGGL(lrg_u_kernel<T>, dim3(grows, (unsigned)((m + 255) / 256)), dim3(256), 0, st, ra);
  SMN_CHECK_LAUNCH(ctx);
  // ---- T = R^-T [bracket] R^-1, as -T's weights in the storage type
  hipLaunchKernelGGL(lrg_bracket_kernel, dim3(gmm), dim3(256), 0, st, g2, cinv, beta_d, (int)m, (int)c, coef);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_trsm(ctx, SMN_F64, R_d, m, ldr, g2, m, m, 1));                        // R^-T B
  SMN_TRY(smn_transpose(ctx, SMN_F64, xt, m, g2, m, m, m));                         // B R^-1 (B symmetric)
  SMN_TRY(smn_trsm(ctx, SMN_F64, R_d, m, ldr, xt, m, m, 1));                        // R^-T B R^-1
  hipLaunchKernelGGL(lrg_cast_matrix_kernel<T>, dim3(gmm), dim3(256), 0, st, xt, (int)m, tm, ldk);
  SMN_CHECK_LAUNCH(ctx);
  // ---- K0 = X Z^T / d and the tables
  hipLaunchKernelGGL(lrg_gather_kernel<T>, dim3((unsigned)((m * ldz + 255) / 256)), dim3(256), 0, st, static_cast<const T*>(x_d), ldx, d,
                     piv_d, (int)m, z, ldz);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(smn_gram(ctx, dtype, x_d, n, ldx, z, m, ldz, d, k0, ldk, q1, q2));
  hipLaunchKernelGGL(lrg_cast_q_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q1, q64, n);
  SMN_CHECK_LAUNCH(ctx);
  const double w2 = w_std * w_std, b2 = b_std * b_std, lw2 = last_w_std * last_w_std;
  XArgs<T> xa{};
  xa.k0 = k0; xa.ldk0 = ldk; xa.piv = piv_d; xa.n = n; xa.m = (int)m; xa.tcols = (int)tcols;
  xa.tab = tab; xa.nsets = nsets; xa.w2 = w2; xa.b2 = b2; xa.lw2 = lw2;
  SMN_TRY(with_net_act(net, act, [&](auto NET, auto ACT) {
    constexpr int N_ = decltype(NET)::value, A_ = decltype(ACT)::value;
    hipLaunchKernelGGL((lrg_tables_kernel<N_, A_, T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q64, n, nsets, w2, b2, tab, dend);
    SMN_CHECK_LAUNCH(ctx);
    XArgs<T> x1 = xa;
    x1.wgt = U; x1.ldw = ldk; x1.rowmap = nullptr; x1.rows = n; x1.scale = 2.0; x1.partial = px;
    hipLaunchKernelGGL((lrg_contract_kernel<T, N_, A_>), dim3((unsigned)nx), dim3(256), 0, st, x1);
    SMN_CHECK_LAUNCH(ctx);
    XArgs<T> x2 = xa;
    x2.wgt = tm; x2.ldw = ldk; x2.rowmap = piv_d; x2.rows = m; x2.scale = -1.0; x2.partial = psq;
    hipLaunchKernelGGL((lrg_contract_kernel<T, N_, A_>), dim3((unsigned)nsq), dim3(256), 0, st, x2);
    SMN_CHECK_LAUNCH(ctx);
    return (int)SMN_OK;
  }));
  hipLaunchKernelGGL(lrg_diag_kernel, dim3((unsigned)ndg), dim3(256), 0, st, g, mg, dend, n, lw2, pdg);
  SMN_CHECK_LAUNCH(ctx);
  ReduceSets rs{{px, psq, pdg}, {nx, nsq, ndg}};
  hipLaunchKernelGGL(lrg_reduce_kernel, dim3(3), dim3(256), 0, st, rs, out_d);
  SMN_CHECK_LAUNCH(ctx);
  double s[12];
  SMN_HIP(ctx, hipMemcpyAsync(s, out_d, sizeof s, hipMemcpyDeviceToHost, st));
  SMN_HIP(ctx, hipStreamSynchronize(st));
  terms_h[0] = ((s[0] + s[4]) + s[8]) * 2.0 * w_std;        // d/dw_std = 2 w d/dw^2
  terms_h[1] = ((s[1] + s[5]) + s[9]) * 2.0 * b_std;
  terms_h[2] = ((s[2] + s[6]) + s[10]) * 2.0 / last_w_std;  // K = lw^2 K_L
  terms_h[3] = s[11];                                       // dK^/d lambda = I
  return SMN_OK;
}

}  // namespace

extern "C" int smn_lowrank_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const int64_t* pivots_h,
                                const void* L_d, int64_t m, int64_t ldl, const double* resid_d, double lambda, int fitc,
                                const void* y_d, int64_t c, int64_t ldy, const double* C_d, const double* beta_d, const double* R_d,
                                int64_t ldr, double coef, double* terms_h) {
  const char* who = "smn_lowrank_grad";
  if (!ctx) return SMN_EINVAL;
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!x_d || !pivots_h || !L_d || !y_d || !C_d || !beta_d || !R_d || !terms_h) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (n <= 0 || m <= 0 || d <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: n = %lld, m = %lld, d = %lld", who, (long long)n, (long long)m, (long long)d);
  if (m > n) return smn_fail(ctx, SMN_EINVAL, "%s: m = %lld is above n = %lld", who, (long long)m, (long long)n);
  if (m > SMN_LOWRANK_MAX_RANK) return smn_fail(ctx, SMN_ENOTSUP, "%s: m = %lld is above SMN_LOWRANK_MAX_RANK = %d", who, (long long)m, SMN_LOWRANK_MAX_RANK);
  if (c < 1 || c > 48) return smn_fail(ctx, c > 48 ? SMN_ENOTSUP : SMN_EINVAL, "%s: c = %lld outside [1, 48]", who, (long long)c);
  SMN_CHECK_LD(ctx, who, ldx, d);
  SMN_CHECK_LD(ctx, who, ldl, m);
  SMN_CHECK_LD(ctx, who, ldy, c);
  SMN_CHECK_LD(ctx, who, ldr, m);
  if (!(lambda > 0.0) || !std::isfinite(lambda)) return smn_fail(ctx, SMN_EINVAL, "%s: lambda = %g is not a positive number", who, lambda);
  if (fitc != 0 && fitc != 1) return smn_fail(ctx, SMN_EINVAL, "%s: fitc = %d is neither 0 nor 1", who, fitc);
  if (fitc && !resid_d) return smn_fail(ctx, SMN_EINVAL, "%s: fitc = 1 needs resid_d", who);
  if (!std::isfinite(coef)) return smn_fail(ctx, SMN_EINVAL, "%s: coef = %g", who, coef);
  SMN_TRY(no_ntk_net(ctx, who, net));
  if (net != SMN_NET_MLP && net != SMN_NET_DENSE_RESNET) return smn_fail(ctx, SMN_EINVAL, "%s: unknown net %d", who, net);
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "%s: Unsupported act %d", who, act);
  if (num_hiddens < 0) return smn_fail(ctx, SMN_EINVAL, "%s: num_hiddens < 0", who);
  const int nsets = net == SMN_NET_MLP ? num_hiddens : num_hiddens + 1;
  if (nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "%s: num_hiddens too large (max %d activation layers)", who, kMaxSets);
  {
    std::vector<char> seen((size_t)n, 0);
    for (int64_t a = 0; a < m; ++a) {
      const int64_t p = pivots_h[a];
      if (p < 0 || p >= n) return smn_fail(ctx, SMN_EINVAL, "%s: pivots_h[%lld] = %lld outside [0, n = %lld)", who, (long long)a, (long long)p, (long long)n);
      if (seen[(size_t)p]) return smn_fail(ctx, SMN_EINVAL, "%s: pivot %lld is listed twice", who, (long long)p);
      seen[(size_t)p] = 1;
    }
  }
  SMN_ENTER(ctx);
  return by_dtype(dtype, [&](auto e) {
    return lowrank_grad_t<decltype(e)>(ctx, dtype, net, act, nsets, w_std, b_std, last_w_std, x_d, n, ldx, d, pivots_h, L_d, m, ldl, resid_d,
                                       lambda, fitc, y_d, c, ldy, C_d, beta_d, R_d, ldr, coef, terms_h);
  });
}
