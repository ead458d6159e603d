// fit_remove.hip — removing training points from a fitted posterior in O(N^2 k) without refitting (smn_fit_remove).
//
// The algebra (include/smnngp.h repeats it).  The state holds L (n x n, lower) with L L^T = K~ = K(X, X) + lambda I and beta^T =
// Y^T L^-T.  With J the k removed rows, R the kept ones in their order and H = L[R, :] ((n - k) x n): H H^T = K~_RR and Y_R = H
// beta.  For any orthogonal Q with H Q = [L' 0], L' lower triangular with a positive diagonal,
//     [ H      ]       [ L'      0     ]      L' L'^T = K(X_R, X_R) + lambda I   (lambda unchanged: the frozen ridge, absolute)
//     [ beta^T ] Q  =  [ beta'^T rho^T ]      beta' = L'^-1 Y_R,  rho is discarded
// -- an orthogonal triangularisation, not a hyperbolic downdate: backward stable, and it cannot fail for lack of positive
// definiteness.  Only the tail moves: with j1 = min J, columns left of j1 and rows above it are untouched, and in the trailing
// block new row i ends at column i + r(i), r(i) <= k the number of removed rows above it: lower triangular plus at most k
// super-diagonals.  It is reduced block by block: for new rows [s, s + b) only columns [s, s + b + k) are non-zero; an LQ
// factorisation of that b x (b + k) block gives Q_s, which is applied from the right to those columns of every row below (the
// beta rows among them); the k columns behind the block carry into the next step.  About m^2 (b + k)^2 / b flops for m kept
// rows behind j1, and a column passes through 1 + k / b transformations, not N / b: rounding does not pile up along the sweep.
//
// Sizes: b = kRB = 64 rows per step, KMAX = kRK = 32 rows per pass (a larger index set goes in passes of KMAX, the highest
// indices first, each pass a complete removal; a pass whose rows are the last rows of the state is the suffix path below).  The
// step width is always b + KMAX = 96 columns: the panel kernel keeps the 64 x 96 block and the explicit 96 x 96 Q_s in fp64 in
// LDS ((64 + 96) x 97 doubles = 121 KB of the 160 KB), and 96 is a K and an N the MFMA tile engine takes.  Inside the panel
// kernel the reflectors are as wide as the pass needs (4, 16 or 32 columns behind the diagonal).
//
// Where the sweep works: in CONTEXT WORKSPACE, not in the state's matrix.  The window starts at w0 = j1 rounded down to b (every
// panel is then aligned for the 16-byte loads; the rows between w0 and j1 are already triangular and cost a little work).  The
// gather pass copies the kept rows' columns [w0, n) -- upper triangle masked -- and the beta rows' into a zeroed matrix of
// (MB + 192) x (MB + 64) elements, MB = round_up(m, 64), m = kept rows from w0 on (slot 4; peak extra bytes = es (MB + 192)
// (MB + 64), at most the size of the factor itself: 1.07 GB in fp32 at n = 16384 when row 0 goes, nothing of it counted by
// smn_fit_info), the sweep runs there, and one pass writes L' (lower) and beta' back.  Compacting rows in place would have
// workgroups overwrite rows that others still read; the workspace costs two O(m n) copies beside an O(m^2 k) sweep.  The kept
// rows' columns LEFT of w0 do not change but move up by r(i) rows: one in-place pass in which a thread owns a 16-byte column
// group and walks down the rows (a row is only ever read at or below where it is written).  The fused form's padded x copy and
// q table are compacted through slot 0.  The freed rows [n - k, n) become identity padding again (zeros and a one), the
// invariant smn_fit_reserve and a failed append restore.
//
// Apply (the hot part): rows below x Q_s on the tile engine of gemm_nt.hpp in the state's dtype, a 128 x 96 tile per workgroup
// with K = 96.  The product reads and writes the same 96 columns of each row: a workgroup OWNS its 128 rows of the window over
// all 96 columns -- every operand read is behind the main loop's last barrier when the accumulators are stored --, so the
// product is written in place and needs no scratch panel or copy back.
//
// Two launches per step on the context's stream (panel, apply), no host synchronisation inside the sweep; one at the end for the
// totals, quad_c = sum beta'^2 and logdet = 2 sum log diag L' over the NEW state in fp64 in a fixed order (never the running sums
// minus |rho|^2: that cancels).  The same removal on the same state gives the same bits.
//
// Suffix removal (J = the last k rows, any k): no arithmetic touches L.  Rows [n - k, n) become padding, the beta columns and
// the x rows are cleared, the totals recomputed: the exact undo of an append.
//
// Afterwards grad_ready = false (ensure_grad_state rebuilds L', alpha^T and X^T at the next smn_fit_predict_grad); n_pad,
// capacity and the allocation stay as they are: a removal never allocates state memory and never shrinks it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fit_state.hpp"
#include "gemm_nt.hpp"

namespace {

constexpr int kRB = 64;            // b: rows per step
constexpr int kRK = 32;            // KMAX: rows removed per pass
constexpr int kRW = kRB + kRK;     // columns of a step
constexpr int kRLD = kRW + 1;      // LDS row stride in doubles (odd: a column walk over rows spreads over the banks)
constexpr size_t kPanelLds = sizeof(double) * ((size_t)(kRB + kRW) * kRLD + kRB);

// w [i, j] = L[src[i], w0 + j] (0 above the diagonal) for i < m, w [mb + k, j] = beta[k, w0 + j] for k < c; j < ncols.
// grid.y strides over the m + c rows.
template <typename T>
__global__ void remove_gather_kernel(T* __restrict__ w, int64_t ldw, const T* __restrict__ a, int64_t lda, const T* __restrict__ beta,
                                     const int64_t* __restrict__ src, int64_t w0, int64_t m, int64_t mb, int64_t ncols, int64_t c) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncols) return;
  for (int64_t i = blockIdx.y; i < m + c; i += gridDim.y) {
    if (i < m) {
      const int64_t r = src[i];
      w[i * ldw + j] = w0 + j <= r ? a[r * lda + w0 + j] : T(0);
    } else {
      w[(mb + i - m) * ldw + j] = beta[(i - m) * lda + w0 + j];
    }
  }
}

// L[w0 + i, w0 + j] = w [i, j] for j <= i < m;  beta[k, w0 + j] = j < m ? w [mb + k, j] : 0 for j < ncols.
template <typename T>
__global__ void remove_scatter_kernel(const T* __restrict__ w, int64_t ldw, T* __restrict__ a, int64_t lda, T* __restrict__ beta,
                                      int64_t w0, int64_t m, int64_t mb, int64_t ncols, int64_t c) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncols) return;
  for (int64_t i = blockIdx.y; i < m + c; i += gridDim.y) {
    if (i < m) {
      if (j <= i) a[(w0 + i) * lda + w0 + j] = w[i * ldw + j];
    } else {
      beta[(i - m) * lda + w0 + j] = j < m ? w[(mb + i - m) * ldw + j] : T(0);
    }
  }
}

// Columns [0, w0) of the kept rows move up: row w0 + i <- row src[i] for i0 <= i < m.  A thread owns one 16-byte column group and
// walks down, eight rows loaded before they are stored: src[i] >= w0 + i and src is increasing, so no row is read after it was
// overwritten, and no two threads share an address.
template <typename T>
__global__ void remove_compact_left_kernel(T* a, int64_t lda, const int64_t* __restrict__ src, int64_t w0, int64_t i0, int64_t m) {
  using V = typename Vec16<T>::type;
  const int64_t col = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * Vec16<T>::N;
  if (col >= w0) return;
  int64_t i = i0;
  for (; i + 8 <= m; i += 8) {
    V r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = *reinterpret_cast<const V*>(a + src[i + u] * lda + col);
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<V*>(a + (w0 + i + u) * lda + col) = r[u];
  }
  for (; i < m; ++i) {
    const V r = *reinterpret_cast<const V*>(a + src[i] * lda + col);
    *reinterpret_cast<V*>(a + (w0 + i) * lda + col) = r;
  }
}

// dst[i, 0:cols) = src_rows[src[i], 0:cols) for i < m (the padded x copy and, with cols = 1, the q table; through workspace)
template <typename T>
__global__ void remove_gather_rows_kernel(T* __restrict__ dst, const T* __restrict__ rows, int64_t cols, const int64_t* __restrict__ src,
                                          int64_t m) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  for (int64_t i = blockIdx.y; i < m; i += gridDim.y) dst[i * cols + j] = rows[src[i] * cols + j];
}

// The panel step, one workgroup of 256 threads: the LQ factorisation of the 64 x 96 block at (s, s) of the window by 64
// Householder reflectors in fp64 in LDS, Q_s accumulated explicitly.  KB >= the rows this pass removes (4, 16 or 32): row i of
// the block is non-zero in columns [.., i + KB] only, so reflector i acts on the KB + 1 columns [i, i + KB]; it is applied, one
// thread per row, to the block rows below and to the rows of Q it can reach (row r of Q is still e_r while r > i + KB).  The
// step is a chain of 64 dependent reflectors, so an iteration is kept to ONE barrier and no cross-lane traffic: every thread
// forms the reflector itself from row i (broadcast LDS reads, the same operations in the same order, hence the same bits in
// every thread), and row i is not written back -- its diagonal goes to dg[i], the rest of it is zero by construction.  The sign
// flip that makes the diagonal positive is a negation of column i, folded into the same pass: Q_s = prod_i H_i S_i.  Out: the
// block (L' in its first 64 columns, exact zeros right of the diagonal) in place, and qt [96, 96] with qt[j, k] = Q_s[k, j] --
// the NT product's second operand.
template <typename T, int KB>
__global__ void __launch_bounds__(256) remove_panel_kernel(T* __restrict__ w, int64_t ldw, int64_t s, T* __restrict__ qt) {
  static_assert(KB % 4 == 0 && KB <= kRK, "band width");
  extern __shared__ double lds[];
  double* blk = lds;                       // [kRB][kRLD]
  double* q = blk + kRB * kRLD;            // [kRW][kRLD]
  double* dg = q + kRW * kRLD;             // [kRB] the diagonal of L'
  const int tid = threadIdx.x;
  T* wb = w + s * ldw + s;
  for (int e = tid; e < kRB * kRW; e += 256) blk[(e / kRW) * kRLD + e % kRW] = (double)wb[(int64_t)(e / kRW) * ldw + e % kRW];
  for (int e = tid; e < kRW * kRW; e += 256) q[(e / kRW) * kRLD + e % kRW] = e / kRW == e % kRW ? 1.0 : 0.0;
  __syncthreads();
  for (int i = 0; i < kRB; ++i) {
    const int nb = kRB - 1 - i, nq = i + KB + 1 < kRW ? i + KB + 1 : kRW;
    if (tid < nb + nq || tid == 255) {
      const double* xr = blk + i * kRLD + i;
      double x[KB + 1];
#pragma unroll
      for (int l = 0; l <= KB; ++l) x[l] = xr[l];
      double sg[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int l = 1; l <= KB; ++l) sg[(l - 1) & 3] += x[l] * x[l];
      const double sig = (sg[0] + sg[1]) + (sg[2] + sg[3]), x0 = x[0];
      // x H = bet e_0, H = I - tau v v^T, v = (1, x[1:] scale); sig == 0: H = I.  The diagonal is then made +|.| by negating column i
      double tau = 0.0, scale = 0.0, diag = fabs(x0);
      if (sig != 0.0) {
        const double norm = sqrt(x0 * x0 + sig);
        const double bet = x0 >= 0.0 ? -norm : norm;
        tau = (bet - x0) / bet;
        scale = 1.0 / (x0 - bet);
        diag = norm;
      }
      const bool flip = sig != 0.0 ? x0 >= 0.0 : x0 < 0.0;
      if (tid == 255) {
        dg[i] = diag;
      } else if (tau != 0.0 || flip) {
        double* r = (tid < nb ? blk + (i + 1 + tid) * kRLD : q + (tid - nb) * kRLD) + i;
        if (tau != 0.0) {
          double rr[KB + 1];
#pragma unroll
          for (int l = 0; l <= KB; ++l) rr[l] = r[l];
          double ac[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int l = 1; l <= KB; ++l) ac[(l - 1) & 3] += rr[l] * x[l];
          const double dot = tau * (rr[0] + scale * ((ac[0] + ac[1]) + (ac[2] + ac[3]))), ds = dot * scale;
          const double r0 = rr[0] - dot;
          r[0] = flip ? -r0 : r0;
#pragma unroll
          for (int l = 1; l <= KB; ++l) r[l] = rr[l] - ds * x[l];
        } else {
          r[0] = -r[0];
        }
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < kRB * kRW; e += 256) {
    const int row = e / kRW, col = e % kRW;
    wb[(int64_t)row * ldw + col] = (T)(col < row ? blk[row * kRLD + col] : col == row ? dg[row] : 0.0);
  }
  for (int e = tid; e < kRW * kRW; e += 256) qt[e] = (T)q[(e % kRW) * kRLD + e / kRW];
}

// The apply step: rows [row0 + 128 blockIdx.x, + 128) of the window, columns [s, s + 96) <- the same x Q_s, in place (this
// workgroup owns those rows over all 96 columns; see the header).
template <typename T>
__global__ void __launch_bounds__(256) remove_apply_kernel(T* w, int64_t ldw, int64_t row0, int64_t s, const T* __restrict__ qt) {
  using Tile = TileNT<T, 128, kRW, 2>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* wr = w + (row0 + (int64_t)blockIdx.x * 128) * ldw + s;
  Tile tile;
  tile.zero();
  tile.template mainloop<0>(wr, ldw, qt, kRW, kRW, smem);
  tile.for_each([&](int mm, int nn, int i, int lr, int lc) { wr[(int64_t)lr * ldw + lc] = tile.acc[mm][nn][i]; });
}

// quad[k] = sum_j beta[k, j]^2, logdet = 2 sum_j log L[j, j] over j < n: fp64, thread t takes j = t, t + 256, ... in order, the
// 256 partial sums meet in a fixed tree.  Published in the mailbox's layout {logdet, info = 0, quad[0 .. c)}.
template <typename T>
__global__ void __launch_bounds__(256) remove_totals_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ beta, int64_t n,
                                                            int c, double* __restrict__ mail) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  for (int k = -1; k < c; ++k) {
    double sum = 0.0;
    for (int64_t j = tid; j < n; j += 256) {
      if (k < 0) sum += log((double)a[j * lda + j]);
      else { const double b = (double)beta[(int64_t)k * lda + j]; sum += b * b; }
    }
    red[tid] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      if (k < 0) { mail[0] = 2.0 * red[0]; mail[1] = 0.0; }
      else mail[2 + k] = red[0];
    }
    __syncthreads();
  }
}

// rows [n_new, n_old) of the factor back to identity padding; the beta columns, those columns of the test rows and (fused) the
// x rows and q entries cleared
int clear_freed_rows(smn_fit* f, int64_t n_new, int64_t n_old, bool clear_beta) {
  smn_ctx* ctx = f->ctx;
  const size_t es = f->es(), pitch = es * (size_t)f->lda;
  SMN_HIP(ctx, hipMemset2DAsync(f->at(n_new, 0), pitch, 0, es * (size_t)f->n_pad, (size_t)(n_old - n_new), ctx->stream));
  SMN_TRY(fill_identity_pad(ctx, f->dtype, f->a, f->lda, n_old, n_new));
  if (clear_beta)
    SMN_HIP(ctx, hipMemset2DAsync(f->at(f->beta_row(), n_new), pitch, 0, es * (size_t)(n_old - n_new), (size_t)f->c, ctx->stream));
  // the test rows: a chunk's cross kernel is written in columns [0, n) only, and the solve reads the whole padded row -- what an
  // earlier prediction left in the columns that are padding again has to go
  SMN_HIP(ctx, hipMemset2DAsync(f->at(f->n_pad, n_new), pitch, 0, es * (size_t)(n_old - n_new), (size_t)f->cap_pad, ctx->stream));
  if (f->fused) {
    SMN_HIP(ctx, hipMemsetAsync(f->q() + n_new, 0, sizeof(double) * (size_t)(n_old - n_new), ctx->stream));
    SMN_HIP(ctx, hipMemsetAsync(f->xp() + es * (size_t)(n_new * f->kp), 0, es * (size_t)(n_old - n_new) * (size_t)f->kp, ctx->stream));
  }
  return SMN_OK;
}

// One pass: the rows `gone` (sorted, at most KMAX of them, not the state's last rows) leave.  src_h is the caller's to keep
// alive until the stream has been synchronised (it is the host source of an asynchronous upload).
template <typename T>
int remove_pass(smn_fit* f, const std::vector<int64_t>& gone, std::vector<int64_t>& src_h) {
  smn_ctx* ctx = f->ctx;
  const int64_t n_old = f->n, k = (int64_t)gone.size(), n_new = n_old - k;
  const int64_t w0 = gone[0] / kRB * kRB, m = n_new - w0, mb = round_up(m, kRB), ncols = n_old - w0;
  const int64_t ldw = mb + kRB, rows_w = mb + kRB + 128;
  src_h.resize((size_t)m);
  {
    size_t g = 0;
    int64_t i = 0;
    for (int64_t r = w0; r < n_old; ++r) {
      if (g < gone.size() && gone[g] == r) { ++g; continue; }
      src_h[(size_t)i++] = r;
    }
  }
  const size_t es = sizeof(T);
  const size_t map_bytes = round_up((int64_t)sizeof(int64_t) * m, 256), qt_bytes = round_up((int64_t)es * kRW * kRW, 256);
  const size_t x_bytes = f->fused ? sizeof(double) * (size_t)m + es * (size_t)m * (size_t)f->kp : 0;
  void *w0p = nullptr, *wsp = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, map_bytes + qt_bytes + x_bytes + 256, &w0p));
  SMN_TRY(smn_workspace(ctx, 4, es * (size_t)rows_w * (size_t)ldw, &wsp));
  void (*panel)(T*, int64_t, int64_t, T*) = k <= 4 ? remove_panel_kernel<T, 4> : k <= 16 ? remove_panel_kernel<T, 16> : remove_panel_kernel<T, kRK>;
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(panel), kPanelLds));
  int64_t* src_d = static_cast<int64_t*>(w0p);
  T* qt = reinterpret_cast<T*>(static_cast<char*>(w0p) + map_bytes);
  char* xtmp = static_cast<char*>(w0p) + map_bytes + qt_bytes;
  T* w = static_cast<T*>(wsp);
  T* a = static_cast<T*>(f->a);
  T* beta = reinterpret_cast<T*>(f->at(f->beta_row(), 0));
  hipStream_t st = ctx->stream;
  ProfScope ps(ctx, PROF_MISC, st);
  SMN_HIP(ctx, hipMemcpyAsync(src_d, src_h.data(), sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, st));
  SMN_HIP(ctx, hipMemsetAsync(w, 0, es * (size_t)rows_w * (size_t)ldw, st));
  const dim3 gw((unsigned)((ncols + 255) / 256), (unsigned)std::min<int64_t>(m + f->c, 32768));
  hipLaunchKernelGGL(remove_gather_kernel<T>, gw, dim3(256), 0, st, w, ldw, a, f->lda, beta, src_d, w0, m, mb, ncols, f->c);
  SMN_CHECK_LAUNCH(ctx);
  // the sweep: two launches per step
  constexpr size_t kApplyLds = TileNT<T, 128, kRW, 2>::LDS_BYTES;
  for (int64_t s = 0; s < mb; s += kRB) {
    hipLaunchKernelGGL(panel, dim3(1), dim3(256), kPanelLds, st, w, ldw, s, qt);
    const int64_t row0 = s + kRB, tiles = (mb + kRB - row0 + 127) / 128;
    hipLaunchKernelGGL(remove_apply_kernel<T>, dim3((unsigned)tiles), dim3(256), kApplyLds, st, w, ldw, row0, s, qt);
  }
  SMN_CHECK_LAUNCH(ctx);
  // the kept rows' columns left of the window, then the window and the beta rows
  const int64_t i0 = gone[0] - w0;
  if (w0 > 0) {
    const int64_t groups = w0 / Vec16<T>::N;
    hipLaunchKernelGGL(remove_compact_left_kernel<T>, dim3((unsigned)((groups + 63) / 64)), dim3(64), 0, st, a, f->lda, src_d, w0, i0, m);
    SMN_CHECK_LAUNCH(ctx);
  }
  hipLaunchKernelGGL(remove_scatter_kernel<T>, gw, dim3(256), 0, st, w, ldw, a, f->lda, beta, w0, m, mb, ncols, f->c);
  SMN_CHECK_LAUNCH(ctx);
  if (f->fused) {
    double* qtmp = reinterpret_cast<double*>(xtmp);
    T* xrows = reinterpret_cast<T*>(xtmp + sizeof(double) * (size_t)m);
    hipLaunchKernelGGL(remove_gather_rows_kernel<double>, dim3(1, (unsigned)std::min<int64_t>(m, 32768)), dim3(64), 0, st, qtmp, f->q(), (int64_t)1, src_d, m);
    hipLaunchKernelGGL(remove_gather_rows_kernel<T>, dim3((unsigned)((f->kp + 255) / 256), (unsigned)std::min<int64_t>(m, 32768)), dim3(256), 0, st, xrows,
                       reinterpret_cast<const T*>(f->xp()), f->kp, src_d, m);
    SMN_CHECK_LAUNCH(ctx);
    SMN_HIP(ctx, hipMemcpyAsync(f->q() + w0, qtmp, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
    SMN_HIP(ctx, hipMemcpyAsync(f->xp() + es * (size_t)(w0 * f->kp), xrows, es * (size_t)m * (size_t)f->kp, hipMemcpyDeviceToDevice, st));
  }
  SMN_TRY(clear_freed_rows(f, n_new, n_old, false));   // (the scatter pass has cleared the beta columns)
  f->n = n_new;
  return SMN_OK;
}

}  // namespace

extern "C" int smn_fit_remove(smn_fit* fit, const int64_t* idx_h, int64_t k, double* quad_h, double* logdet_h) {
  if (!fit || !fit->ctx) return SMN_EINVAL;
  smn_ctx* ctx = fit->ctx;
  SMN_ENTER(ctx);
  const char* who = "smn_fit_remove";
  const int64_t n = fit->n;
  if (k < 1) return smn_fail(ctx, SMN_EINVAL, "%s: k = %lld must be at least 1", who, (long long)k);
  if (!idx_h) return smn_fail(ctx, SMN_EINVAL, "%s: idx_h is NULL", who);
  if (k >= n)
    return smn_fail(ctx, SMN_EINVAL, "%s: k = %lld of the state's n = %lld training rows: a state keeps at least one", who, (long long)k,
                    (long long)n);
  if (fit->info != 0)
    return smn_fail(ctx, SMN_EINVAL, "%s: the state's matrix was not positive definite (info = %d): nothing to remove from", who, fit->info);
  std::vector<int64_t> idx(idx_h, idx_h + k);
  for (int64_t v : idx)
    if (v < 0 || v >= n) return smn_fail(ctx, SMN_EINVAL, "%s: index %lld is outside [0, %lld)", who, (long long)v, (long long)n);
  std::sort(idx.begin(), idx.end());
  for (int64_t i = 1; i < k; ++i)
    if (idx[(size_t)i] == idx[(size_t)i - 1]) return smn_fail(ctx, SMN_EINVAL, "%s: index %lld is given twice", who, (long long)idx[(size_t)i]);
  {   // workspace of the largest pass (the one with the lowest indices) before the first launch: a slot that has to grow
      // synchronises the stream, so it grows here and not between two passes
    const size_t es = fit->es();
    const int64_t m_max = n - idx[0] / kRB * kRB, mb = round_up(m_max, kRB);
    void* w = nullptr;
    SMN_TRY(smn_workspace(ctx, 0, (size_t)round_up((int64_t)sizeof(int64_t) * m_max, 256) + (size_t)round_up((int64_t)es * kRW * kRW, 256) +
                                      sizeof(double) * (size_t)m_max + es * (size_t)m_max * (size_t)fit->kp + 256, &w));
    SMN_TRY(smn_workspace(ctx, 4, es * (size_t)(mb + kRB + 128) * (size_t)(mb + kRB), &w));
  }
  // passes from the highest indices down: the indices of what is still to go do not move
  std::vector<std::vector<int64_t>> maps;   // the passes' upload sources, alive until the synchronisation below
  int64_t hi = k;
  while (hi > 0) {
    // the trailing run of idx[0, hi) that is exactly the state's last rows: the suffix path, whatever its length
    int64_t run = 0;
    while (run < hi && idx[(size_t)(hi - 1 - run)] == fit->n - 1 - run) ++run;
    if (run > 0) {
      SMN_TRY(clear_freed_rows(fit, fit->n - run, fit->n, true));
      fit->n -= run;
      hi -= run;
      continue;
    }
    const int64_t lo = std::max<int64_t>(0, hi - kRK);
    const std::vector<int64_t> gone(idx.begin() + lo, idx.begin() + hi);
    maps.emplace_back();
    const int rc = by_dtype(fit->dtype, [&](auto e) { return remove_pass<decltype(e)>(fit, gone, maps.back()); });
    if (rc != SMN_OK) {
      (void)hipStreamSynchronize(ctx->stream);
      return rc;
    }
    hi = lo;
  }
  fit->grad_ready = false;
  by_dtype(fit->dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(remove_totals_kernel<T>, dim3(1), dim3(256), 0, ctx->stream, static_cast<const T*>(fit->a), fit->lda,
                       reinterpret_cast<const T*>(fit->at(fit->beta_row(), 0)), fit->n, (int)fit->c, ctx->d_mail);
  });
  SMN_CHECK_LAUNCH(ctx);
  HeadScalars h;
  SMN_TRY(fetch_mail(ctx, (int)fit->c, &h));
  for (int64_t c = 0; c < fit->c; ++c) fit->quad[c] = h.quad[c];
  fit->logdet = h.logdet;
  for (int64_t c = 0; c < fit->c && quad_h; ++c) quad_h[c] = fit->quad[c];
  if (logdet_h) *logdet_h = fit->logdet;
  return SMN_OK;
}
