// lowrank.hip — regression on a rank-M factor L [n, m] of the kernel matrix (csrc/pchol.hip): K^ = L L^T + D with
// D = diag(d), d_i = fitc max(resid_i, 0) + lambda, evaluated by the Woodbury identity at O(n m^2) work and O(n m) memory.
//     W = D^-1,  G = L^T W L,  B = L^T W Y,  s_k = sum_i w_i y_ik^2,  A = I + G = C C^T
//     y_k^T K^^-1 y_k = s_k - |C^-1 B_k|^2,   log|K^| = log|A| + sum_i log d_i,   beta = A^-1 B
//     prediction at x*:  phi = R^-1 K(Z, x*)  (R = L[pivots, :], lower triangular: K(Z, Z) = R R^T),
//                        mean = phi^T beta,  var = k** - |phi|^2 + |C^-1 phi|^2      (the DTC / FITC predictive)
//
// The weighted Gram G contracts over the ROWS of a row-major [n, m] matrix, which the NT tile engine cannot do without a
// transposed copy.  lowrank_gram_kernel does it in place: for v_mfma_*_16x16x4 both operands are column slices of the same
// four rows of L -- lane l holds row (l >> 4) of its column -- so a lane reads along k at a fixed column and nothing is
// transposed.  One 16-byte load per lane and row gives the lane V = 4 (f32) / 2 (f64) adjacent columns; MFMA tile f of a wave
// block therefore holds the columns V r + f (r: the tile's row index), a permutation the store undoes.  A workgroup is 2 x 2
// waves on a 32 V x 32 V block of G; only blocks a >= b are computed, and of a diagonal block's four wave blocks the upper one
// is skipped.  Operands come straight from global memory: the four waves share rows through the cache, and a step of 16 rows
// is 8 loads against 64 (f32) / 16 (f64) MFMAs.
//
// Determinism: the rows are cut into splits of kSplit = SMN_LOWRANK_SPLIT rows, a build-time constant.  Split s of block t
// accumulates in the MFMA's own precision (f32: weight rounded to f32, w l rounded, then the MFMA's products and sums) and
// leaves its block in the workspace; lowrank_gram_reduce_kernel adds the splits in ascending order in fp64 and writes G with
// its upper half mirrored from the lower.  No floating-point atomics; the order of every sum is fixed by (n, m) alone, so two
// calls give the same bits and the bits depend neither on ldl nor on the alignment (the scalar load path feeds the same
// registers) nor on a grid.  B and s are small: plain fp64 sums per split, rows ascending, reduced the same way.
//
// The M x M side -- A, its factor C, beta, the two triangular solves of the read-out -- is fp64 for both storage types, as
// SVSP's I x I side is: it is O(m^3) beside O(n m^2), and 1 + G_aa reaches 1 / lambda, where an f32 factor would lose what
// the f32 Gram still has.  The factorisation is smn_cholesky in f64 on [A B; B^T 0]: its appended rows come back as
// (C^-1 B)^T.
#include <cfloat>
#include <cmath>
#include <vector>

#include "gemm_nt.hpp"
#include "internal.hpp"

namespace {

constexpr int kSplit = SMN_LOWRANK_SPLIT;
constexpr int kRowsPerIter = 16;    // rows of L per loop iteration of the Gram kernel: 4 MFMA k-steps
constexpr int kReadoutCols = 4;     // test points one wave carries through the two triangular solves
constexpr int kYChunk = 8;          // target columns one pass of the B kernel keeps in registers

template <typename T>
struct GramCfg {
  static constexpr int V = Vec16<T>::N;
  static constexpr int WB = 16 * V;   // columns of a wave block
  static constexpr int BT = 2 * WB;   // columns of a workgroup block
};

// columns [c, c + V) of a row of L; zero behind m
template <typename T>
__device__ __forceinline__ typename Vec16<T>::type load_cols(const T* __restrict__ row, int c, int m, bool vec_ok) {
  constexpr int V = Vec16<T>::N;
  typename Vec16<T>::type v;
  if (vec_ok && c + V <= m) {
    v = *reinterpret_cast<const typename Vec16<T>::type*>(row + c);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = c + k < m ? row[c + k] : T(0);
  }
  return v;
}

template <typename T>
__global__ void __launch_bounds__(256) lowrank_gram_kernel(const T* __restrict__ L, int64_t n, int m, int64_t ldl, int vec_ok,
                                                           const double* __restrict__ w, T* __restrict__ part, int npairs,
                                                           int64_t total) {
  using M = Mfma<T>;
  using Cfg = GramCfg<T>;
  using vec_t = typename Vec16<T>::type;
  constexpr int V = Cfg::V, WB = Cfg::WB, BT = Cfg::BT, U = kRowsPerIter / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  // Work item l = split * npairs + block pair: the pairs of one split read the same kSplit rows of L.  Workgroups are dealt
  // round-robin over the 8 XCDs, so XCD x takes the contiguous share [x chunk, (x + 1) chunk) of the items: the ~npairs
  // workgroups that share a slab of rows run side by side behind one L2 (placement only: any order computes the same blocks).
  const int64_t chunk = (int64_t)(gridDim.x >> 3);
  const int64_t item = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
  if (item >= total) return;
  const int64_t split = item / npairs;
  const int pair = (int)(item - split * npairs);
  int ta, tb;
  tri_decode((int64_t)pair, ta, tb);
  const int ca0 = ta * BT + wr * WB, cb0 = tb * BT + wc * WB;
  if (ca0 >= m || cb0 >= m || cb0 > ca0 + WB - 1) return;   // nothing of this wave block is read by the reduction
  const int mi = lane & 15, kk = lane >> 4;
  const int ca = ca0 + V * mi, cb = cb0 + V * mi;
  const int64_t r0 = split * kSplit;
  const int64_t r1 = r0 + kSplit < n ? r0 + kSplit : n;

  typename M::acc_t acc[V][V];
#pragma unroll
  for (int fa = 0; fa < V; ++fa)
#pragma unroll
    for (int fb = 0; fb < V; ++fb)
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) acc[fa][fb][i] = T(0);

  for (int64_t i0 = r0; i0 < r1; i0 += kRowsPerIter) {
    vec_t a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = i0 + 4 * u + kk;
      if (row < r1) {
        const T* lr = L + row * ldl;
        a[u] = load_cols<T>(lr, ca, m, vec_ok != 0);
        b[u] = load_cols<T>(lr, cb, m, vec_ok != 0);
        if (w) {
          const T wt = (T)w[row];
#pragma unroll
          for (int k = 0; k < V; ++k) a[u][k] *= wt;
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          a[u][k] = T(0); b[u][k] = T(0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int fa = 0; fa < V; ++fa)
#pragma unroll
        for (int fb = 0; fb < V; ++fb) {
          if constexpr (sizeof(T) == 4) acc[fa][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][fa], b[u][fb], acc[fa][fb], 0, 0, 0);
          else acc[fa][fb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][fa], b[u][fb], acc[fa][fb], 0, 0, 0);
        }
  }

  // MFMA tile (fa, fb), row r, column q  ->  G block element (V r + fa, V q + fb): the V tiles fb of a lane are adjacent
  T* blk = part + item * (int64_t)(BT * BT);
#pragma unroll
  for (int fa = 0; fa < V; ++fa)
#pragma unroll
    for (int i = 0; i < M::ACC; ++i) {
      const int la = wr * WB + V * M::acc_row(lane, i) + fa;
      const int lb = wc * WB + V * M::acc_col(lane);
      vec_t o;
#pragma unroll
      for (int fb = 0; fb < V; ++fb) o[fb] = acc[fa][fb][i];
      *reinterpret_cast<vec_t*>(blk + la * BT + lb) = o;
    }
}

// G[a, b] = G[b, a] = sum over the splits, ascending, in fp64
template <typename T>
__global__ void __launch_bounds__(256) lowrank_gram_reduce_kernel(const T* __restrict__ part, int64_t splits, int npairs, int m,
                                                                  double* __restrict__ G, int64_t ldg) {
  constexpr int BT = GramCfg<T>::BT;
  int ta, tb;
  tri_decode((int64_t)blockIdx.y, ta, tb);
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int a = ta * BT + e / BT, b = tb * BT + e % BT;
  if (a >= m || b >= m || b > a) return;
  const T* p = part + (int64_t)blockIdx.y * (BT * BT) + e;
  const int64_t stride = (int64_t)npairs * (BT * BT);
  double sum = 0.0;
  for (int64_t s = 0; s < splits; ++s) sum += (double)p[s * stride];
  G[(int64_t)a * ldg + b] = sum;
  G[(int64_t)b * ldg + a] = sum;
}

// One split of B = L^T W Y and of s_k = sum_i w_i y_ik^2 in fp64, rows ascending: thread = column a of L.
template <typename T>
__global__ void __launch_bounds__(256) lowrank_by_kernel(const T* __restrict__ L, int64_t n, int m, int64_t ldl,
                                                         const double* __restrict__ w, const T* __restrict__ y, int c, int64_t ldy,
                                                         double* __restrict__ part_b, double* __restrict__ part_s) {
  const int64_t s = blockIdx.x;
  const int64_t r0 = s * kSplit;
  const int64_t r1 = r0 + kSplit < n ? r0 + kSplit : n;
  const int a = blockIdx.y * 256 + threadIdx.x;
  if (blockIdx.y == 0 && (int)threadIdx.x < c) {
    const int k = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      const double yv = (double)y[i * ldy + k];
      acc = fma((w ? w[i] : 1.0) * yv, yv, acc);
    }
    part_s[s * c + k] = acc;
  }
  if (a >= m) return;
  for (int k0 = 0; k0 < c; k0 += kYChunk) {
    double acc[kYChunk];
#pragma unroll
    for (int q = 0; q < kYChunk; ++q) acc[q] = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      const double wl = (w ? w[i] : 1.0) * (double)L[i * ldl + a];
#pragma unroll
      for (int q = 0; q < kYChunk; ++q)
        if (k0 + q < c) acc[q] = fma(wl, (double)y[i * ldy + k0 + q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < kYChunk; ++q)
      if (k0 + q < c) part_b[(s * m + a) * c + k0 + q] = acc[q];
  }
}

// out[e] = sum over the splits, ascending, of part[s * count + e]
__global__ void lowrank_sum_splits_kernel(const double* __restrict__ part, int64_t splits, int64_t count, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  double sum = 0.0;
  for (int64_t s = 0; s < splits; ++s) sum += part[s * count + e];
  out[e] = sum;
}

// w_i = 1 / d_i, d_i = fitc max(resid_i, 0) + lambda
__global__ void lowrank_weights_kernel(const double* __restrict__ resid, int64_t n, double lambda, int fitc, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = (fitc && resid ? fmax(resid[i], 0.0) : 0.0) + lambda;
  w[i] = 1.0 / d;
}

// One workgroup: *out = sum_i log d_i (thread t takes i = t, t + 256, ...; then a tree)
__global__ void __launch_bounds__(256) lowrank_logd_kernel(const double* __restrict__ resid, int64_t n, double lambda, int fitc,
                                                           double* __restrict__ out) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double sum = 0.0;
  for (int64_t i = t; i < n; i += 256) sum += log((fitc && resid ? fmax(resid[i], 0.0) : 0.0) + lambda);
  sh[t] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) *out = sh[0];
}

// A = I + G in the leading block of aug [m + c, lda]; B^T in the appended rows; zeros behind them
__global__ void lowrank_aug_kernel(double* __restrict__ aug, int64_t lda, int m, int c, const double* __restrict__ B) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t mc = (int64_t)m + c;
  if (e >= (int64_t)c * mc + m) return;
  if (e < m) {
    aug[e * lda + e] += 1.0;
    return;
  }
  const int64_t f = e - m;
  const int k = (int)(f / mc), j = (int)(f % mc);
  aug[(int64_t)(m + k) * lda + j] = j < m ? B[(int64_t)j * c + k] : 0.0;
}

// C (lower, zeros above), Z^T = (C^-1 B) as [m, c] and quad_k = s_k - |Z_k|^2 out of the factored aug; info != 0: NaN
__global__ void lowrank_unpack_kernel(const double* __restrict__ aug, int64_t lda, int m, int c, const double* __restrict__ s,
                                      int failed, double* __restrict__ Cf, double* __restrict__ zt, double* __restrict__ quad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t mm = (int64_t)m * m, mc = (int64_t)m * c;
  const double nan = __builtin_nan("");
  if (e < mm) {
    const int i = (int)(e / m), j = (int)(e % m);
    Cf[e] = failed ? nan : (j <= i ? aug[(int64_t)i * lda + j] : 0.0);
  } else if (e < mm + mc) {
    const int64_t f = e - mm;
    const int j = (int)(f / c), k = (int)(f % c);
    zt[f] = failed ? nan : aug[(int64_t)(m + k) * lda + j];
  } else if (e < mm + mc + c) {
    const int k = (int)(e - mm - mc);
    double z2 = 0.0;
    for (int j = 0; j < m; ++j) {
      const double z = aug[(int64_t)(m + k) * lda + j];
      z2 = fma(z, z, z2);
    }
    quad[k] = failed ? nan : s[k] - z2;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// x <- T^-1 x for the kReadoutCols vectors in sh (T lower triangular [m, ldt]): row i's dot product is taken by the wave, lane
// l over the columns l, l + 64, ... ascending, then the butterfly; the order does not depend on which vectors share the wave.
__device__ __forceinline__ void solve_lower(const double* __restrict__ Tm, int64_t ldt, int m, double* sh, int lane) {
  for (int i = 0; i < m; ++i) {
    const double* ti = Tm + (int64_t)i * ldt;
    double acc[kReadoutCols];
#pragma unroll
    for (int q = 0; q < kReadoutCols; ++q) acc[q] = 0.0;
    for (int j = lane; j < i; j += 64) {
      const double tv = ti[j];
#pragma unroll
      for (int q = 0; q < kReadoutCols; ++q) acc[q] = fma(tv, sh[q * m + j], acc[q]);
    }
    const double tii = ti[i];
    double v[kReadoutCols];
#pragma unroll
    for (int q = 0; q < kReadoutCols; ++q) v[q] = (sh[q * m + i] - wave_sum(acc[q])) / tii;
    if (lane == (i & 63)) {
#pragma unroll
      for (int q = 0; q < kReadoutCols; ++q) sh[q * m + i] = v[q];
    }
    __syncthreads();   // (one wave per workgroup) x_i is in place before row i + 1 reads it
  }
}

// One wave = kReadoutCols test points.  sh [kReadoutCols][m] holds K(Z, x*), then phi, then C^-1 phi, in place.
template <typename T>
__global__ void __launch_bounds__(64) lowrank_readout_kernel(const T* __restrict__ kzt, int64_t ldk, const T* __restrict__ ktt,
                                                             int64_t t, int m, const double* __restrict__ R, int64_t ldr,
                                                             const double* __restrict__ Cf, const double* __restrict__ beta, int c,
                                                             T* __restrict__ mean, T* __restrict__ var) {
  extern __shared__ double sh[];
  const int lane = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * kReadoutCols;
  for (int i = lane; i < m; i += 64)
#pragma unroll
    for (int q = 0; q < kReadoutCols; ++q) sh[q * m + i] = j0 + q < t ? (double)kzt[(int64_t)i * ldk + j0 + q] : 0.0;
  __syncthreads();
  solve_lower(R, ldr, m, sh, lane);
  double nphi[kReadoutCols];
#pragma unroll
  for (int q = 0; q < kReadoutCols; ++q) {
    double a = 0.0;
    for (int i = lane; i < m; i += 64) a = fma(sh[q * m + i], sh[q * m + i], a);
    nphi[q] = wave_sum(a);
  }
  for (int k = 0; k < c; ++k)
#pragma unroll
    for (int q = 0; q < kReadoutCols; ++q) {
      double a = 0.0;
      for (int i = lane; i < m; i += 64) a = fma(sh[q * m + i], beta[(int64_t)i * c + k], a);
      a = wave_sum(a);
      if (lane == 0 && j0 + q < t) mean[(j0 + q) * c + k] = (T)a;
    }
  __syncthreads();
  solve_lower(Cf, m, m, sh, lane);
#pragma unroll
  for (int q = 0; q < kReadoutCols; ++q) {
    double a = 0.0;
    for (int i = lane; i < m; i += 64) a = fma(sh[q * m + i], sh[q * m + i], a);
    a = wave_sum(a);
    if (lane == 0 && j0 + q < t) var[j0 + q] = (T)((double)ktt[j0 + q] - nphi[q] + a);
  }
}

// ------------------------------------------------------------------ host side
bool aligned16(const void* p, int64_t ld, size_t es) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * (int64_t)es) % 16 == 0; }

int check_factor(smn_ctx* ctx, const char* who, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!L_d) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (n <= 0 || m <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: n = %lld, m = %lld", who, (long long)n, (long long)m);
  if (m > SMN_LOWRANK_MAX_RANK)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: m = %lld is above SMN_LOWRANK_MAX_RANK = %d", who, (long long)m, SMN_LOWRANK_MAX_RANK);
  SMN_CHECK_LD(ctx, who, ldl, m);
  if ((n + kSplit - 1) / kSplit > (int64_t)INT_MAX) return smn_fail(ctx, SMN_ENOTSUP, "%s: n = %lld is too large", who, (long long)n);
  return SMN_OK;
}

int check_targets(smn_ctx* ctx, const char* who, const void* y_d, int64_t c, int64_t cmin, int64_t ldy) {
  if (c < cmin || c > 48) return smn_fail(ctx, c > 48 ? SMN_ENOTSUP : SMN_EINVAL, "%s: c = %lld outside [%lld, 48]", who, (long long)c, (long long)cmin);
  if (c > 0 && !y_d) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (c > 0) SMN_CHECK_LD(ctx, who, ldy, c);
  return SMN_OK;
}

// the Gram stage of both entries: arguments already checked; G_d [m, ldg], B_d [m, c], s_d [c] in fp64
int gram_run(smn_ctx* ctx, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl, const double* w_d, const void* y_d,
             int64_t c, int64_t ldy, double* G_d, int64_t ldg, double* B_d, double* s_d) {
  const int64_t splits = (n + kSplit - 1) / kSplit;
  return by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    constexpr int BT = GramCfg<T>::BT;
    const int64_t tiles = (m + BT - 1) / BT;
    const int npairs = (int)(tiles * (tiles + 1) / 2);
    const size_t g_bytes = al256(sizeof(T) * (size_t)splits * (size_t)npairs * (size_t)(BT * BT));
    const size_t b_bytes = al256(sizeof(double) * (size_t)splits * (size_t)m * (size_t)c);
    const size_t s_bytes = al256(sizeof(double) * (size_t)splits * (size_t)c);
    void* base = nullptr;
    SMN_TRY(smn_workspace(ctx, 4, g_bytes + b_bytes + s_bytes, &base));
    T* part = static_cast<T*>(base);
    double* part_b = reinterpret_cast<double*>(static_cast<char*>(base) + g_bytes);
    double* part_s = reinterpret_cast<double*>(static_cast<char*>(base) + g_bytes + b_bytes);
    const T* L = static_cast<const T*>(L_d);
    const int64_t total = splits * npairs;
    if (total > (int64_t)INT_MAX - 8) return smn_fail(ctx, SMN_ENOTSUP, "smn_lowrank_gram: n = %lld, m = %lld is too large", (long long)n, (long long)m);
    hipLaunchKernelGGL(lowrank_gram_kernel<T>, dim3((unsigned)round_up(total, 8)), dim3(256), 0, ctx->stream, L, n, (int)m, ldl,
                       aligned16(L_d, ldl, sizeof(T)) ? 1 : 0, w_d, part, npairs, total);
    SMN_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(lowrank_gram_reduce_kernel<T>, dim3(BT * BT / 256, (unsigned)npairs), dim3(256), 0, ctx->stream, part, splits,
                       npairs, (int)m, G_d, ldg);
    SMN_CHECK_LAUNCH(ctx);
    if (c > 0) {
      hipLaunchKernelGGL(lowrank_by_kernel<T>, dim3((unsigned)splits, (unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, L, n,
                         (int)m, ldl, w_d, static_cast<const T*>(y_d), (int)c, ldy, part_b, part_s);
      SMN_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(lowrank_sum_splits_kernel, dim3((unsigned)((m * c + 255) / 256)), dim3(256), 0, ctx->stream, part_b, splits,
                         m * c, B_d);
      SMN_CHECK_LAUNCH(ctx);
      hipLaunchKernelGGL(lowrank_sum_splits_kernel, dim3(1), dim3(256), 0, ctx->stream, part_s, splits, c, s_d);
      SMN_CHECK_LAUNCH(ctx);
    }
    return (int)SMN_OK;
  });
}

}  // namespace

extern "C" int smn_lowrank_gram(smn_ctx* ctx, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl, const double* w_d,
                                const void* y_d, int64_t c, int64_t ldy, double* G_d, int64_t ldg, double* B_d, double* s_d) {
  if (!ctx) return SMN_EINVAL;
  SMN_TRY(check_factor(ctx, "smn_lowrank_gram", dtype, L_d, n, m, ldl));
  SMN_TRY(check_targets(ctx, "smn_lowrank_gram", y_d, c, 0, ldy));
  if (!G_d || (c > 0 && (!B_d || !s_d))) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_gram: NULL pointer");
  SMN_CHECK_LD(ctx, "smn_lowrank_gram", ldg, m);
  SMN_ENTER(ctx);
  return gram_run(ctx, dtype, L_d, n, m, ldl, w_d, y_d, c, ldy, G_d, ldg, B_d, s_d);
}

extern "C" int smn_lowrank_fit(smn_ctx* ctx, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl, const double* resid_d,
                               double lambda, int fitc, const void* y_d, int64_t c, int64_t ldy, double* C_d, double* beta_d,
                               double* quad_h, double* logdet_h, int* info_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_TRY(check_factor(ctx, "smn_lowrank_fit", dtype, L_d, n, m, ldl));
  SMN_TRY(check_targets(ctx, "smn_lowrank_fit", y_d, c, 1, ldy));
  if (!C_d || !beta_d || !quad_h || !logdet_h || !info_h) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_fit: NULL pointer");
  if (!(lambda > 0.0) || !std::isfinite(lambda)) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_fit: lambda = %g is not a positive number", lambda);
  if (fitc != 0 && fitc != 1) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_fit: fitc = %d is neither 0 nor 1", fitc);
  SMN_ENTER(ctx);
  // slot 5: the weights, [A B; B^T 0], B, s and the results {quad[c], sum log d}
  const int64_t lda = m + c;
  const size_t w_bytes = al256(sizeof(double) * (size_t)n), a_bytes = al256(sizeof(double) * (size_t)lda * (size_t)lda);
  const size_t b_bytes = al256(sizeof(double) * (size_t)m * (size_t)c), s_bytes = al256(sizeof(double) * (size_t)c);
  void* base = nullptr;
  SMN_TRY(smn_workspace(ctx, 5, w_bytes + a_bytes + b_bytes + 2 * s_bytes + 256, &base));
  char* p = static_cast<char*>(base);
  double* w = reinterpret_cast<double*>(p); p += w_bytes;
  double* aug = reinterpret_cast<double*>(p); p += a_bytes;
  double* B = reinterpret_cast<double*>(p); p += b_bytes;
  double* s = reinterpret_cast<double*>(p); p += s_bytes;
  double* res = reinterpret_cast<double*>(p);
  hipLaunchKernelGGL(lowrank_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, resid_d, n, lambda, fitc, w);
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(lowrank_logd_kernel, dim3(1), dim3(256), 0, ctx->stream, resid_d, n, lambda, fitc, res + c);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(gram_run(ctx, dtype, L_d, n, m, ldl, w, y_d, c, ldy, aug, lda, B, s));
  hipLaunchKernelGGL(lowrank_aug_kernel, dim3((unsigned)((c * lda + m + 255) / 256)), dim3(256), 0, ctx->stream, aug, lda, (int)m,
                     (int)c, B);
  SMN_CHECK_LAUNCH(ctx);
  int info = 0;
  double logdet_a = 0.0;
  SMN_TRY(smn_cholesky(ctx, SMN_F64, aug, lda, m, lda, 0, 0.0, 0.0, &info, &logdet_a));
  const int64_t cells = m * m + m * c + c;
  hipLaunchKernelGGL(lowrank_unpack_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, aug, lda, (int)m, (int)c,
                     s, info != 0 ? 1 : 0, C_d, beta_d, res);
  SMN_CHECK_LAUNCH(ctx);
  if (info == 0) SMN_TRY(smn_trsm(ctx, SMN_F64, C_d, m, m, beta_d, c, c, 1));   // beta = C^-T (C^-1 B)
  std::vector<double> h((size_t)c + 1);
  SMN_HIP(ctx, hipMemcpyAsync(h.data(), res, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t k = 0; k < c; ++k) quad_h[k] = h[(size_t)k];
  *logdet_h = info != 0 ? std::nan("") : logdet_a + h[(size_t)c];
  *info_h = info;
  return SMN_OK;
}

extern "C" int smn_lowrank_readout(smn_ctx* ctx, int dtype, const void* kzt_d, int64_t ldk, const void* ktt_d, int64_t t, int64_t m,
                                   const double* R_d, int64_t ldr, const double* C_d, const double* beta_d, int64_t c, void* mean_d,
                                   void* var_d) {
  if (!ctx) return SMN_EINVAL;
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_readout: bad dtype %d", dtype);
  if (!kzt_d || !ktt_d || !R_d || !C_d || !beta_d || !mean_d || !var_d) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_readout: NULL pointer");
  if (t <= 0 || m <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_lowrank_readout: t = %lld, m = %lld", (long long)t, (long long)m);
  if (m > SMN_LOWRANK_MAX_RANK)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_lowrank_readout: m = %lld is above SMN_LOWRANK_MAX_RANK = %d", (long long)m, SMN_LOWRANK_MAX_RANK);
  if (c < 1 || c > 48) return smn_fail(ctx, c > 48 ? SMN_ENOTSUP : SMN_EINVAL, "smn_lowrank_readout: c = %lld outside [1, 48]", (long long)c);
  SMN_CHECK_LD(ctx, "smn_lowrank_readout", ldk, t);
  SMN_CHECK_LD(ctx, "smn_lowrank_readout", ldr, m);
  const int64_t groups = (t + kReadoutCols - 1) / kReadoutCols;
  if (groups > (int64_t)INT_MAX) return smn_fail(ctx, SMN_ENOTSUP, "smn_lowrank_readout: t = %lld is too large", (long long)t);
  SMN_ENTER(ctx);
  const size_t lds = sizeof(double) * (size_t)kReadoutCols * (size_t)m;
  return by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(lowrank_readout_kernel<T>), lds));
    hipLaunchKernelGGL(lowrank_readout_kernel<T>, dim3((unsigned)groups), dim3(64), lds, ctx->stream, static_cast<const T*>(kzt_d), ldk,
                       static_cast<const T*>(ktt_d), t, (int)m, R_d, ldr, C_d, beta_d, (int)c, static_cast<T*>(mean_d),
                       static_cast<T*>(var_d));
    SMN_CHECK_LAUNCH(ctx);
    return (int)SMN_OK;
  });
}
