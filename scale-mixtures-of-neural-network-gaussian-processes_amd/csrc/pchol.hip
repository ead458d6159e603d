// pchol.hip — partial Cholesky factorisation with greedy (largest residual variance) pivoting: K ~ L L^T from the kernel's
// diagonal and M of its rows, without the N x N matrix.
//
// State: L [n, ldl] in the storage type T (column j written at step j) and resid [n] in fp64, r_i = K_ii - sum_t L_it^2.
// One step with pivot p and its kernel row k = K(x_p, X):
//     l_i = (k_i - sum_{t<j} L_it L_pt) / sqrt(r_p),   L_ij = l_i (rounded to T),   r_i <- r_i - L_ij^2
// The pivot's own row gets L_pj = sqrt(r_p) and r_p = 0; a row whose residual is exactly 0 (an earlier pivot, a zero diagonal)
// gets L_ij = 0 and keeps r_i = 0, so it can never be picked (again).  The next pivot is argmax r_i, ties to the lowest index;
// the remaining trace is sum_i max(r_i, 0).
//
// Two forms share one step kernel:
//   matrix form (smn_pchol_begin / smn_pchol_step): the host hands in each row k, from any kernel function;
//   fused form  (smn_pchol_mlp): the MLP / dense-ResNet NNGP row is made in the kernel -- K0 = x_i . x_p / d as a GEMV that
//     streams X once per step, carried through the layer stack by the scalar rules of layer_prog.hpp -- and the whole loop is
//     queued without a host round trip: pivot, residual and trace of every step stay in device memory.
//
// The step kernel (memory bound: X once, the first j columns of L once):
//   one workgroup = 4 waves = 16 rows, 4 rows per wave with their loads interleaved; x_p and L_p are staged in LDS in tiles of
//   2048 elements, once per workgroup; rows are read with 16-byte loads where the base and the leading dimension allow it and
//   element by element otherwise, in the SAME element-to-lane assignment, so the bits do not depend on the alignment.
//   Every product and sum is fp64 (a product of two f32 is exact there): lane l adds its elements in ascending order, the 64
//   lane sums are reduced by a butterfly.  The layer map runs in fp64 for both storage types -- it is one element per row and
//   step, nothing beside the stream -- with fp64 per-row variance tables made once per call.
//   Each workgroup leaves (max r, lowest index, sum max(r, 0)) of its 16 rows, taken in row order; a second, single-workgroup
//   kernel reduces these partials in a fixed order (thread t takes partials t, t + 256, ...; then a tree) and writes pivot
//   j + 1, its residual and the trace where the next step reads them.  No floating-point atomics: two calls give the same
//   bits, and since a partial is always 16 rows the bits do not depend on the grid either.
//
// Prescribed pivots (smn_pchol_mlp_at; the matrix form's host loop simply hands smn_pchol_step the given pivot): the same step
// kernel is queued; the finish kernel between two steps writes piv[j] = given[j] and rmax[j] = resid[given[j]] in place of the
// arg-max -- behind step j - 1 and in front of step j, so the pivot's residual is read before its own workgroup overwrites it.
// The step kernel therefore sees the (p, r_p) it saw in the greedy run that chose these pivots, and leaves that run's bits.
//
// Rank: the loop stops before step j when trace_j <= tol_rel trace_0 or when the largest residual is not above
// 4 (j + 1) eps_T max_i K_ii, eps_T the unit roundoff of the storage type: the size of the rounding error of a residual that was
// computed from j columns stored in T (the gamma_{j+1} bound of a Cholesky's Schur complement), with a factor 4 of room.  Below
// it a residual is noise of the L it was computed from -- the residual of an exact duplicate of a pivot comes out as a few
// eps_T K_ii of either sign, never as 0 -- and its square root would scale a column of noise.  The floor grows with the columns
// made, not with n: a healthy matrix of any size runs to max_rank.  The decision is made on the device; steps queued behind it
// write zeros into their column and touch nothing else.
#include <cfloat>
#include <cmath>
#include <vector>

#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

constexpr int kRowsPerWave = 4;
constexpr int kRowsPerWg = 16;      // the unit of the partials: fixed, so the reduction order does not depend on a launch shape
constexpr int kTileElems = 2048;    // elements of x_p / L_p staged per LDS tile (8 KB f32, 16 KB f64)

struct PcholCtl {
  double dmax;      // max_i K_ii (set with the first pivot): a residual at or below 4 (j + 1) eps_T dmax is rounding noise
  double tol_rel;
  int stop;         // -1 while the loop runs; else the number of columns made when it stopped
  int max_rank;     // 0: no stop decision (matrix form: the host decides)
};

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; static constexpr int V = 4; };
template <> struct Vec16<double> { using type = double2; static constexpr int V = 2; };

template <typename T>
__device__ __forceinline__ void load_elems(const T* __restrict__ row, int64_t c, int64_t len, bool vec_ok, T (&a)[Vec16<T>::V]) {
  constexpr int V = Vec16<T>::V;
  if (vec_ok && c + V <= len) {
    const typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(row + c);
    if constexpr (V == 4) {
      a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else {
      a[0] = v.x; a[1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) a[k] = c + k < len ? row[c + k] : T(0);
  }
}

// sh[0, round_up(tl, V)) <- src[c0, c0 + tl), zero behind tl
template <typename T>
__device__ __forceinline__ void stage_tile(const T* __restrict__ src, int64_t c0, int tl, T* sh) {
  constexpr int V = Vec16<T>::V;
  const int fill = (tl + V - 1) / V * V;
  for (int c = threadIdx.x; c < fill; c += 256) sh[c] = c < tl ? src[c0 + c] : T(0);
}

// acc[r] += sum_{c < tl} rows[r][c0 + c] * sh[c]; lane l takes the elements [V (l + 64 m), V (l + 64 m) + V), m = 0, 1, ...
template <typename T>
__device__ __forceinline__ void dot_tile(const T* const (&rows)[kRowsPerWave], const T* sh, int64_t c0, int tl, int64_t len,
                                         bool vec_ok, int lane, double (&acc)[kRowsPerWave]) {
  constexpr int V = Vec16<T>::V;
  for (int c = lane * V; c < tl; c += 64 * V) {
    T b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) b[k] = sh[c + k];
    T a[kRowsPerWave][V];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) load_elems<T>(rows[r], c0 + c, len, vec_ok, a[r]);
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r)
#pragma unroll
      for (int k = 0; k < V; ++k) acc[r] = fma((double)a[r][k], (double)b[k], acc[r]);
  }
}

// acc[r] = rows[r][0, len) . vec[0, len) for the wave's 4 rows; vec is staged through sh by the whole workgroup (every wave of
// it must call this with the same vec and len).
template <typename T>
__device__ __forceinline__ void dot_rows(const T* const (&rows)[kRowsPerWave], const T* __restrict__ vec, int64_t len, bool vec_ok,
                                         T* sh, int lane, double (&acc)[kRowsPerWave]) {
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) acc[r] = 0.0;
  for (int64_t c0 = 0; c0 < len; c0 += kTileElems) {
    const int tl = (int)(len - c0 < kTileElems ? len - c0 : kTileElems);
    __syncthreads();   // the readers of the tile before this one are done
    stage_tile<T>(vec, c0, tl, sh);
    __syncthreads();
    dot_tile<T>(rows, sh, c0, tl, len, vec_ok, lane, acc);
  }
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
}

template <typename T>
struct StepArgs {
  const T* x; int64_t n, ldx, d; double inv_d; int x_vec;   // fused form
  const double* tab; LayerProg prog;                       // fused form: [2 nsets][n] per-row (r, s), fp64
  const T* krow; int64_t pivot; double rp;                 // matrix form: the row, the pivot and its residual from the host
  T* L; int64_t ldl; int l_vec; int j;
  double* resid;
  const PcholCtl* ctl; const int64_t* piv; const double* rmax;   // fused form: piv[j], rmax[j] as the finish kernel left them
  double* pmax; double* psum; int64_t* pidx;               // [ceil(n / 16)]
};

template <typename T, int NET, int ACT, bool FUSED>
__global__ void __launch_bounds__(256) pchol_step_kernel(StepArgs<T> a) {
  __shared__ __align__(16) T sh[kTileElems];
  __shared__ double sh_r[kRowsPerWg];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wg0 = (int64_t)blockIdx.x * kRowsPerWg;
  int64_t p = a.pivot;
  double rp = a.rp;
  if (FUSED) {
    if (a.ctl->stop >= 0) {   // the loop has stopped: this column is zero, nothing else moves
      const int64_t i = wg0 + threadIdx.x;
      if (threadIdx.x < kRowsPerWg && i < a.n) a.L[i * a.ldl + a.j] = T(0);
      return;
    }
    p = a.piv[a.j];
    rp = a.rmax[a.j];
  }
  const int64_t row0 = wg0 + wave * kRowsPerWave;
  int64_t ri[kRowsPerWave];
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) ri[r] = row0 + r < a.n ? row0 + r : a.n - 1;   // (a row past the end repeats the last one; its result is dropped)

  double k0[kRowsPerWave] = {0.0, 0.0, 0.0, 0.0}, dot[kRowsPerWave] = {0.0, 0.0, 0.0, 0.0};
  if (FUSED) {
    const T* rows[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) rows[r] = a.x + ri[r] * a.ldx;
    dot_rows<T>(rows, a.x + p * a.ldx, a.d, a.x_vec != 0, sh, lane, k0);
  }
  if (a.j > 0) {
    const T* rows[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) rows[r] = a.L + ri[r] * a.ldl;
    dot_rows<T>(rows, a.L + p * a.ldl, a.j, a.l_vec != 0, sh, lane, dot);
  }

  // lane r < 4 finishes row r of the wave (every lane computes the row lane & 3: no divergence in the map)
  const int rsel = lane & 3;
  double kv = k0[0], dv = dot[0];
  int64_t i = ri[0];
#pragma unroll
  for (int r = 1; r < kRowsPerWave; ++r)
    if (rsel == r) {
      kv = k0[r]; dv = dot[r]; i = ri[r];
    }
  double k;
  if constexpr (FUSED) {
    k = kv * a.inv_d;
    double th = 0.0;
    const ElemProg<double, NET, ACT, false> prog(a.prog);
    prog.pre(k, th);
    for (int s = 0; s < a.prog.nsets; ++s) {
      const double* t0 = a.tab + (int64_t)(2 * s) * a.n;
      const double* t1 = t0 + a.n;
      prog.step(s, k, th, t0[i] * t0[p], t1[i] * t1[p]);
    }
    prog.post(k, th, 0.0);
  } else {
    k = (double)a.krow[i];
  }
  const bool mine = lane < kRowsPerWave && row0 + lane < a.n;
  double r_new = 0.0;
  if (mine) {
    const double r_old = a.resid[i];
    T lt;
    if (i == p) {
      lt = (T)sqrt(rp);
      r_new = 0.0;
    } else if (r_old == 0.0) {
      lt = T(0);
      r_new = 0.0;
    } else {
      lt = (T)((k - dv) / sqrt(rp));
      r_new = r_old - (double)lt * (double)lt;
    }
    a.L[i * a.ldl + a.j] = lt;
    a.resid[i] = r_new;
  }
  if (lane < kRowsPerWave) sh_r[wave * kRowsPerWave + lane] = r_new;
  __syncthreads();
  if (threadIdx.x == 0) {
    double best = sh_r[0], sum = fmax(sh_r[0], 0.0);
    int64_t bi = wg0;
    for (int q = 1; q < kRowsPerWg && wg0 + q < a.n; ++q) {
      const double v = sh_r[q];
      if (v > best) {
        best = v; bi = wg0 + q;
      }
      sum += fmax(v, 0.0);
    }
    a.pmax[blockIdx.x] = best; a.pidx[blockIdx.x] = bi; a.psum[blockIdx.x] = sum;
  }
}

// the partials of resid as it stands (the start of a factorisation): one thread per 16 rows, in row order
__global__ void pchol_partial_kernel(const double* __restrict__ resid, int64_t n, double* __restrict__ pmax,
                                     double* __restrict__ psum, int64_t* __restrict__ pidx) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i0 = g * kRowsPerWg;
  if (i0 >= n) return;
  double best = resid[i0], sum = fmax(resid[i0], 0.0);
  int64_t bi = i0;
  for (int q = 1; q < kRowsPerWg && i0 + q < n; ++q) {
    const double v = resid[i0 + q];
    if (v > best) {
      best = v; bi = i0 + q;
    }
    sum += fmax(v, 0.0);
  }
  pmax[g] = best; pidx[g] = bi; psum[g] = sum;
}

// One workgroup: (max, lowest index of it, sum) over the P partials in a fixed order -> trace[jn], rmax[jn], piv[jn], and the
// stop decision for step jn.
__global__ void __launch_bounds__(256) pchol_finish_kernel(const double* __restrict__ pmax, const double* __restrict__ psum,
                                                           const int64_t* __restrict__ pidx, int64_t P, int jn, PcholCtl* ctl,
                                                           double* __restrict__ trace, double* __restrict__ rmax,
                                                           int64_t* __restrict__ piv, double floor_scale,
                                                           const int64_t* __restrict__ fixed, int nfixed,
                                                           const double* __restrict__ resid) {
  __shared__ double sm[256], ss[256];
  __shared__ int64_t si[256];
  if (ctl->stop >= 0) return;
  const int t = threadIdx.x;
  double best = -INFINITY, sum = 0.0;
  int64_t bi = INT64_MAX;
  for (int64_t g = t; g < P; g += 256) {
    const double v = pmax[g];
    if (v > best) {   // (g ascending and a partial's index is the lowest of its maxima: the first hit is the lowest index)
      best = v; bi = pidx[g];
    }
    sum += psum[g];
  }
  sm[t] = best; si[t] = bi; ss[t] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      if (sm[t + o] > sm[t] || (sm[t + o] == sm[t] && si[t + o] < si[t])) {
        sm[t] = sm[t + o]; si[t] = si[t + o];
      }
      ss[t] += ss[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    // prescribed pivots (smn_pchol_mlp_at): step jn is taken at fixed[jn], whose residual is read here -- behind step jn - 1 and
    // in front of step jn, whose own workgroup overwrites it; the floor and the trace are those of the greedy loop
    const bool given = fixed != nullptr && jn < nfixed;
    const int64_t pj = given ? fixed[jn] : si[0];
    const double rj = given ? resid[pj] : sm[0];
    trace[jn] = ss[0]; rmax[jn] = rj; piv[jn] = pj;
    if (jn == 0) ctl->dmax = fmax(sm[0], 0.0);
    const double floor = floor_scale * (double)(jn + 1) * ctl->dmax;
    if (jn < ctl->max_rank && (!(rj > floor) || ss[0] <= ctl->tol_rel * trace[0])) ctl->stop = jn;
  }
}

template <typename T>
__global__ void pchol_resid_from_diag_kernel(const T* __restrict__ diag, int64_t n, double* __restrict__ resid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) resid[i] = (double)diag[i];
}

// q_i = |x_i|^2 / d, one wave per row, summed as the build's padding pass sums it (pad_rows_kernel): lane l takes the elements
// l, l + 64, ... in fp64, then the butterfly.
template <typename T>
__global__ void __launch_bounds__(256) pchol_q_kernel(const T* __restrict__ x, int64_t n, int64_t ldx, int64_t d, double inv_d,
                                                      double* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const T* xr = x + row * ldx;
  double s = 0.0;
  for (int64_t c = lane; c < d; c += 64) {
    const T v = xr[c];
    s += (double)v * (double)v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) q[row] = s * inv_d;
}

// The build's exact-diagonal rule (diag_tables_kernel of kernel_build.hip, its generic form) in fp64: tab[(2 set) n + i] = r,
// tab[(2 set + 1) n + i] = s, and resid[i] = K(x_i, x_i) in closed form.
__global__ void pchol_tables_kernel(const double* __restrict__ q0, int64_t n, LayerProg p, double* __restrict__ tab,
                                    double* __restrict__ resid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double q = q0[i];
  if (p.net == NET_RESNET) q = p.w2 * q + p.b2;
  for (int s = 0; s < p.nsets; ++s) {
    const double qt = (p.net == NET_MLP) ? p.w2 * q + p.b2 : q;   // pre-activation variance
    double r, sv, qa;
    if (p.act == ACT_RELU) {
      r = qt > 0.0 ? 1.0 / sqrt(qt) : 0.0;
      sv = sqrt(qt / (2.0 * nngp::kPi));
      qa = 0.5 * qt;
    } else {
      r = 1.0 / sqrt(1.0 + 2.0 * qt);
      sv = 0.0;
      qa = (2.0 / nngp::kPi) * asin(2.0 * qt / (1.0 + 2.0 * qt));
    }
    tab[(int64_t)(2 * s) * n + i] = r;
    tab[(int64_t)(2 * s + 1) * n + i] = sv;
    if (p.net == NET_MLP || s == p.nsets - 1) q = qa;
    else q += p.w2 * qa + p.b2;
  }
  resid[i] = q * p.lw2;
}

// ------------------------------------------------------------------ host side
struct PcholWs {
  PcholCtl* ctl; double* trace; double* rmax; int64_t* piv; double* pmax; double* psum; int64_t* pidx; double* q; double* tab;
  int64_t* fixed;   // prescribed pivots [max_rank + 1] (smn_pchol_mlp_at), else nullptr
  int64_t P;
};

int pchol_ws(smn_ctx* ctx, int64_t n, int64_t max_rank, int nsets, bool fused, PcholWs* w, bool fixed = false) {
  const int64_t P = (n + kRowsPerWg - 1) / kRowsPerWg;
  const size_t m1 = (size_t)max_rank + 1;
  size_t words = 8 + 3 * m1 + 3 * (size_t)P;           // 8-byte words: ctl (padded to 64 bytes), trace, rmax, piv, the partials
  if (fused) words += (size_t)n * (size_t)(1 + 2 * nsets);
  if (fixed) words += m1;
  void* base = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, 8 * words, &base));
  double* b = static_cast<double*>(base);
  w->ctl = reinterpret_cast<PcholCtl*>(b); b += 8;
  w->trace = b; b += m1;
  w->rmax = b; b += m1;
  w->piv = reinterpret_cast<int64_t*>(b); b += m1;
  w->pmax = b; b += P;
  w->psum = b; b += P;
  w->pidx = reinterpret_cast<int64_t*>(b); b += P;
  w->q = fused ? b : nullptr;
  w->tab = fused ? b + n : nullptr;
  if (fused) b += (size_t)n * (size_t)(1 + 2 * nsets);
  w->fixed = fixed ? reinterpret_cast<int64_t*>(b) : nullptr;
  w->P = P;
  return SMN_OK;
}

bool aligned16(const void* p, int64_t ld, size_t es) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * (int64_t)es) % 16 == 0; }

double unit_roundoff(int dtype) { return dtype == SMN_F64 ? DBL_EPSILON : (double)FLT_EPSILON; }

int launch_finish(smn_ctx* ctx, const PcholWs& w, int jn, double floor_scale, int nfixed = 0, const double* resid = nullptr) {
  hipLaunchKernelGGL(pchol_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, w.pmax, w.psum, w.pidx, w.P, jn, w.ctl, w.trace,
                     w.rmax, w.piv, floor_scale, static_cast<const int64_t*>(nfixed > 0 ? w.fixed : nullptr), nfixed, resid);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

template <typename T, int NET, int ACT, bool FUSED>
int launch_step_t(smn_ctx* ctx, const StepArgs<T>& a, int64_t P) {
  hipLaunchKernelGGL((pchol_step_kernel<T, NET, ACT, FUSED>), dim3((unsigned)P), dim3(256), 0, ctx->stream, a);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

template <typename T>
int launch_step_fused(smn_ctx* ctx, const StepArgs<T>& a, int64_t P) {
  const int net = a.prog.net, act = a.prog.act;
  if (net == NET_MLP && act == ACT_RELU) return launch_step_t<T, NET_MLP, ACT_RELU, true>(ctx, a, P);
  if (net == NET_MLP && act == ACT_ERF) return launch_step_t<T, NET_MLP, ACT_ERF, true>(ctx, a, P);
  if (net == NET_RESNET && act == ACT_RELU) return launch_step_t<T, NET_RESNET, ACT_RELU, true>(ctx, a, P);
  if (net == NET_RESNET && act == ACT_ERF) return launch_step_t<T, NET_RESNET, ACT_ERF, true>(ctx, a, P);
  return smn_fail(ctx, SMN_EINVAL, "smn_pchol_mlp: bad net/act");
}

int check_pchol(smn_ctx* ctx, const char* who, int dtype, int64_t n) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (n <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: n = %lld", who, (long long)n);
  if ((n + kRowsPerWg - 1) / kRowsPerWg > (int64_t)INT_MAX) return smn_fail(ctx, SMN_ENOTSUP, "%s: n = %lld is too large", who, (long long)n);
  return SMN_OK;
}

// (pivot, rmax, trace) of slot jn, after everything queued so far
int read_back(smn_ctx* ctx, const PcholWs& w, int jn, int64_t* pivot, double* rmax, double* trace) {
  SMN_HIP(ctx, hipMemcpyAsync(pivot, w.piv + jn, 8, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipMemcpyAsync(rmax, w.rmax + jn, 8, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipMemcpyAsync(trace, w.trace + jn, 8, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}

__global__ void pchol_init_kernel(PcholCtl* ctl, int max_rank, double tol_rel) {
  ctl->dmax = 0.0; ctl->tol_rel = tol_rel; ctl->stop = -1; ctl->max_rank = max_rank;
}

int init_ctl(smn_ctx* ctx, const PcholWs& w, int max_rank, double tol_rel) {   // (a launch, not a copy: no synchronisation)
  hipLaunchKernelGGL(pchol_init_kernel, dim3(1), dim3(1), 0, ctx->stream, w.ctl, max_rank, tol_rel);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

}  // namespace

extern "C" int smn_pchol_begin(smn_ctx* ctx, int dtype, int64_t n, const void* diag_d, double* resid_d, int64_t* pivot_h,
                               double* rmax_h, double* trace_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_TRY(check_pchol(ctx, "smn_pchol_begin", dtype, n));
  if (!diag_d || !resid_d || !pivot_h || !rmax_h || !trace_h) return smn_fail(ctx, SMN_EINVAL, "smn_pchol_begin: NULL pointer");
  SMN_ENTER(ctx);
  PcholWs w;
  SMN_TRY(pchol_ws(ctx, n, 0, 0, false, &w));
  SMN_TRY(init_ctl(ctx, w, 0, 0.0));
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(pchol_resid_from_diag_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       static_cast<const T*>(diag_d), n, resid_d);
  });
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(pchol_partial_kernel, dim3((unsigned)((w.P + 255) / 256)), dim3(256), 0, ctx->stream, resid_d, n, w.pmax,
                     w.psum, w.pidx);
  SMN_CHECK_LAUNCH(ctx);
  SMN_TRY(launch_finish(ctx, w, 0, 0.0));
  return read_back(ctx, w, 0, pivot_h, rmax_h, trace_h);
}

extern "C" int smn_pchol_step(smn_ctx* ctx, int dtype, int64_t n, int64_t j, int64_t pivot, const void* krow_d, void* L_d,
                              int64_t ldl, double* resid_d, int64_t* next_pivot_h, double* rmax_h, double* trace_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_TRY(check_pchol(ctx, "smn_pchol_step", dtype, n));
  if (!krow_d || !L_d || !resid_d || !next_pivot_h || !rmax_h || !trace_h)
    return smn_fail(ctx, SMN_EINVAL, "smn_pchol_step: NULL pointer");
  if (j < 0 || j >= ldl || j >= n || j >= (int64_t)INT_MAX)
    return smn_fail(ctx, SMN_EINVAL, "smn_pchol_step: step j = %lld outside [0, min(ldl = %lld, n = %lld))", (long long)j,
                    (long long)ldl, (long long)n);
  SMN_CHECK_LD(ctx, "smn_pchol_step", ldl, j + 1);
  if (pivot < 0 || pivot >= n) return smn_fail(ctx, SMN_EINVAL, "smn_pchol_step: pivot %lld outside [0, %lld)", (long long)pivot, (long long)n);
  SMN_ENTER(ctx);
  double rp = 0.0;
  SMN_HIP(ctx, hipMemcpyAsync(&rp, resid_d + pivot, 8, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!(rp > 0.0))
    return smn_fail(ctx, SMN_EINVAL, "smn_pchol_step: the residual of pivot %lld is %g, not > 0 (the state is untouched)", (long long)pivot, rp);
  PcholWs w;
  SMN_TRY(pchol_ws(ctx, n, 0, 0, false, &w));
  SMN_TRY(init_ctl(ctx, w, 0, 0.0));
  SMN_TRY(by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    StepArgs<T> a{};
    a.n = n; a.krow = static_cast<const T*>(krow_d); a.pivot = pivot; a.rp = rp;
    a.L = static_cast<T*>(L_d); a.ldl = ldl; a.l_vec = aligned16(L_d, ldl, sizeof(T)) ? 1 : 0; a.j = (int)j;
    a.resid = resid_d; a.ctl = w.ctl; a.piv = w.piv; a.rmax = w.rmax;
    a.pmax = w.pmax; a.psum = w.psum; a.pidx = w.pidx;
    return launch_step_t<T, NET_NONE, ACT_RELU, false>(ctx, a, w.P);
  }));
  SMN_TRY(launch_finish(ctx, w, 0, 0.0));
  return read_back(ctx, w, 0, next_pivot_h, rmax_h, trace_h);
}

namespace {

// The fused loop behind smn_pchol_mlp (given_h == nullptr: greedy, the pivots come back in pivots_h) and smn_pchol_mlp_at
// (given_h [max_rank]: step j is taken at given_h[j]).
int pchol_mlp_run(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                  double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, int64_t max_rank, double tol_rel,
                  void* L_d, int64_t ldl, double* resid_d, int64_t* pivots_h, const int64_t* given_h, double* trace_h,
                  int64_t* rank_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_TRY(check_pchol(ctx, who, dtype, n));
  if (!x_d || !L_d || !resid_d || (!pivots_h && !given_h) || !trace_h || !rank_h) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (d <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: d = %lld", who, (long long)d);
  if (max_rank < 1 || max_rank > n || max_rank >= (int64_t)INT_MAX)
    return smn_fail(ctx, SMN_EINVAL, "%s: max_rank = %lld outside [1, n = %lld]", who, (long long)max_rank, (long long)n);
  if (!(tol_rel >= 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: tol_rel = %g is negative", who, tol_rel);
  SMN_CHECK_LD(ctx, who, ldx, d);
  SMN_CHECK_LD(ctx, who, ldl, max_rank);
  if (given_h)
    for (int64_t t = 0; t < max_rank; ++t)
      if (given_h[t] < 0 || given_h[t] >= n)
        return smn_fail(ctx, SMN_EINVAL, "%s: pivots_h[%lld] = %lld outside [0, n = %lld)", who, (long long)t, (long long)given_h[t], (long long)n);
  SMN_TRY(no_ntk_net(ctx, who, net));
  if (net != SMN_NET_MLP && net != SMN_NET_DENSE_RESNET) return smn_fail(ctx, SMN_EINVAL, "%s: unknown net %d", who, net);
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "%s: Unsupported act %d", who, act);
  if (num_hiddens < 0) return smn_fail(ctx, SMN_EINVAL, "%s: num_hiddens < 0", who);
  LayerProg prog;
  prog.net = net; prog.act = act; prog.fast = 0;
  prog.nsets = net == SMN_NET_MLP ? num_hiddens : num_hiddens + 1;
  if (prog.nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "%s: num_hiddens too large (max %d activation layers)", who, kMaxSets);
  prog.w2 = w_std * w_std; prog.b2 = b_std * b_std; prog.lw2 = last_w_std * last_w_std;
  SMN_ENTER(ctx);
  PcholWs w;
  SMN_TRY(pchol_ws(ctx, n, max_rank, prog.nsets, true, &w, given_h != nullptr));
  const int nfixed = given_h ? (int)max_rank : 0;
  if (given_h) SMN_HIP(ctx, hipMemcpyAsync(w.fixed, given_h, 8 * (size_t)max_rank, hipMemcpyHostToDevice, ctx->stream));
  SMN_TRY(init_ctl(ctx, w, (int)max_rank, tol_rel));
  const double inv_d = 1.0 / (double)d;
  const double floor_scale = 4.0 * unit_roundoff(dtype);
  SMN_TRY(by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(pchol_q_kernel<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, static_cast<const T*>(x_d), n,
                       ldx, d, inv_d, w.q);
    SMN_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(pchol_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, w.q, n, prog, w.tab,
                       resid_d);
    SMN_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(pchol_partial_kernel, dim3((unsigned)((w.P + 255) / 256)), dim3(256), 0, ctx->stream, resid_d, n, w.pmax,
                       w.psum, w.pidx);
    SMN_CHECK_LAUNCH(ctx);
    SMN_TRY(launch_finish(ctx, w, 0, floor_scale, nfixed, resid_d));
    StepArgs<T> a{};
    a.x = static_cast<const T*>(x_d); a.n = n; a.ldx = ldx; a.d = d; a.inv_d = inv_d;
    a.x_vec = aligned16(x_d, ldx, sizeof(T)) ? 1 : 0;
    a.tab = w.tab; a.prog = prog;
    a.L = static_cast<T*>(L_d); a.ldl = ldl; a.l_vec = aligned16(L_d, ldl, sizeof(T)) ? 1 : 0;
    a.resid = resid_d; a.ctl = w.ctl; a.piv = w.piv; a.rmax = w.rmax;
    a.pmax = w.pmax; a.psum = w.psum; a.pidx = w.pidx;
    for (int64_t j = 0; j < max_rank; ++j) {
      a.j = (int)j;
      SMN_TRY(launch_step_fused<T>(ctx, a, w.P));
      SMN_TRY(launch_finish(ctx, w, (int)j + 1, floor_scale, nfixed, resid_d));
    }
    return (int)SMN_OK;
  }));
  PcholCtl h;
  std::vector<double> tr((size_t)max_rank + 1);
  std::vector<int64_t> pv((size_t)max_rank + 1);
  SMN_HIP(ctx, hipMemcpyAsync(&h, w.ctl, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipMemcpyAsync(tr.data(), w.trace, 8 * tr.size(), hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipMemcpyAsync(pv.data(), w.piv, 8 * pv.size(), hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int64_t rank = h.stop >= 0 ? h.stop : max_rank;
  for (int64_t t = 0; pivots_h && t < rank; ++t) pivots_h[t] = pv[(size_t)t];
  for (int64_t t = 0; t <= rank; ++t) trace_h[t] = tr[(size_t)t];
  *rank_h = rank;
  return SMN_OK;
}

}  // namespace

extern "C" int smn_pchol_mlp(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                             double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, int64_t max_rank,
                             double tol_rel, void* L_d, int64_t ldl, double* resid_d, int64_t* pivots_h, double* trace_h,
                             int64_t* rank_h) {
  if (ctx && !pivots_h) return smn_fail(ctx, SMN_EINVAL, "smn_pchol_mlp: NULL pointer");
  return pchol_mlp_run(ctx, "smn_pchol_mlp", dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, d, max_rank, tol_rel,
                       L_d, ldl, resid_d, pivots_h, nullptr, trace_h, rank_h);
}

extern "C" int smn_pchol_mlp_at(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const int64_t* pivots_h,
                                int64_t m, double tol_rel, void* L_d, int64_t ldl, double* resid_d, double* trace_h,
                                int64_t* rank_h) {
  if (ctx && !pivots_h) return smn_fail(ctx, SMN_EINVAL, "smn_pchol_mlp_at: NULL pointer");
  return pchol_mlp_run(ctx, "smn_pchol_mlp_at", dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, d, m, tol_rel, L_d,
                       ldl, resid_d, nullptr, pivots_h, trace_h, rank_h);
}
