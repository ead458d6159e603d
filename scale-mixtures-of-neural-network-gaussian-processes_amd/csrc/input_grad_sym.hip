// input_grad_sym.hip — the log-marginal likelihood differentiated in the INPUTS of an MLP / dense-ResNet kernel: the form of
// input_grad.hip in which both arguments move (x2 == x1), contracted with the seed of grad.hip.  It carries automatic relevance
// determination (one positive scale per input feature, spax.kernels input_scales) and d loss / d X.
//
// With x~ the inputs as the kernel sees them, Lambda = log p(y | X) and G = coef A A^T - C K~^-1 (grad.hip:1-6; A = K~^-1 Y [n, C]),
// d Lambda = 1/2 sum_nm G_nm dK~_nm.  For n != m, K_nm = F(u_nm, v_n, v_m) with u = x~_n . x~_m / d and v_n = |x~_n|^2 / d; the
// diagonal is the closed form K_nn = F_d(v_n).  With F_1 = dF/du, F_2[n, m] = dK_nm/dv_n and ddiag_n = F_d'(v_n):
//     W_nm   = G_nm F_1[n, m]                       (n != m; W_nn = 0; W is symmetric)
//     r_n    = sum_{m != n} G_nm F_2[n, m]
//     gx_n   = dLambda/dx~_n = (sum_m W_nm x~_m + (2 r_n + G_nn ddiag_n) x~_n) / d
//     feat_j = sum_n gx[n, j] x~[n, j]              (dLambda/ds_j = feat_j / s_j for x~ = s o x;  dLambda/dx_n = s o gx_n)
// F_1, F_2 by the forward-mode chain of input_tangent.hpp (the rules and the guards at the singular points are there) with BOTH
// variance-side tangents (NV = 2): an entry of the lower triangle serves (n, m) and (m, n) at once, so beside the row-side
// tangent (seed p_n = dq_n/dv_n) it carries the column-side one (seed p_m).
//
// Kernels.
//   igs_pass_kernel      THE HOT KERNEL.  Elementwise over the 64 x 64 tiles of the lower triangle of the kept K0 = X~ X~^T / d
//                        (grad.hip's layout: a thread owns one column and the rows w, w + 4, ... of its wave; row-side table
//                        entries are wave-uniform).  State per entry (k, k_u, k_v, k_v'), NTK (theta, theta_u, theta_v, theta_v')
//                        too; G is formed per entry behind the layer loop and never stored.  Writes W for the tile and its mirror
//                        image (through LDS: both stores coalesced), zero on the diagonal and in the padding, and the tile's fp64
//                        sums of G o F_2: row side (xor tree over the 64 lanes of a row) into slot tc of the row, column side (per
//                        thread in row order, the four waves in wave order) into slot tr + 1 of the column.  A row of tile row t
//                        owns the slots 0..t (row side) and t + 1..T (column side): every slot is written exactly once.
//   igs_rowsum_kernel    s_n = the slots in order + 1/2 G_nn ddiag_n.  No floating-point atomics: two calls give the same bits.
//   (input_grad.hip)     ig_contract_kernel through input_grad_contract: out = ca (W X~) + cs s_n x~_n on the tile engine, its
//                        FEAT form leaving per (tile row, feature) the fp64 sum of out o x~; storing out is optional.
//   igs_colsum_kernel    feat_j = the tile rows' partial sums in tile-row order.
//   igs_scale_kernel     out[r, j] = x[r, j] s[j]: streaming, 16-byte accesses where the leading dimensions allow.
// Every form of the pass is free of scratch (compiler figures: profiles/r31_input_tangent.txt): the f64 NTK forms carry 4 rows at
// a time, f32 NTK and f64 NNGP 8, f32 NNGP 16.
#include <algorithm>
#include <vector>

#include "gemm_nt.hpp"
#include "input_tangent.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

constexpr int ST = 64;   // tile edge of the pass

template <typename T>
struct SymArgs {
  const T* k0; int64_t ld0;          // x~ x~^T / d, lower triangle
  const T* nkinv; int64_t ldki;      // -K~^-1, lower triangle
  const T* alpha; int nc;            // A [n, nc] row-major
  int64_t n, rows;                   // points; padded to a multiple of 128
  const T* tab; int nsets;           // [nsets][4][rows]
  T w2, b2, lw2, coef;
  T* w; int64_t ldw;                 // [rows, rows]
  double* partial;                   // [rows / 64 + 1][rows]
};

template <typename T, int NET, int ACT, bool NTK>
__global__ void __launch_bounds__(256) igs_pass_kernel(SymArgs<T> a) {
  constexpr int NR = NTK ? (sizeof(T) == 8 ? 4 : 8) : (sizeof(T) == 8 ? 8 : 16);   // rows a thread carries together
  constexpr int NPASS = (ST / 4) / NR;
  __shared__ T tile[ST][ST + 1];
  __shared__ double rowred[ST];
  __shared__ double colred[4][ST];
  int tr, tc;
  tri_decode(blockIdx.x, tr, tc);
  const int64_t row0 = (int64_t)tr * ST, col0 = (int64_t)tc * ST, n = a.n, rows = a.rows;
  const int tid = threadIdx.x;
  const int lc = tid % ST;
  const int w = __builtin_amdgcn_readfirstlane(tid / ST);
  const int64_t j = col0 + lc, jc = j < n ? j : n - 1;
  using Chain = InputTangent<T, NET, ACT, NTK, 2>;
  const Chain chain{a.w2, a.b2, a.lw2};
  const T coef = a.coef;
  double cs = 0.0;   // the column's sum of G o F_2 (column side) over the thread's rows
#pragma unroll 1
  for (int p = 0; p < NPASS; ++p) {
    const int lr0 = w + 4 * NR * p;
    typename Chain::State st[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = row0 + lr0 + 4 * r, ic = i < n ? i : n - 1;
      const int64_t hi = ic > jc ? ic : jc, lo = ic > jc ? jc : ic;
      chain.init(st[r], a.k0[hi * a.ld0 + lo]);
    }
    for (int s = 0; s < a.nsets; ++s) {
      const T* ts = a.tab + (int64_t)s * kTabFields * rows;
      const T cp = ts[rows + j], cra = ts[2 * rows + j], crb = ts[3 * rows + j];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t i = row0 + lr0 + 4 * r;   // wave-uniform
        const T pp[2] = {ts[rows + i], cp};
        chain.step(st[r], s == a.nsets - 1, ts[2 * rows + i], ts[3 * rows + i], cra, crb, pp);
      }
    }
    // the seed, formed behind the layer loop: C (-K~^-1)_ij + coef sum_c A_ic A_jc (k is dead: its slots take it)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t i = row0 + lr0 + 4 * r, ic = i < n ? i : n - 1;
      const int64_t hi = ic > jc ? ic : jc, lo = ic > jc ? jc : ic;
      st[r].k = T(a.nc) * a.nkinv[hi * a.ldki + lo];
    }
    const T* aj = a.alpha + jc * a.nc;
    for (int c = 0; c < a.nc; ++c) {
      const T ajc = aj[c];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t i = row0 + lr0 + 4 * r, ic = i < n ? i : n - 1;   // wave-uniform
        st[r].k = fma(coef * a.alpha[ic * a.nc + c], ajc, st[r].k);
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int li = lr0 + 4 * r;
      const int64_t i = row0 + li;
      const bool valid = i < n && j < i;   // the strict lower triangle (j < i < n)
      const T g = st[r].k;
      const T f1 = chain.f1(st[r]), f2r = chain.f2(st[r], 0), f2c = chain.f2(st[r], 1);
      tile[li][lc] = valid ? g * f1 : T(0);
      double rs = valid ? (double)(g * f2r) : 0.0;
      cs += valid ? (double)(g * f2c) : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) rs += __shfl_xor(rs, o);
      if (lc == 0) rowred[li] = rs;
    }
  }
  colred[w][lc] = cs;
  __syncthreads();
  if (tid < ST) {
    a.partial[(int64_t)tc * rows + row0 + tid] = rowred[tid];
  } else if (tid < 2 * ST) {
    const int t = tid - ST;
    a.partial[(int64_t)(tr + 1) * rows + col0 + t] = ((colred[0][t] + colred[1][t]) + colred[2][t]) + colred[3][t];
  }
  const bool diag = tr == tc;
#pragma unroll 4
  for (int r = 0; r < ST / 4; ++r) {
    const int li = w + 4 * r;
    const T m = tile[lc][li];   // the mirror image's entry (li, lc)
    a.w[(row0 + li) * a.ldw + col0 + lc] = diag ? tile[li][lc] + m : tile[li][lc];
    if (!diag) a.w[(col0 + li) * a.ldw + row0 + lc] = m;
  }
}

template <typename T>
__global__ void igs_rowsum_kernel(const double* __restrict__ partial, int64_t rows, int nslots, int64_t n,
                                  const T* __restrict__ nkinv, int64_t ldki, const T* __restrict__ alpha, int nc, T coef,
                                  const T* __restrict__ ddiag, double* __restrict__ s) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  double v = 0.0;
  for (int t = 0; t < nslots; ++t) v += partial[(int64_t)t * rows + r];
  if (r < n) {
    T g = T(nc) * nkinv[r * ldki + r];
    for (int c = 0; c < nc; ++c) g = fma(coef * alpha[r * nc + c], alpha[r * nc + c], g);
    v += 0.5 * (double)(g * ddiag[r]);
  } else {
    v = 0.0;
  }
  s[r] = v;
}

__global__ void igs_colsum_kernel(const double* __restrict__ fpart, int64_t dpad, int tiles, int64_t d, double* __restrict__ feat) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d) return;
  double v = 0.0;
  for (int t = 0; t < tiles; ++t) v += fpart[(int64_t)t * dpad + e];
  feat[e] = v;
}

// one thread per 16-byte chunk of a row (grid.x over the chunks, grid.y strides the rows)
template <typename T>
__global__ void __launch_bounds__(256) igs_scale_kernel(const T* x, int64_t ldx, int64_t n, int64_t d, const T* __restrict__ s, T* out,
                                                        int64_t ldo, int vec) {
  using V = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VN;
  if (k >= d) return;
  if (vec && k + VN <= d) {
    const V sv = *reinterpret_cast<const V*>(s + k);
    const T* es = reinterpret_cast<const T*>(&sv);
    for (int64_t r = blockIdx.y; r < n; r += gridDim.y) {
      const V xv = *reinterpret_cast<const V*>(x + r * ldx + k);
      const T* ex = reinterpret_cast<const T*>(&xv);
      V ov;
      T* eo = reinterpret_cast<T*>(&ov);
#pragma unroll
      for (int u = 0; u < VN; ++u) eo[u] = ex[u] * es[u];
      *reinterpret_cast<V*>(out + r * ldo + k) = ov;
    }
  } else {
    for (int64_t r = blockIdx.y; r < n; r += gridDim.y)
      for (int u = 0; u < VN && k + u < d; ++u) out[r * ldo + k + u] = x[r * ldx + k + u] * s[k + u];
  }
}

// One call's scratch in workspace slot 4 (beside what the gradient pipeline takes: one more rows^2 matrix, W, and the transposed
// inputs), and the padded inputs with their fp64 row variances in slot 0 (the layout and size of the Gram build's own copy).
struct SymWs {
  int64_t rows, kp, dpad;
  int nslots;
  size_t tab, ddiag, s, partial, w, xt, fpart, feat, bytes4, bytes0;
};

SymWs sym_ws(int dtype, int nsets, int64_t n, int64_t d) {
  const size_t es = dtype_size(dtype), ns = (size_t)(nsets > 0 ? nsets : 1);
  SymWs p{};
  p.rows = round_up(n, kTile);
  p.kp = k_pad(dtype, d);
  p.dpad = round_up(d, kTile);
  p.nslots = (int)(p.rows / ST) + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t r = off; off += al256(bytes); return r; };
  p.tab = take(es * ns * kTabFields * (size_t)p.rows);
  p.ddiag = take(es * (size_t)p.rows);
  p.s = take(sizeof(double) * (size_t)p.rows);
  p.partial = take(sizeof(double) * (size_t)p.nslots * (size_t)p.rows);
  p.w = take(es * (size_t)p.rows * (size_t)p.rows);
  p.xt = take(es * (size_t)p.dpad * (size_t)p.rows);
  p.fpart = take(sizeof(double) * (size_t)(p.rows / kTile) * (size_t)p.dpad);
  p.feat = take(sizeof(double) * (size_t)p.dpad);
  p.bytes4 = off;
  p.bytes0 = sizeof(double) * 2 * (size_t)p.rows + es * (size_t)p.kp * (size_t)p.rows;
  return p;
}

// gx / feat from the kept Gram matrix k0 (lower triangle), -K~^-1 (lower triangle), A [n, c] and coef.  x_d: the inputs as the
// kernel sees them.  feat_h != nullptr: one synchronisation at the end.
template <typename T>
int sym_run_t(smn_ctx* ctx, const BuildSpec& spec, bool ntk, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* k0,
              int64_t ld0, const void* ninv, int64_t ldinv, const void* alpha, int64_t c, double coef, void* gx_d, int64_t ldgx,
              double* feat_h) {
  const int dtype = spec.dtype;
  const int nsets = input_grad_nsets(spec);
  const SymWs p = sym_ws(dtype, nsets, n, d);
  void *w0 = nullptr, *w4 = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, p.bytes0, &w0));
  SMN_TRY(smn_workspace(ctx, 4, p.bytes4, &w4));
  char* base = static_cast<char*>(w4);
  double* q64 = static_cast<double*>(w0);
  T* xp = reinterpret_cast<T*>(q64 + 2 * p.rows);
  T* tab = reinterpret_cast<T*>(base + p.tab);
  T* ddiag = reinterpret_cast<T*>(base + p.ddiag);
  double* s = reinterpret_cast<double*>(base + p.s);
  double* partial = reinterpret_cast<double*>(base + p.partial);
  T* wm = reinterpret_cast<T*>(base + p.w);
  T* xt = reinterpret_cast<T*>(base + p.xt);
  double* fpart = reinterpret_cast<double*>(base + p.fpart);
  double* featd = reinterpret_cast<double*>(base + p.feat);
  SMN_TRY(pad_rows(ctx, dtype, x_d, n, ldx, d, xp, p.rows, p.kp, q64));
  SMN_TRY(input_grad_transpose(ctx, dtype, xp, p.rows, p.kp, d, xt));
  SMN_TRY(input_grad_tables(ctx, spec, ntk, q64, p.rows, tab, ddiag));
  const double w2 = spec.w_std * spec.w_std, b2 = spec.b_std * spec.b_std, lw2 = spec.last_w_std * spec.last_w_std;
  SymArgs<T> a;
  a.k0 = static_cast<const T*>(k0); a.ld0 = ld0;
  a.nkinv = static_cast<const T*>(ninv); a.ldki = ldinv;
  a.alpha = static_cast<const T*>(alpha); a.nc = (int)c;
  a.n = n; a.rows = p.rows;
  a.tab = tab; a.nsets = nsets;
  a.w2 = (T)w2; a.b2 = (T)b2; a.lw2 = (T)lw2; a.coef = (T)coef;
  a.w = wm; a.ldw = p.rows;
  a.partial = partial;
  const int64_t t64 = p.rows / ST, ntiles = t64 * (t64 + 1) / 2;
  {
    ProfScope ps(ctx, PROF_MISC, ctx->stream);
    with_net_form(spec.net, spec.act, ntk, [&](auto NET, auto ACT, auto NTK) -> int {
      hipLaunchKernelGGL((igs_pass_kernel<T, decltype(NET)::value, decltype(ACT)::value, decltype(NTK)::value>),
                         dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
      return SMN_OK;
    });
  }
  SMN_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(igs_rowsum_kernel<T>, dim3((unsigned)((p.rows + 255) / 256)), dim3(256), 0, ctx->stream, partial, p.rows,
                     p.nslots, n, a.nkinv, ldinv, a.alpha, (int)c, a.coef, ddiag, s);
  SMN_CHECK_LAUNCH(ctx);
  // input_grad.hip's contraction with x2 = x1 = x~: gx = (W X~ + 2 s o x~) / d, no diagonal term (s holds it)
  InputGradOps o{};
  o.spec = spec;
  o.x1p = xp; o.n1 = n; o.rows1 = p.rows;
  o.x2t = xt; o.rows2 = p.rows;
  o.kp = p.kp; o.d = d;
  InputGradWs ws{};
  ws.w = wm; ws.s = s;
  SMN_TRY(input_grad_contract(ctx, o, ws, 1.0 / (double)d, 2.0 / (double)d, 0.0, gx_d, ldgx, feat_h ? fpart : nullptr));
  if (!feat_h) return SMN_OK;
  hipLaunchKernelGGL(igs_colsum_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, ctx->stream, fpart, p.dpad,
                     (int)(p.rows / kTile), d, featd);
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipMemcpyAsync(feat_h, featd, sizeof(double) * (size_t)d, hipMemcpyDeviceToHost, ctx->stream));
  SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SMN_OK;
}

// The argument checks the two entries share: input_grad_check (which leaves the architecture in spec->net), then their operands.
int sym_check(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
              double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, int64_t c, const void* gx_d, int64_t ldgx,
              const double* feat_h, BuildSpec* spec, bool* ntk) {
  SMN_TRY(input_grad_check(ctx, who, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, spec, ntk));
  if (!x_d) return smn_fail(ctx, SMN_EINVAL, "%s: x_d is NULL", who);
  if (!gx_d && !feat_h) return smn_fail(ctx, SMN_EINVAL, "%s: gx_d and feat_h are both NULL", who);
  if (n <= 0 || d <= 0 || c < 1)
    return smn_fail(ctx, SMN_EINVAL, "%s: empty operand (n=%lld d=%lld c=%lld)", who, (long long)n, (long long)d, (long long)c);
  if (c > 48) return smn_fail(ctx, SMN_ENOTSUP, "%s: more than 48 output columns", who);
  SMN_CHECK_LD(ctx, who, ldx, d);
  if (gx_d) SMN_CHECK_LD(ctx, who, ldgx, d);
  return SMN_OK;
}

}  // namespace

extern "C" int smn_scale_columns(smn_ctx* ctx, int dtype, const void* x_d, int64_t n, int64_t ldx, int64_t d, const double* s_h,
                                 void* out_d, int64_t ldo) {
  if (!ctx) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_scale_columns";
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!x_d || !s_h || !out_d) return smn_fail(ctx, SMN_EINVAL, "%s: x_d, s_h or out_d is NULL", who);
  if (n <= 0 || d <= 0) return smn_fail(ctx, SMN_EINVAL, "%s: empty operand (n=%lld d=%lld)", who, (long long)n, (long long)d);
  SMN_CHECK_LD(ctx, who, ldx, d);
  SMN_CHECK_LD(ctx, who, ldo, d);
  return by_dtype(dtype, [&](auto e) -> int {
    using T = decltype(e);
    constexpr int VN = Vec16<T>::N;
    void* sv = nullptr;
    SMN_TRY(smn_workspace(ctx, 4, sizeof(T) * (size_t)d, &sv));
    std::vector<T> stage((size_t)d);
    for (int64_t k = 0; k < d; ++k) stage[(size_t)k] = (T)s_h[k];   // s rounded to the storage type first
    SMN_HIP(ctx, hipMemcpyAsync(sv, stage.data(), sizeof(T) * (size_t)d, hipMemcpyHostToDevice, ctx->stream));
    SMN_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (stage is a local: the upload has read it)
    const int vec = ldx % VN == 0 && ldo % VN == 0 && reinterpret_cast<uintptr_t>(x_d) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(out_d) % 16 == 0;
    const int64_t chunks = (d + VN - 1) / VN;
    const dim3 grid((unsigned)((chunks + 255) / 256), (unsigned)(n < 4096 ? n : 4096));
    hipLaunchKernelGGL(igs_scale_kernel<T>, grid, dim3(256), 0, ctx->stream, static_cast<const T*>(x_d), ldx, n, d,
                       static_cast<const T*>(sv), static_cast<T*>(out_d), ldo, vec);
    SMN_CHECK_LAUNCH(ctx);
    return SMN_OK;
  });
}

extern "C" int smn_kernel_mlp_input_grad_sym(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                             double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d,
                                             const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, int64_t c, double coef,
                                             void* gx_d, int64_t ldgx, double* feat_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_kernel_mlp_input_grad_sym";
  BuildSpec spec{};
  bool ntk = false;
  SMN_TRY(sym_check(ctx, who, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, d, c, gx_d, ldgx, feat_h, &spec,
                    &ntk));
  if (!neg_kinv_d || !alpha_d) return smn_fail(ctx, SMN_EINVAL, "%s: neg_kinv_d or alpha_d is NULL", who);
  SMN_CHECK_LD(ctx, who, ldkinv, n);
  // every workspace before the first launch: the Gram matrix and its diagonal in slot 5 (the gradient pipeline's layout), then
  // the pass's own (sym_ws)
  const size_t es = dtype_size(dtype);
  const int64_t ld0 = round_up(n, 16 / (int64_t)es);
  const SymWs p = sym_ws(dtype, input_grad_nsets(spec), n, d);
  void *k0 = nullptr, *w0 = nullptr, *w4 = nullptr;
  SMN_TRY(smn_workspace(ctx, 5, es * ((size_t)n * (size_t)ld0 + (size_t)n), &k0));
  SMN_TRY(smn_workspace(ctx, 0, p.bytes0, &w0));
  SMN_TRY(smn_workspace(ctx, 4, p.bytes4, &w4));
  void* q = static_cast<char*>(k0) + es * (size_t)n * (size_t)ld0;
  SMN_TRY(gram_lower(ctx, dtype, x_d, n, ldx, d, k0, ld0, q));
  return by_dtype(dtype, [&](auto e) {
    return sym_run_t<decltype(e)>(ctx, spec, ntk, x_d, n, ldx, d, k0, ld0, neg_kinv_d, ldkinv, alpha_d, c, coef, gx_d, ldgx, feat_h);
  });
}

extern "C" int smn_spr_loss_grad_inputs(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                        double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                                        int64_t c, double eps_abs, double df, double scale, double* quad_h, double* quad_cols_h,
                                        double* logdet_h, int* info_h, double terms_h[4], void* gx_d, int64_t ldgx, double* feat_h) {
  if (!ctx) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_spr_loss_grad_inputs";
  BuildSpec spec{};
  bool ntk = false;
  SMN_TRY(sym_check(ctx, who, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, x_d, n, ldx, d, c, gx_d, ldgx, feat_h, &spec,
                    &ntk));
  if (!y_d || !terms_h) return smn_fail(ctx, SMN_EINVAL, "%s: y_d or terms_h is NULL", who);
  if (df > 0.0 && !(scale > 0.0)) return smn_fail(ctx, SMN_EINVAL, "%s: scale must be > 0", who);
  // the pass's workspace ahead of the pipeline's first launch; slot 4 also serves the tangent contraction of the scalar terms
  // (grad.hip), which asks for less and so gets this allocation
  const SymWs p = sym_ws(dtype, input_grad_nsets(spec), n, d);
  const size_t t64 = (size_t)((n + ST - 1) / ST), terms_bytes =
      sizeof(double) * ((size_t)n * (1 + 5 * (size_t)kMaxSets) + t64 * (t64 + 1) / 2 * 4 + 4);
  void *w0 = nullptr, *w4 = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, p.bytes0, &w0));
  SMN_TRY(smn_workspace(ctx, 4, std::max(p.bytes4, terms_bytes), &w4));
  const BuildSpec full{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};   // (net with its SMN_NET_NTK flag)
  Posterior post;
  SMN_TRY(posterior_from_x(ctx, full, x_d, n, ldx, d, y_d, c, eps_abs, &post));
  const double tot = publish_head(post, c, true, n, df, scale, nullptr, quad_h, quad_cols_h, logdet_h, info_h, terms_h);
  if (post.info != 0) return SMN_OK;   // gx and feat are left untouched
  const double coef = lml_coef(df, scale, tot, n, c);
  SMN_TRY(smn_lml_grad_terms_multi(ctx, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, post.k0, n, post.ld0, post.q,
                                   post.ninv, post.ldinv, post.alpha, c, coef, terms_h));
  return by_dtype(dtype, [&](auto e) {
    return sym_run_t<decltype(e)>(ctx, spec, ntk, x_d, n, ldx, d, post.k0, post.ld0, post.ninv, post.ldinv, post.alpha, c, coef,
                                  gx_d, ldgx, feat_h);
  });
}
