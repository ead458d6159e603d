// input_grad.hip — the derivative of an MLP / dense-ResNet kernel entry with respect to its FIRST argument
// (smn_kernel_mlp_input_grad; the device side of smn_fit_predict_grad, fit.hip).
//
// K(x1_r, x2_j) = F(u, v) with u = k0_rj = x1_r . x2_j / d and v = q0_r = |x1_r|^2 / d (x2 is a constant), so
//     dK_rj / dx1_r = (F_1 x2_j + 2 F_2 x1_r) / d,      F_1 = dF/du,  F_2 = dF/dv
// and for a seed G [n1, n2]
//     gx[r, :] = sum_j G_rj dK_rj/dx1_r = ((G o F_1) X2 + 2 rowsum(G o F_2) o x1) / d.
// F_1 and F_2 come from forward mode through the layer stack: the chain of input_tangent.hpp (its rules, their derivation and
// the guards at the singular points are there) with the row-side variance tangent alone, every column-side tangent being 0.
//
// Kernels.
//   ig_tables_kernel   per row and activation layer, fp64 arithmetic stored in the chain's type: q, p = dq/dq0, ra, rb; and per
//                      row the derivative of the closed-form diagonal, dK_rr/dq0 (NNGP) or dTheta_rr/dq0 (NTK).
//   ig_tile_kernel     THE HOT KERNEL.  One workgroup per 128 x 128 tile of (x1 rows) x (x2 rows): K0 on the MFMA tile engine
//                      (gemm_nt.hpp; never stored), the tangent chain (input_tangent.hpp, NV = 1) in the epilogue in the storage
//                      type's arithmetic, four entries of one row at a time (the chain's live state is 4 x 3 values, NTK 4 x 6,
//                      beside the tile's 64 accumulators).  Plain form: F_1 and F_2 [rows1, rows2] to workspace.  Seeded form: G o F_1 instead of F_1
//                      and, instead of F_2, the tile's fp64 row sums of G o F_2 (lanes of a row by the xor tree, the two
//                      waves of a row in wave order), one slot per (tile column, row).
//   ig_rowsum_kernel   the tile columns' partial sums added in tile order: no floating-point atomics anywhere, two calls give
//                      the same bits.
//   ig_seed_kernel     streaming, 16-byte accesses: W = F_1 o seed and s_r = sum_j F_2[r, j] seed[r, j] in fp64 (the read-out
//                      kernel's order, fit.hip) for a seed that is one vector for all rows (alpha_k) or a matrix (U).
//   ig_contract_kernel (G o F_1) X2 on the tile engine as the NT product W [rows1, rows2] x X2T [d, rows2]^T, the epilogue
//                      adding the row term:  out[r, e] = ca acc + (cs s_r + cd dd_r) x1[r, e]  (the dd term optional: the
//                      predictive variance has it).  THE contraction of input_grad_sym.hip too (x2 = x1), whose FEAT form adds,
//                      per (tile row, feature), the fp64 sum of out o x1 (per thread in accumulator order, then the eight
//                      threads of a column in a fixed order); storing out is optional there.
// Routes.  Every form of the hot kernel is fused (Gram tile + chain in one launch) and free of scratch, with one exception: the
// SEEDED f64 NTK forms are not built -- the largest of them (dense ResNet, ReLU) came out of the compiler with its 64 accumulators
// in a 544-byte stack object -- and smn_kernel_mlp_input_grad takes those through the plain fused form and ig_seed_kernel on a
// padded copy of the seed instead.  Compiler figures: profiles/r31_input_tangent.txt (r21_input_grad.txt: when the kernel was written).
#include <algorithm>

#include "gemm_nt.hpp"
#include "input_tangent.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

namespace {

template <int NET, int ACT, typename R>
__global__ void ig_tables_kernel(const double* __restrict__ q0, int64_t n, int nsets, double w2, double b2, double lw2, int ntk,
                                 R* __restrict__ tab, R* __restrict__ ddiag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // (q, q_t) the variance and (th, th_t) the tangent-kernel diagonal with their derivatives in q0; ResNet: th holds T
  double q = q0[i], qt = 1.0, th = 0.0, tht = 0.0;
  if (NET == NET_RESNET) {
    q = w2 * q + b2;
    qt = w2;
    th = q;
    tht = qt;
  }
  for (int s = 0; s < nsets; ++s) {
    if (NET == NET_MLP) {   // Dense in front of every activation
      q = w2 * q + b2;
      qt = w2 * qt;
      th = q + w2 * th;
      tht = qt + w2 * tht;
    }
    R* t = tab + (int64_t)s * kTabFields * n + i;
    t[0] = (R)q;
    t[n] = (R)qt;
    double o, oq, dd, ddq;   // the activation on the diagonal: phi(q, q, q), its slope, D and its slope
    if (ACT == ACT_RELU) {
      t[2 * n] = (R)(q > 0.0 ? 1.0 / sqrt(q) : 0.0);
      t[3 * n] = (R)(q > 0.0 ? sqrt(q) : 0.0);
      o = 0.5 * q; oq = 0.5; dd = 0.5; ddq = 0.0;
    } else {
      const double t1 = 1.0 + 2.0 * q, t2 = 1.0 + 4.0 * q, r2 = sqrt(t2);
      t[2 * n] = (R)(1.0 / sqrt(t1));
      t[3 * n] = (R)(1.0 / t1);
      o = (2.0 / kPiD) * asin(2.0 * q / t1);
      oq = (4.0 / kPiD) / (t1 * r2);
      dd = (4.0 / kPiD) / r2;
      ddq = -(8.0 / kPiD) / (t2 * r2);
    }
    const double ot = oq * qt, to = th * dd, tot = tht * dd + th * ddq * qt;
    if (NET == NET_RESNET && s != nsets - 1) {   // S <- Dense(act(S)) + S
      const double a2 = w2 * o + b2, a2t = w2 * ot;
      q += a2; qt += a2t;
      th += a2 + w2 * to; tht += a2t + w2 * tot;
    } else {
      q = o; qt = ot; th = to; tht = tot;
    }
  }
  if (ddiag) ddiag[i] = (R)(lw2 * (ntk ? qt + tht : qt));
}

template <typename T>
struct IgArgs {
  const T* x1; const T* x2; int64_t kp;          // padded operands (ld = kp)
  const T* tab1; int64_t ldt1;                   // ig_tables_kernel output of the x1 rows / the x2 rows
  const T* tab2; int64_t ldt2;
  int nsets;
  T inv_d, w2, b2, lw2;
  int64_t n1, n2, rows1;
  T* f1; T* f2; int64_t ldf;                     // [rows1, ldf >= rows2]; seeded: f1 = G o F_1, f2 unused
  const T* g; int64_t ldg;                       // seeded: the seed [n1, n2]
  double* partial;                               // seeded: [tiles_n][rows1]
  TileMap map;
};

// LDS behind the mainloop: the row-side tables (p, ra, rb) and column-side tables (ra, rb) of the tile's activation layers, then
// (seeded) the two waves' row sums
template <typename T>
size_t ig_tile_lds(int nsets) {
  return std::max<size_t>(MainTile<T>::LDS_BYTES, sizeof(T) * (size_t)nsets * 5 * kTile + sizeof(double) * 2 * kTile);
}

// (waves per SIMD stated: left to itself the compiler aims the largest f64 form at two waves and spills the accumulators)
template <typename T, int NET, int ACT, bool NTK, bool SEEDED>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, sizeof(T) == 8 ? 1 : 2))) ig_tile_kernel(IgArgs<T> a) {
  using Tile = MainTile<T>;
  using M = typename Tile::M;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int tr, tc;
  if (!a.map.decode(blockIdx.x, tr, tc)) return;
  const int64_t row0 = (int64_t)tr * kTile, col0 = (int64_t)tc * kTile;
  Tile t;
  t.zero();
  t.mainloop(a.x1 + row0 * a.kp, a.kp, a.x2 + col0 * a.kp, a.kp, (int)a.kp, smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int nsets = a.nsets;
  T* srow = reinterpret_cast<T*>(smem);            // [nsets][3][128]
  T* scol = srow + (size_t)nsets * 3 * kTile;      // [nsets][2][128]
  double* red = reinterpret_cast<double*>(smem + sizeof(T) * (size_t)nsets * 5 * kTile);   // [2][128]
  for (int idx = tid; idx < nsets * kTile; idx += 256) {
    const int s = idx / kTile, r = idx % kTile;
    const T* t1 = a.tab1 + (int64_t)s * kTabFields * a.ldt1 + row0 + r;
    const T* t2 = a.tab2 + (int64_t)s * kTabFields * a.ldt2 + col0 + r;
    srow[(s * 3 + 0) * kTile + r] = t1[a.ldt1];
    srow[(s * 3 + 1) * kTile + r] = t1[2 * a.ldt1];
    srow[(s * 3 + 2) * kTile + r] = t1[3 * a.ldt1];
    scol[(s * 2 + 0) * kTile + r] = t2[2 * a.ldt2];
    scol[(s * 2 + 1) * kTile + r] = t2[3 * a.ldt2];
  }
  __syncthreads();

  constexpr int NT = Tile::NT;
  constexpr int NG = (sizeof(T) == 8 && NTK) ? 2 : NT;   // entries of a row carried together (six f64 values each: two)
  using Chain = InputTangent<T, NET, ACT, NTK, 1>;
  const Chain chain{a.w2, a.b2, a.lw2};
  int lcs[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) lcs[n] = wc * Tile::WN + n * M::TN + M::acc_col(lane);
#pragma unroll
  for (int m = 0; m < Tile::MT; ++m)
#pragma unroll
    for (int i = 0; i < M::ACC; ++i) {
      const int lr = wr * Tile::WM + m * M::TM + M::acc_row(lane, i);
      const int64_t row = row0 + lr;
      double rs = 0.0;
#pragma unroll
     for (int n0 = 0; n0 < NT; n0 += NG) {
      typename Chain::State st[NG];
#pragma unroll
      for (int n = 0; n < NG; ++n) chain.init(st[n], t.acc[m][n0 + n][i] * a.inv_d);
      for (int s = 0; s < nsets; ++s) {
        const T rp[1] = {srow[(s * 3 + 0) * kTile + lr]};
        const T rra = srow[(s * 3 + 1) * kTile + lr], rrb = srow[(s * 3 + 2) * kTile + lr];
#pragma unroll
        for (int n = 0; n < NG; ++n)
          chain.step(st[n], s == nsets - 1, rra, rrb, scol[(s * 2 + 0) * kTile + lcs[n0 + n]],
                     scol[(s * 2 + 1) * kTile + lcs[n0 + n]], rp);
      }
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        const int64_t col = col0 + lcs[n0 + n];
        const T f1 = chain.f1(st[n]), f2 = chain.f2(st[n], 0);
        if (SEEDED) {
          const T g = (row < a.n1 && col < a.n2) ? a.g[row * a.ldg + col] : T(0);
          a.f1[row * a.ldf + col] = g * f1;
          rs += (double)(g * f2);
        } else {
          a.f1[row * a.ldf + col] = f1;
          a.f2[row * a.ldf + col] = f2;
        }
      }
     }
      if (SEEDED) {   // the 16 lanes that share this row (both MFMA layouts: the row is a function of lane >> 4)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) rs += __shfl_xor(rs, o);
        if ((lane & 15) == 0) red[wc * kTile + lr] = rs;
      }
    }
  if (SEEDED) {
    __syncthreads();
    if (tid < kTile) a.partial[(int64_t)tc * a.rows1 + row0 + tid] = red[tid] + red[kTile + tid];
  }
}

__global__ void ig_rowsum_kernel(const double* __restrict__ partial, int64_t rows, int tiles_n, double* __restrict__ s) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  double v = 0.0;
  for (int t = 0; t < tiles_n; ++t) v += partial[(int64_t)t * rows + r];
  s[r] = v;
}

// One workgroup (four waves) per row r:  w[r, j] = f1[r, j] seed_rj,  s[r] = sum_j f2[r, j] seed_rj  (j < cols, a multiple of
// 128; seed_rj = seed[r * lds + j], lds = 0: one vector for every row).  fp64 sums per lane in column order, the xor tree over a
// wave, the four waves in wave order: the order depends on cols alone.
template <typename T>
__global__ void __launch_bounds__(256) ig_seed_kernel(const T* __restrict__ f1, const T* __restrict__ f2, int64_t ldf, int64_t cols,
                                                      const T* __restrict__ seed, int64_t lds, T* __restrict__ w, int64_t ldw,
                                                      double* __restrict__ s) {
  using V = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  __shared__ double red[4];
  const int64_t row = blockIdx.x;
  const T* a1 = f1 + row * ldf;
  const T* a2 = f2 + row * ldf;
  const T* sd = seed + row * lds;
  T* wr = w + row * ldw;
  double ss = 0.0;
  for (int64_t k = (int64_t)threadIdx.x * VN; k < cols; k += 256 * VN) {
    const V v1 = *reinterpret_cast<const V*>(a1 + k), v2 = *reinterpret_cast<const V*>(a2 + k);
    const V sv = *reinterpret_cast<const V*>(sd + k);
    const T* e1 = reinterpret_cast<const T*>(&v1);
    const T* e2 = reinterpret_cast<const T*>(&v2);
    const T* es = reinterpret_cast<const T*>(&sv);
    V ov;
    T* eo = reinterpret_cast<T*>(&ov);
#pragma unroll
    for (int u = 0; u < VN; ++u) {
      eo[u] = e1[u] * es[u];
      ss += (double)e2[u] * (double)es[u];
    }
    *reinterpret_cast<V*>(wr + k) = ov;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) s[row] = ((red[0] + red[1]) + red[2]) + red[3];
}

// dst[r, cols - 1 - j] = src[r, j]: the column reversal that turns the backward substitution of solved rows into the forward
// sweep (heads.hip smn_trsm, trans = 1), coalesced on both sides.
template <typename T>
__global__ void ig_flip_rows_kernel(T* __restrict__ dst, int64_t ldd, const T* __restrict__ src, int64_t lds, int64_t rows,
                                    int64_t cols) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) dst[r * ldd + (cols - 1 - j)] = src[r * lds + j];
}

template <typename T>
struct IgcArgs {
  const T* w; int64_t ldw;       // [rows1, K]
  const T* x2t; int64_t ldt;     // [round_up(d, 128), K]
  int K;
  const T* x1; int64_t kp;       // the padded x1 (row term)
  const double* s; const T* dd;  // row sums; diagonal derivative (or null)
  double ca, cs, cd;
  T* out; int64_t ldo;           // (FEAT: or null)
  double* fpart; int64_t dpad;   // FEAT: [rows1 / 128][dpad]
  int64_t n1, d;
};

template <typename T, bool FEAT>
__global__ void __launch_bounds__(256) ig_contract_kernel(IgcArgs<T> a) {
  using Tile = MainTile<T>;
  using M = typename Tile::M;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t row0 = (int64_t)blockIdx.y * kTile, e0 = (int64_t)blockIdx.x * kTile;
  Tile t;
  t.zero();
  t.mainloop(a.w + row0 * a.ldw, a.ldw, a.x2t + e0 * a.ldt, a.ldt, a.K, smem);
  double fs[Tile::NT];   // FEAT: per column of the thread, the sum of out o x1 over its rows
#pragma unroll
  for (int n = 0; n < Tile::NT; ++n) fs[n] = 0.0;
  t.for_each([&](int m, int n, int i, int lr, int lc) {
    const int64_t r = row0 + lr, e = e0 + lc;
    if (r < a.n1 && e < a.d) {
      const double x = (double)a.x1[r * a.kp + e];
      const double rc = a.cs * a.s[r] + (a.dd ? a.cd * (double)a.dd[r] : 0.0);
      const T o = (T)(a.ca * (double)t.acc[m][n][i] + rc * x);
      if (!FEAT || a.out) a.out[r * a.ldo + e] = o;
      if (FEAT) fs[n] += (double)o * x;
    }
  });
  if (FEAT) {   // (the mainloop ends with a barrier: its LDS is free)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double* red = reinterpret_cast<double*>(smem);   // [2 wave rows][4 row groups of a wave][128 columns]
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n)
      red[(wr * 4 + (lane >> 4)) * kTile + wc * Tile::WN + n * M::TN + M::acc_col(lane)] = fs[n];
    __syncthreads();
    if (threadIdx.x < kTile) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) v += red[q * kTile + threadIdx.x];
      a.fpart[(int64_t)blockIdx.y * a.dpad + e0 + threadIdx.x] = v;
    }
  }
}

template <typename T>
int ig_factors_t(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, const void* gbar, int64_t ldg) {
  const int nsets = input_grad_nsets(o.spec);
  const double w2 = o.spec.w_std * o.spec.w_std, b2 = o.spec.b_std * o.spec.b_std, lw2 = o.spec.last_w_std * o.spec.last_w_std;
  const bool seeded = gbar != nullptr;
  IgArgs<T> a;
  a.x1 = static_cast<const T*>(o.x1p); a.x2 = static_cast<const T*>(o.x2p); a.kp = o.kp;
  a.tab1 = static_cast<const T*>(w.tab1); a.ldt1 = o.rows1;
  a.tab2 = static_cast<const T*>(w.tab2); a.ldt2 = o.rows2;
  a.nsets = nsets;
  a.inv_d = (T)(1.0 / (double)o.d); a.w2 = (T)w2; a.b2 = (T)b2; a.lw2 = (T)lw2;
  a.n1 = o.n1; a.n2 = o.n2; a.rows1 = o.rows1;
  a.f1 = static_cast<T*>(seeded ? w.w : w.f1); a.f2 = static_cast<T*>(w.f2); a.ldf = o.rows2;
  a.g = static_cast<const T*>(gbar); a.ldg = ldg;
  a.partial = w.partial;
  a.map = TileMap::make(o.rows1 / kTile, o.rows2 / kTile, 0);
  const size_t lds = ig_tile_lds<T>(nsets);
  return with_net_form(o.spec.net, o.spec.act, o.ntk, [&](auto NET, auto ACT, auto NTK) -> int {
    constexpr int net = decltype(NET)::value, act = decltype(ACT)::value;
    constexpr bool ntk = decltype(NTK)::value;
    const dim3 gt1((unsigned)((o.rows1 + 255) / 256)), gt2((unsigned)((o.rows2 + 255) / 256));
    hipLaunchKernelGGL((ig_tables_kernel<net, act, T>), gt1, dim3(256), 0, ctx->stream, o.q1, o.rows1, nsets, w2, b2, lw2,
                       ntk ? 1 : 0, static_cast<T*>(w.tab1), static_cast<T*>(w.ddiag));
    hipLaunchKernelGGL((ig_tables_kernel<net, act, T>), gt2, dim3(256), 0, ctx->stream, o.q2, o.rows2, nsets, w2, b2, lw2,
                       ntk ? 1 : 0, static_cast<T*>(w.tab2), static_cast<T*>(nullptr));
    SMN_CHECK_LAUNCH(ctx);
    ProfScope ps(ctx, PROF_BUILD, ctx->stream);
    if (seeded) {
      if constexpr (sizeof(T) == 8 && ntk) {   // (input_grad_seeded_fused: these forms are not built)
        return smn_fail(ctx, SMN_EINVAL, "input_grad_factors: the f64 NTK form has no fused seeded kernel");
      } else {
        auto kern = ig_tile_kernel<T, net, act, ntk, true>;
        SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)a.map.grid), dim3(256), lds, ctx->stream, a);
      }
    } else {
      auto kern = ig_tile_kernel<T, net, act, ntk, false>;
      SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
      hipLaunchKernelGGL(kern, dim3((unsigned)a.map.grid), dim3(256), lds, ctx->stream, a);
    }
    SMN_CHECK_LAUNCH(ctx);
    if (seeded) {
      hipLaunchKernelGGL(ig_rowsum_kernel, gt1, dim3(256), 0, ctx->stream, w.partial, o.rows1, (int)(o.rows2 / kTile), w.s);
      SMN_CHECK_LAUNCH(ctx);
    }
    return SMN_OK;
  });
}

}  // namespace

bool input_grad_seeded_fused(int dtype, bool ntk) { return !(dtype == SMN_F64 && ntk); }

int input_grad_nsets(const BuildSpec& spec) { return spec.net == SMN_NET_MLP ? spec.num_hiddens : spec.num_hiddens + 1; }

int input_grad_check(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                     double last_w_std, BuildSpec* spec, bool* ntk) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  SMN_TRY(split_net(ctx, &net, ntk));
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "%s: Unsupported act %d", who, act);
  if (num_hiddens < 0) return smn_fail(ctx, SMN_EINVAL, "%s: num_hiddens = %d", who, num_hiddens);
  *spec = BuildSpec{dtype, net, act, num_hiddens, w_std, b_std, last_w_std};
  if (input_grad_nsets(*spec) > kMaxSets)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: num_hiddens too large (max %d activation layers)", who, kMaxSets);
  return SMN_OK;
}

InputGradWs input_grad_ws_carve(void* base, int dtype, int nsets, int64_t rows1, int64_t rows2, bool seeded) {
  const size_t es = dtype_size(dtype), ns = (size_t)(nsets > 0 ? nsets : 1), mat = es * (size_t)rows1 * (size_t)rows2;
  char* p = static_cast<char*>(base);
  auto take = [&](size_t bytes) { void* r = p; p += al256(bytes); return r; };
  InputGradWs w{};
  w.tab1 = take(es * ns * kTabFields * (size_t)rows1);
  w.tab2 = take(es * ns * kTabFields * (size_t)rows2);
  w.ddiag = take(es * (size_t)rows1);
  w.s = static_cast<double*>(take(sizeof(double) * (size_t)rows1));
  w.w = take(mat);
  if (seeded) {
    w.partial = static_cast<double*>(take(sizeof(double) * (size_t)(rows2 / kTile) * (size_t)rows1));
  } else {
    w.f1 = take(mat);
    w.f2 = take(mat);
  }
  w.bytes = (size_t)(p - static_cast<char*>(base));
  return w;
}

// (the layout laid over a null base: only the size is read)
size_t input_grad_ws_bytes(int dtype, int nsets, int64_t rows1, int64_t rows2, bool seeded) {
  return input_grad_ws_carve(nullptr, dtype, nsets, rows1, rows2, seeded).bytes;
}

int input_grad_factors(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, const void* gbar_d, int64_t ldg) {
  return by_dtype(o.spec.dtype, [&](auto e) { return ig_factors_t<decltype(e)>(ctx, o, w, gbar_d, ldg); });
}

int input_grad_tables(smn_ctx* ctx, const BuildSpec& spec, bool ntk, const double* q64, int64_t rows, void* tab_d, void* ddiag_d) {
  const int nsets = input_grad_nsets(spec);
  const double w2 = spec.w_std * spec.w_std, b2 = spec.b_std * spec.b_std, lw2 = spec.last_w_std * spec.last_w_std;
  by_dtype(spec.dtype, [&](auto e) {
    using T = decltype(e);
    with_net_form(spec.net, spec.act, ntk, [&](auto NET, auto ACT, auto) -> int {
      hipLaunchKernelGGL((ig_tables_kernel<decltype(NET)::value, decltype(ACT)::value, T>), dim3((unsigned)((rows + 255) / 256)),
                         dim3(256), 0, ctx->stream, q64, rows, nsets, w2, b2, lw2, ntk ? 1 : 0, static_cast<T*>(tab_d),
                         static_cast<T*>(ddiag_d));
      return SMN_OK;
    });
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

int input_grad_seed(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, const void* seed_d, int64_t lds) {
  by_dtype(o.spec.dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(ig_seed_kernel<T>, dim3((unsigned)o.rows1), dim3(256), 0, ctx->stream, static_cast<const T*>(w.f1),
                       static_cast<const T*>(w.f2), o.rows2, o.rows2, static_cast<const T*>(seed_d), lds, static_cast<T*>(w.w),
                       o.rows2, w.s);
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

int input_grad_contract(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, double ca, double cs, double cd, void* out_d,
                        int64_t ldo, double* fpart_d) {
  return by_dtype(o.spec.dtype, [&](auto e) -> int {
    using T = decltype(e);
    IgcArgs<T> a;
    a.w = static_cast<const T*>(w.w); a.ldw = o.rows2;
    a.x2t = static_cast<const T*>(o.x2t); a.ldt = o.rows2;
    a.K = (int)o.rows2;
    a.x1 = static_cast<const T*>(o.x1p); a.kp = o.kp;
    a.s = w.s; a.dd = cd != 0.0 ? static_cast<const T*>(w.ddiag) : nullptr;
    a.ca = ca; a.cs = cs; a.cd = cd;
    a.out = static_cast<T*>(out_d); a.ldo = ldo;
    a.fpart = fpart_d; a.dpad = round_up(o.d, kTile);
    a.n1 = o.n1; a.d = o.d;
    auto kern = fpart_d ? ig_contract_kernel<T, true> : ig_contract_kernel<T, false>;
    const size_t lds = MainTile<T>::LDS_BYTES;
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
    ProfScope ps(ctx, PROF_TRAIL, ctx->stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.dpad / kTile), (unsigned)(o.rows1 / kTile)), dim3(256), lds, ctx->stream, a);
    SMN_CHECK_LAUNCH(ctx);
    return SMN_OK;
  });
}

int input_grad_transpose(smn_ctx* ctx, int dtype, const void* xp, int64_t rows, int64_t kp, int64_t d, void* xt_d) {
  SMN_HIP(ctx, hipMemsetAsync(xt_d, 0, dtype_size(dtype) * (size_t)round_up(d, kTile) * (size_t)rows, ctx->stream));
  return transpose_matrix(ctx, dtype, xt_d, rows, xp, kp, rows, d);
}

int flip_rows(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return SMN_OK;
  const dim3 g((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768));
  by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(ig_flip_rows_kernel<T>, g, dim3(256), 0, ctx->stream, static_cast<T*>(dst), ldd, static_cast<const T*>(src),
                       lds, rows, cols);
  });
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

extern "C" int smn_kernel_mlp_input_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                         double last_w_std, const void* x1_d, int64_t n1, int64_t ldx1, const void* x2_d,
                                         int64_t n2, int64_t ldx2, int64_t d, const void* gbar_d, int64_t ldg, void* gx_d,
                                         int64_t ldgx) {
  if (!ctx) return SMN_EINVAL;
  SMN_ENTER(ctx);
  const char* who = "smn_kernel_mlp_input_grad";
  InputGradOps o{};
  SMN_TRY(input_grad_check(ctx, who, dtype, net, act, num_hiddens, w_std, b_std, last_w_std, &o.spec, &o.ntk));
  if (!x2_d)
    return smn_fail(ctx, SMN_EINVAL, "%s: x2_d is NULL: the form in which both arguments move (x2 == x1) is not implemented", who);
  if (!x1_d || !gbar_d || !gx_d) return smn_fail(ctx, SMN_EINVAL, "%s: x1_d, gbar_d or gx_d is NULL", who);
  if (n1 <= 0 || n2 <= 0 || d <= 0)
    return smn_fail(ctx, SMN_EINVAL, "%s: empty operand (n1=%lld n2=%lld d=%lld)", who, (long long)n1, (long long)n2, (long long)d);
  SMN_CHECK_LD(ctx, who, ldx1, d);
  SMN_CHECK_LD(ctx, who, ldx2, d);
  SMN_CHECK_LD(ctx, who, ldg, n2);
  SMN_CHECK_LD(ctx, who, ldgx, d);
  const bool ntk = o.ntk;
  const int nsets = input_grad_nsets(o.spec);
  const size_t es = dtype_size(dtype);
  o.kp = k_pad(dtype, d); o.d = d;
  o.n1 = n1; o.rows1 = round_up(n1, kTile);
  o.n2 = n2; o.rows2 = round_up(n2, kTile);
  // every workspace before the first launch: the padded operands (slot 0); tables, sums and G o F_1, then X2^T, then (f64 NTK)
  // the padded seed, all in slot 4
  void *xs = nullptr, *wsv = nullptr;
  SMN_TRY(smn_workspace(ctx, 0, sizeof(double) * (size_t)(o.rows1 + o.rows2) + es * (size_t)o.kp * (size_t)(o.rows1 + o.rows2), &xs));
  const bool fused = input_grad_seeded_fused(dtype, ntk);
  const size_t ig_bytes = input_grad_ws_bytes(dtype, nsets, o.rows1, o.rows2, fused);
  const size_t xt_bytes = al256(es * (size_t)round_up(d, kTile) * (size_t)o.rows2);
  SMN_TRY(smn_workspace(ctx, 4, ig_bytes + xt_bytes + (fused ? 0 : es * (size_t)o.rows1 * (size_t)o.rows2), &wsv));
  void* xt = static_cast<char*>(wsv) + ig_bytes;
  double* q1 = static_cast<double*>(xs);
  double* q2 = q1 + o.rows1;
  char* x1p = reinterpret_cast<char*>(q2 + o.rows2);
  char* x2p = x1p + es * (size_t)o.kp * (size_t)o.rows1;
  SMN_TRY(pad_rows(ctx, dtype, x1_d, n1, ldx1, d, x1p, o.rows1, o.kp, q1));
  SMN_TRY(pad_rows(ctx, dtype, x2_d, n2, ldx2, d, x2p, o.rows2, o.kp, q2));
  o.x1p = x1p; o.q1 = q1; o.x2p = x2p; o.q2 = q2;
  SMN_TRY(input_grad_transpose(ctx, dtype, x2p, o.rows2, o.kp, d, xt));
  o.x2t = xt;
  const InputGradWs w = input_grad_ws_carve(wsv, dtype, nsets, o.rows1, o.rows2, fused);
  if (fused) {
    SMN_TRY(input_grad_factors(ctx, o, w, gbar_d, ldg));
  } else {   // F_1, F_2 by the plain form, then the streaming seed pass on a zero-padded copy of gbar
    void* gp = static_cast<char*>(wsv) + ig_bytes + xt_bytes;
    SMN_HIP(ctx, hipMemsetAsync(gp, 0, es * (size_t)o.rows1 * (size_t)o.rows2, ctx->stream));
    SMN_TRY(copy_matrix(ctx, dtype, gp, o.rows2, gbar_d, ldg, n1, n2, 0));
    SMN_TRY(input_grad_factors(ctx, o, w, nullptr, 0));
    SMN_TRY(input_grad_seed(ctx, o, w, gp, o.rows2));
  }
  const double inv_d = 1.0 / (double)d;
  return input_grad_contract(ctx, o, w, inv_d, 2.0 * inv_d, 0.0, gx_d, ldgx);
}
