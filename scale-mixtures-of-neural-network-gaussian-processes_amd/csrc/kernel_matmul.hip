// kernel_matmul.hip — out = K(x1, x2) V without K: the fused build's Gram tile and epilogue, with a second MFMA in place of the store.
//
// A workgroup owns 128 rows i of the output and one split of SMN_MATMUL_SPLIT contraction rows j.  It walks the 128x128 tiles of
// its split: the tile is built TRANSPOSED, rows j (the contraction operand, x2) by columns i (x1), by the build's own mainloop
// and epilogue (build_tile.hpp) -- every product of row and column factors in the epilogue is commutative, so element (j, i)
// carries the bits the build stores at (i, j).  The finished tile stays in the accumulator registers.  For v_mfma_*_16x16x4 an
// accumulator register is directly a B-operand fragment when the contraction runs over the tile's ROWS: lane l holds, in
// register r, row (f32: 4 (l >> 4) + r, f64: (l >> 4) + 4 r) and column l & 15 of a 16x16 block, which is B[k = l >> 4][n = l & 15]
// of a 4-deep step whose k-th element is that row.  The A operand is then V[that row][column l & 15] -- read from global memory
// by the same index formula, so the permutation of k inside a step is the same on both sides and nothing crosses LDS.  One
// 16x16 MFMA block gives out^T[16 columns of V][16 rows i]; a wave adds its 64 tile rows into NT = 4 such blocks, and the two
// waves that share the columns i are added through LDS in a fixed order at the end of the split.
//
// Determinism: a split accumulates in the MFMA's precision, tiles ascending, rows in the order above; the split's block goes to
// the workspace as fp64 and matmul_reduce_kernel adds the splits in ascending order in fp64, then shift * V in fp64.  No
// floating-point atomics.  A column of V meets only its own MFMA row, so its bits do not depend on t or on the other columns;
// operands are padded copies and V and out are element accesses, so leading dimensions and alignment do not enter.
//
// Columns: one pass holds kMatmulPass = 16 columns of V (one MFMA block row: 16 accumulator registers in f32, 32 in f64, beside
// the tile's 64 / 128); t > 16 takes further passes, each of which recomputes the Gram tiles.  K = K^T is not exploited: the
// symmetric form builds every tile of the square ("Matrix-free product").
#include <cmath>

#include "build_tile.hpp"

namespace {

constexpr int kMatmulPass = SMN_MATMUL_PASS;
constexpr int kSplitTiles = SMN_MATMUL_SPLIT / kTile;
static_assert(SMN_MATMUL_SPLIT % kTile == 0 && kSplitTiles >= 1, "SMN_MATMUL_SPLIT: a multiple of the tile edge");
static_assert(kMatmulPass == 16, "one MFMA block row of V columns per pass");

template <typename T>
struct MatmulArgs {
  const T* v; int64_t ldv;
  int64_t n2;          // valid contraction rows (rows of V); the padded rows behind them contribute exact zeros
  int64_t n1;          // valid output rows
  int64_t t, c0;       // columns of V; first column of this pass
  int nsplit, tiles_c; // splits; 128-row tiles of the contraction
  double* part;        // [nsplit][n1][t]
};

template <typename T, int NET, int ACT, bool NTK>
__global__ void __launch_bounds__(256, sizeof(T) == 8 ? 1 : 2) matmul_kernel(BuildArgs<T> a, MatmulArgs<T> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Tile = MainTile<T>;
  using M = typename Tile::M;
  using acc_t = typename Tile::acc_t;
  const int ti = (int)(blockIdx.x / (unsigned)g.nsplit), sp = (int)(blockIdx.x % (unsigned)g.nsplit);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int64_t col0 = (int64_t)ti * kTile;
  const int tj0 = sp * kSplitTiles;
  const int tj1 = tj0 + kSplitTiles < g.tiles_c ? tj0 + kSplitTiles : g.tiles_c;
  const int64_t vcol = g.c0 + (lane & 15);
  const bool vcol_ok = vcol < g.t;

  acc_t D[Tile::NT];
#pragma unroll
  for (int n = 0; n < Tile::NT; ++n)
#pragma unroll
    for (int i = 0; i < M::ACC; ++i) D[n][i] = T(0);

  for (int tj = tj0; tj < tj1; ++tj) {
    const int64_t row0 = (int64_t)tj * kTile;
    Tile t;
    t.zero();
    t.mainloop(a.x1 + row0 * a.ld1, a.ld1, a.x2 + col0 * a.ld2, a.ld2, a.kp, smem);
    build_epilogue<T, NET, ACT, NTK, kTile>(a, t, row0, col0, smem, [&](int m, int n, int i, int64_t gr, int64_t, T k, T h) {
      T val = k;
      if constexpr (NTK) val = h;
      t.acc[m][n][i] = gr < g.n2 ? val : T(0);
    });
    // the second product: out^T[16 columns of V][16 rows i] += V[rows of the block]^T  tile block
#pragma unroll
    for (int m = 0; m < Tile::MT; ++m) {
      T vv[M::ACC];
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        const int64_t j = row0 + wr * Tile::WM + m * M::TM + M::acc_row(lane, i);
        vv[i] = (vcol_ok && j < g.n2) ? g.v[j * g.ldv + vcol] : T(0);
      }
#pragma unroll
      for (int i = 0; i < M::ACC; ++i)
#pragma unroll
        for (int n = 0; n < Tile::NT; ++n) {
          if constexpr (sizeof(T) == 4) D[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[i], t.acc[m][n][i], D[n], 0, 0, 0);
          else D[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[i], t.acc[m][n][i], D[n], 0, 0, 0);
        }
    }
    __syncthreads();   // the epilogue's table reads are done before the next mainloop stages operands over them
  }

  // rows [0, 64) of every tile (waves wr = 0) + rows [64, 128) (wr = 1), in that order
  acc_t* sd = reinterpret_cast<acc_t*>(smem);
  if (wr == 1) {
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n) sd[(wc * Tile::NT + n) * 64 + lane] = D[n];
  }
  __syncthreads();
  if (wr == 0) {
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n) {
      const acc_t o = sd[(wc * Tile::NT + n) * 64 + lane];
      const int64_t gi = col0 + wc * Tile::WN + n * M::TN + M::acc_col(lane);
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        const int64_t k = g.c0 + M::acc_row(lane, i);
        if (gi < g.n1 && k < g.t) g.part[((int64_t)sp * g.n1 + gi) * g.t + k] = (double)(D[n][i] + o[i]);
      }
    }
  }
}

// out[i, k] = sum over the splits, ascending, in fp64 (+ shift V[i, k], the symmetric form)
template <typename T>
__global__ void matmul_reduce_kernel(const double* __restrict__ part, int nsplit, int64_t n1, int64_t t, double shift,
                                     const T* __restrict__ v, int64_t ldv, double* __restrict__ out, int64_t ldo) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n1 * t) return;
  const int64_t i = e / t, k = e % t;
  double sum = 0.0;
  for (int s = 0; s < nsplit; ++s) sum += part[(int64_t)s * n1 * t + e];
  if (shift != 0.0) sum += shift * (double)v[i * ldv + k];
  out[i * ldo + k] = sum;
}

template <typename T>
int matmul_t(smn_ctx* ctx, const BuildSpec& spec, bool ntk, const void* x1_d, int64_t n1, int64_t ldx1, const void* x2_d, int64_t n2,
             int64_t ldx2, int64_t d, double shift, const void* v_d, int64_t t, int64_t ldv, double* out_d, int64_t ldo) {
  const bool sym = x2_d == nullptr;
  const int64_t nc = sym ? n1 : n2;                       // contraction rows
  const int64_t kp = k_pad(spec.dtype, d);
  const int64_t r1 = round_up(n1, kTile), rc = sym ? r1 : round_up(n2, kTile);
  const int64_t tiles_i = r1 / kTile, tiles_c = rc / kTile;
  const int64_t nsplit = (tiles_c + kSplitTiles - 1) / kSplitTiles;
  if (tiles_i * nsplit >= (int64_t)INT_MAX || nsplit > 65535)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_mlp_matmul: n1 = %lld, n2 = %lld is too large", (long long)n1, (long long)nc);
  const int nsets = spec.net == SMN_NET_MLP ? spec.num_hiddens : spec.num_hiddens + 1;
  // every workspace before the first launch: padded operands (slot 0), tables (slot 1, taken again by layer_tables), partials
  void *xs = nullptr, *tabv = nullptr, *pv = nullptr;
  const size_t xbytes = sizeof(T) * (size_t)kp * (size_t)(r1 + (sym ? 0 : rc)) + sizeof(double) * (size_t)(r1 + rc);
  SMN_TRY(smn_workspace(ctx, 0, xbytes, &xs));
  SMN_TRY(smn_workspace(ctx, 1, sizeof(T) * (size_t)(2 * nsets + 2) * (size_t)(sym ? r1 : r1 + rc), &tabv));
  SMN_TRY(smn_workspace(ctx, 16, sizeof(double) * (size_t)nsplit * (size_t)n1 * (size_t)t, &pv));
  double* q1 = static_cast<double*>(xs);
  double* qc = q1 + r1;
  T* x1p = reinterpret_cast<T*>(qc + rc);
  T* xcp = sym ? x1p : x1p + kp * r1;
  SMN_TRY(pad_rows(ctx, spec.dtype, x1_d, n1, ldx1, d, x1p, r1, kp, q1));
  if (!sym) SMN_TRY(pad_rows(ctx, spec.dtype, x2_d, n2, ldx2, d, xcp, rc, kp, qc));
  LayerTables lt;
  SMN_TRY(layer_tables(ctx, spec, ntk, sym ? q1 : qc, rc, sym ? nullptr : q1, sym ? 0 : r1, &lt));   // first operand: the tile's rows

  BuildArgs<T> a{};
  a.x1 = xcp; a.ld1 = kp; a.x2 = x1p; a.ld2 = kp; a.kp = (int)kp;
  a.tab1 = static_cast<const T*>(lt.tab1); a.tab2 = static_cast<const T*>(lt.tab2); a.ldt1 = a.ldt2 = lt.ldt;
  a.dg = static_cast<const T*>(lt.dg); a.dgt = static_cast<const T*>(lt.dgt);
  a.inv_d = (T)(1.0 / (double)d); a.prog = lt.prog;
  a.symmetric = sym ? 1 : 0; a.exact_diag = sym ? 1 : 0;
  MatmulArgs<T> g{};
  g.v = static_cast<const T*>(v_d); g.ldv = ldv; g.n2 = nc; g.n1 = n1; g.t = t;
  g.nsplit = (int)nsplit; g.tiles_c = (int)tiles_c; g.part = static_cast<double*>(pv);
  size_t lds = MainTile<T>::LDS_BYTES;
  const size_t tab_lds = (size_t)(nsets * 2 + 1) * 2 * kTile * sizeof(T);
  if (tab_lds > lds) lds = tab_lds;
  SMN_TRY(with_net_form(spec.net, spec.act, ntk, [&](auto NET, auto ACT, auto NTK) {
    auto kern = matmul_kernel<T, decltype(NET)::value, decltype(ACT)::value, decltype(NTK)::value>;
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
    ProfScope ps(ctx, PROF_BUILD, ctx->stream);
    for (int64_t c0 = 0; c0 < t; c0 += kMatmulPass) {
      g.c0 = c0;
      hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_i * nsplit)), dim3(256), lds, ctx->stream, a, g);
      SMN_CHECK_LAUNCH(ctx);
    }
    return (int)SMN_OK;
  }));
  hipLaunchKernelGGL(matmul_reduce_kernel<T>, dim3((unsigned)((n1 * t + 255) / 256)), dim3(256), 0, ctx->stream, g.part, (int)nsplit, n1,
                     t, sym ? shift : 0.0, g.v, ldv, out_d, ldo);
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

}  // namespace

// The argument checks of smn_kernel_mlp_matmul, shared with smn_pcg_solve (pcg.hip): nothing is allocated or launched.
int matmul_check(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, const void* x1_d, int64_t n1, int64_t ldx1,
                 const void* x2_d, int64_t n2, int64_t ldx2, int64_t d, BuildSpec* spec, bool* ntk) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  SMN_TRY(split_net(ctx, &net, ntk));
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "%s: Unsupported act %d", who, act);
  if (num_hiddens < 0) return smn_fail(ctx, SMN_EINVAL, "%s: num_hiddens < 0", who);
  const int nsets = net == SMN_NET_MLP ? num_hiddens : num_hiddens + 1;
  if (nsets > kMaxSets) return smn_fail(ctx, SMN_ENOTSUP, "%s: %d activation layers (at most %d)", who, nsets, kMaxSets);
  if (!x1_d) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (n1 < 1 || d < 1 || (x2_d && n2 < 1))
    return smn_fail(ctx, SMN_EINVAL, "%s: empty operand (n1=%lld n2=%lld d=%lld)", who, (long long)n1, (long long)n2, (long long)d);
  SMN_CHECK_LD(ctx, who, ldx1, d);
  if (x2_d) SMN_CHECK_LD(ctx, who, ldx2, d);
  spec->dtype = dtype; spec->net = net; spec->act = act; spec->num_hiddens = num_hiddens;
  return SMN_OK;
}

extern "C" int smn_kernel_mlp_matmul(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                     double last_w_std, const void* x1_d, int64_t n1, int64_t ldx1, const void* x2_d, int64_t n2,
                                     int64_t ldx2, int64_t d, double shift, const void* v_d, int64_t t, int64_t ldv, double* out_d,
                                     int64_t ldo) {
  if (!ctx) return SMN_EINVAL;
  const char* who = "smn_kernel_mlp_matmul";
  BuildSpec spec{};
  bool ntk = false;
  SMN_TRY(matmul_check(ctx, who, dtype, net, act, num_hiddens, x1_d, n1, ldx1, x2_d, n2, ldx2, d, &spec, &ntk));
  if (!v_d || !out_d) return smn_fail(ctx, SMN_EINVAL, "%s: NULL pointer", who);
  if (t < 1) return smn_fail(ctx, SMN_EINVAL, "%s: t = %lld", who, (long long)t);
  SMN_CHECK_LD(ctx, who, ldv, t);
  SMN_CHECK_LD(ctx, who, ldo, t);
  if (!std::isfinite(shift)) return smn_fail(ctx, SMN_EINVAL, "%s: shift = %g is not finite", who, shift);
  if (x2_d && shift != 0.0) return smn_fail(ctx, SMN_EINVAL, "%s: shift = %g in the cross form (x2_d given) must be 0", who, shift);
  spec.w_std = w_std; spec.b_std = b_std; spec.last_w_std = last_w_std;
  SMN_ENTER(ctx);
  return by_dtype(dtype, [&](auto e) {
    return matmul_t<decltype(e)>(ctx, spec, ntk, x1_d, n1, ldx1, x2_d, n2, ldx2, d, shift, v_d, t, ldv, out_d, ldo);
  });
}
