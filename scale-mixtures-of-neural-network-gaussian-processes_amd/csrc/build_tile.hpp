// build_tile.hpp — what the fused kernel build (kernel_build.hip) and the matrix-free product (kernel_matmul.hip) share: the
// argument block of a build launch, the per-row tables behind it, and THE epilogue of a 128x128 Gram tile -- prog.pre, the layer
// loop, prog.post and the exact diagonal -- as one body of text.  What becomes of a finished element is the caller's `sink`:
// the build stores it, the product keeps it in the accumulator registers as the operand of its second MFMA.
#pragma once
#include "gemm_nt.hpp"
#include "internal.hpp"
#include "layer_prog.hpp"

template <typename T>
struct BuildArgs {
  const T* x1; const T* x2; int64_t ld1, ld2; int kp;
  int tiles_n; int tiles_m; int symmetric; int mirror;
  int lower_skip;             // rectangular grid: drop tiles lying wholly above the global diagonal
  const T* tab1; const T* tab2; int64_t ldt1, ldt2; const T* dg; const T* dgt;
  T inv_d; LayerProg prog;
  int64_t row_off, col_off; int exact_diag;
  int store_mode; int64_t out_rows, out_cols; int64_t nv0, aug0, nv1;
  T* out_k; T* out_t; int64_t ldo;
  int use_map; TileMap map;   // XCD-aware patch order (gemm_nt.hpp)
  // paired lower-block shard (smn_kernel_mlp_shard): two trapezoids of row tiles, each packed into its own
  // output with its own leading dimension; operands and tables are the symmetric ones
  int shard; int sh_b0[2]; int sh_cnt0; T* sh_k[2]; T* sh_t[2]; int64_t sh_ld[2]; int64_t sh_cols[2];
  // cyclic column-first shard (smn_kernel_mlp_shard_cols, shard == 2): the rank's tile rows are t_j = j P + (j even ? rank :
  // P-1-rank), every lower tile of them, stored into the rank's chunk piece by piece (a piece = the tile columns
  // [cy_c[g], cy_c[g+1]) of every tile row from cy_c[g] down, cy_c[g] a multiple of P): slot (j - cy_c[g]/P) of piece g is a
  // 128 x (width of the piece) strip.  sh_k[0] / sh_t[0] are the chunk bases.
  int cy_P, cy_rank, cy_T, cy_np; int cy_c[kMaxColPieces + 1]; int64_t cy_off[kMaxColPieces];
  // batched build (smn_spr_loss_batch / smn_spr_predict_batch): problem blockIdx.y = the same operands under its own layer
  // program progs[y] (same net, act and depth; its own w, b, last_w), its own table block and its own output matrix
  const LayerProg* progs; int64_t tab_bs, out_bs; int nbatch;
  // explicit tile order (split build): tile l = tlist[l] = tr | tc << 16, dealt to the XCDs in equal contiguous shares like the map
  const int* tlist; int tlist_n;
};

// The layer program and the per-row tables of one build (kernel_build.hip): tab1 / tab2 [2 nsets + 2][ldt] of spec.dtype for the
// rows1 / rows2 padded rows whose q = |x|^2 / d is q1 / q2 (rows2 == 0: one operand, tab2 = tab1), dg / dgt the closed-form
// NNGP / NTK diagonals of the first operand.  In workspace slot 1: valid until the context's next build.
struct LayerTables {
  LayerProg prog;
  void* tab1; void* tab2; int64_t ldt; void* dg; void* dgt;
};
int layer_tables(smn_ctx* ctx, const BuildSpec& spec, bool ntk, const double* q1, int64_t rows1, const double* q2, int64_t rows2,
                 LayerTables* out);

// Tile t holds the raw Gram accumulators of rows [row0, row0 + BM) x columns [col0, col0 + 128) (mainloop has ended on a
// barrier: smem is free).  sink(m, n, i, gr, gc, k, h) gets every finished element once: (m, n, i) its accumulator slot,
// (gr, gc) its row and column in the padded operands, k / h the NNGP / NTK value (h: NTK forms only).
template <typename T, int NET, int ACT, bool NTK, int BM, typename Tile, typename Sink>
__device__ __forceinline__ void build_epilogue(const BuildArgs<T>& a, Tile& t, int64_t row0, int64_t col0, char* smem, Sink&& sink) {
  using M = typename Tile::M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  ElemProg<T, NET, ACT, NTK> prog(a.prog);
  const int nsets = a.prog.nsets;
  // (locals, not writes into `a`: a kernel argument that is written gets a private copy in scratch)
  const T* tab1 = a.tab1; const T* tab2 = a.tab2; const T* dgp = a.dg; const T* dgtp = a.dgt;
  if (a.progs) {
    prog = ElemProg<T, NET, ACT, NTK>(a.progs[blockIdx.y]);
    const int64_t tb = (int64_t)blockIdx.y * a.tab_bs;
    tab1 += tb; tab2 += tb; dgp += tb; dgtp += tb;
  }

  // stage the per-row / per-column layer tables of this tile in LDS (mainloop ended on a barrier)
  constexpr bool FAST = ElemProg<T, NET, ACT, NTK>::FAST;
  const int trows = nsets * 2 + (FAST ? 1 : 0);   // FAST: one more row, sigma (kept in the NTK-diagonal slot)
  T* srow = reinterpret_cast<T*>(smem);
  T* scol = srow + trows * kTile;
  for (int idx = tid; idx < trows * kTile; idx += 256) {
    const int s2 = idx / kTile, r = idx % kTile;
    const int g2 = s2 < nsets * 2 ? s2 : nsets * 2 + 1;
    if (r < BM) srow[idx] = tab1[(int64_t)g2 * a.ldt1 + row0 + r];
    scol[idx] = tab2[(int64_t)g2 * a.ldt2 + col0 + r];
  }
  __syncthreads();

  const T inv_d = a.inv_d;
  const bool exact_diag = a.exact_diag != 0;
  const int64_t row_off = a.row_off, col_off = a.col_off;
  typename Tile::acc_t th[Tile::MT][Tile::NT];
#pragma unroll
  for (int m = 0; m < Tile::MT; ++m)
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n)
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        T k = t.acc[m][n][i] * inv_d;
        T h = T(0);
        prog.pre(k, h);
        t.acc[m][n][i] = k;
        th[m][n][i] = h;
      }

  for (int s = 0; s < nsets; ++s) {
    const T* sr = srow + s * 2 * kTile;
    const T* sc = scol + s * 2 * kTile;
    T cr[Tile::NT], cs[Tile::NT];
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n) {
      const int lc = wc * Tile::WN + n * M::TN + M::acc_col(lane);
      cr[n] = sc[lc];
      cs[n] = sc[kTile + lc];
    }
#pragma unroll
    for (int m = 0; m < Tile::MT; ++m)
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        const int lr = wr * Tile::WM + m * M::TM + M::acc_row(lane, i);
        const T ri = sr[lr], si = sr[kTile + lr];
#pragma unroll
        for (int n = 0; n < Tile::NT; ++n) {
          T k = t.acc[m][n][i], h = th[m][n][i];
          prog.step(s, k, h, ri * cr[n], si * cs[n]);
          t.acc[m][n][i] = k;
          th[m][n][i] = h;
        }
      }
  }

#pragma unroll
  for (int m = 0; m < Tile::MT; ++m)
#pragma unroll
    for (int n = 0; n < Tile::NT; ++n)
#pragma unroll
      for (int i = 0; i < M::ACC; ++i) {
        const int64_t gr = row0 + wr * Tile::WM + m * M::TM + M::acc_row(lane, i);
        const int64_t gc = col0 + wc * Tile::WN + n * M::TN + M::acc_col(lane);
        T k = t.acc[m][n][i], h = th[m][n][i];
        T sig = T(0);
        if (FAST)
          sig = srow[nsets * 2 * kTile + (int)(gr - row0)] * scol[nsets * 2 * kTile + (int)(gc - col0)];
        prog.post(k, h, sig);
        if (exact_diag && gr + row_off == gc + col_off) {
          k = dgp[gr];
          if (NTK) h = dgtp[gr];
        }
        sink(m, n, i, gr, gc, k, h);
      }
}
