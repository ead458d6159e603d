// cnn_pairs.hpp — what the conv-NNGP pair kernels share (cnn.hip: the forward build, cnn_grad.hip: its forward-mode
// tangents): the layer program, the launch arguments of a pair kernel and the order in which the waves walk the image pairs.
#pragma once
#include "internal.hpp"

namespace smn_cnn {

template <typename T>
__device__ __forceinline__ T rsqrt_any(T x);
template <>
__device__ __forceinline__ float rsqrt_any<float>(float x) { return __builtin_amdgcn_rsqf(x); }
template <>
__device__ __forceinline__ double rsqrt_any<double>(double x) { return 1.0 / sqrt(x); }
template <typename T>
__device__ __forceinline__ T rcp_any(T x);
template <>
__device__ __forceinline__ float rcp_any<float>(float x) { return __builtin_amdgcn_rcpf(x); }
template <>
__device__ __forceinline__ double rcp_any<double>(double x) {   // v_rcp_f64 + two Newton steps: full double precision
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}

struct ConvProg {
  int act, layers, H, W, C;
  double w2, b2, lw2;
};

template <typename T>
struct PairArgs {
  const T* x1; const T* x2; const T* R1; const T* R2; const T* diag;
  int64_t n1, n2; int symmetric, mirror;
  ConvProg prog;
  T* out; int64_t ldo; int64_t npairs;
  int tile_bn;   // > 0: XCD-tiled pair order (below), tiles of tile_bn x 32 image pairs; 0: plain strided order
};

// The pair list of one wave: plain strided order, or the XCD-tiled order described below.  next() is wave-uniform.
template <typename T>
struct PairWalk {
  const PairArgs<T>& a;
  bool tiled; int xcd, tidx; int64_t tiles_m, tiles_n, tn, tm, pr, step;
  __device__ __forceinline__ PairWalk(const PairArgs<T>& a_, int wave) : a(a_) {
    tiled = a.tile_bn > 0;
    xcd = (int)(blockIdx.x & 7);
    tidx = (int)(blockIdx.x >> 3) * 4 + wave;   // this wave's pair inside every tile of its XCD
    tiles_m = (a.n2 + 31) / 32;
    tiles_n = tiled ? (a.n1 + a.tile_bn - 1) / a.tile_bn : 0;
    tn = 0;
    tm = xcd - 8;
    step = (int64_t)gridDim.x * 4;
    pr = (int64_t)blockIdx.x * 4 + wave - step;
  }
  __device__ __forceinline__ int64_t row_tiles(int64_t r) const {   // tiles of tile row r that hold a wanted pair
    if (!a.symmetric) return tiles_m;
    const int64_t c = (r * a.tile_bn + a.tile_bn - 1) / 32 + 1;
    return c < tiles_m ? c : tiles_m;
  }
  __device__ __forceinline__ bool next(int64_t& n, int64_t& m) {
    if (tiled) {
      // XCD x walks the lower (or all) tiles with (tn + tm) % 8 == x, row by row: dealt round-robin inside a tile row
      // with the offset rotating from row to row, so every XCD gets the same share of the triangle
      for (;;) {
        tm += 8;
        while (tn < tiles_n && tm >= row_tiles(tn)) {
          ++tn;
          tm = (xcd - tn) & 7;
        }
        if (tn >= tiles_n) return false;
        n = tn * a.tile_bn + (tidx >> 5);
        m = tm * 32 + (tidx & 31);
        if (n < a.n1 && m < a.n2 && !(a.symmetric && m > n)) return true;
      }
    }
    pr += step;
    if (pr >= a.npairs) return false;
    if (a.symmetric) {
      int64_t r = (int64_t)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
      while ((r + 1) * (r + 2) / 2 <= pr) ++r;
      while (r * (r + 1) / 2 > pr) --r;
      n = r;
      m = pr - r * (r + 1) / 2;
    } else {
      n = pr / a.n2;
      m = pr % a.n2;
    }
    return true;
  }
};

}  // namespace smn_cnn
