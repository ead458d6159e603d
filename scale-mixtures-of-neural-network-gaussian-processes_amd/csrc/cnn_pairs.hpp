// cnn_pairs.hpp — what the conv-NNGP kernels share (cnn.hip: the forward build, cnn_resnet.hip: the WideResnet, cnn_grad.hip:
// forward-mode tangents, cnn_input_grad.hip: reverse mode for the input images).
//   device, pair kernels:  rsqrt_any / rcp_any / rcp_fast;  ConvProg, PairArgs and PairWalk (the layer program, the launch
//                          arguments and the order in which the waves walk the image pairs; tri_decode);  WaveMap (a wave's
//                          private padded LDS map and its 3x3 box sum);  load_k0 (the K0 phase);  act_value / act_factors (the
//                          activation step of a pair, value only or with its two derivative factors);  store_pair (epilogue)
//   device, per image:     q0_into_map, box9, diag_act, block_mean
//   host:                  make_prog, conv_check, wave_map_lds_bytes, resident_blocks, tiled_pair_grid
#pragma once
#include <cstdint>

#include "internal.hpp"
#include "nngp_math.hpp"

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
__device__ __forceinline__ float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double rcp_fast(double x) {   // v_rcp_f64 + one Newton step: 2^-50
  const double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}

struct ConvProg {
  int act, layers, H, W, C;
  double w2, b2, lw2;
};
inline ConvProg make_prog(int act, int layers, int64_t H, int64_t W, int64_t C, double w_std, double b_std, double last_w_std) {
  return ConvProg{act, layers, (int)H, (int)W, (int)C, w_std * w_std, b_std * b_std, last_w_std * last_w_std};
}

template <typename T>
struct PairArgs {
  const T* x1; const T* x2; const T* R1; const T* R2; const T* diag;
  int64_t n1, n2; int symmetric, mirror;
  ConvProg prog;
  T* out; int64_t ldo; int64_t npairs;
  int tile_bn;   // > 0: XCD-tiled pair order (below), tiles of tile_bn x 32 image pairs; 0: plain strided order
};

// Pair number pr of the lower triangle, row by row: pr = n (n + 1) / 2 + m, m <= n.
__device__ __forceinline__ void tri_decode(int64_t pr, int64_t& n, int64_t& m) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= pr) ++r;
  while (r * (r + 1) / 2 > pr) --r;
  n = r;
  m = pr - r * (r + 1) / 2;
}

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
      tri_decode(pr, n, m);
    } else {
      n = pr / a.n2;
      m = pr % a.n2;
    }
    return true;
  }
};

// ---------------------------------------------------------------- a wave's padded LDS map
// 4 waves per workgroup, each with ONE padded (H + 2) x (W + 2) map of its own in dynamic LDS, zero halo.  A lane keeps the
// values of its NP pixels (pixel lane + 64 i) in registers, publishes them to the map, reads the nine taps of each of its
// pixels and overwrites the registers.  LDS operations of one wave execute in order, so a box sum needs no workgroup barrier
// (only a compiler fence), and the next publish may follow the tap reads directly: no second map.
// Lanes whose pixel index runs past H*W are not branched around: they load from a clamped (valid) pixel and publish to a dummy
// slot in a row of its own below the map: its neighbourhood is the map's bottom halo row (read only, always zero),
// [PSZ, PSZ + 2] and [PSZ + PW, PSZ + PW + 2]; no pixel of the image reads at or past PSZ.  own(i) tells them apart.
// EXACT (H*W == 64 NP and W divides 64): there are none, pixel i sits 64 / W rows below pixel i - 1, the offsets are
// off0 + i * rstep and no per-pixel table is kept in registers.
// box() is the tangent and reverse kernels', which carry more state than the forward kernel:
//   * the row stride is re-read as an opaque scalar per box sum: left loop-invariant, the compiler keeps three row addresses per
//     owned pixel alive across the whole layer loop (48 registers for 16 pixels) and spills the state instead;
//   * the tap reads are fenced off in groups of four pixels (36 taps in flight, not 144).
// The forward kernel fuses its taps with the activation (publish() + taps()) and needs neither.
// Which kernel uses which of these, and of the two re-reads below, follows the compiler's figures
// (profiles/r11_cnn_shared.txt), not tidiness.
inline size_t wave_map_elems(int64_t H, int64_t W) { return (size_t)(H + 2) * (W + 2) + (size_t)(W + 2) + 3; }
template <typename T>
inline size_t wave_map_lds_bytes(int64_t H, int64_t W) { return 4 * wave_map_elems(H, W) * sizeof(T); }

template <typename T, int NP, bool EXACT>
struct WaveMap {
  T* map;
  int HW, PW, lane, vlane, off0, rstep;
  int off_tab[EXACT ? 1 : NP];   // centre of pixel lane + 64 i in the padded map
  __device__ __forceinline__ WaveMap(char* smem, int H, int W, int lane_, int wave) {
    PW = W + 2;
    HW = H * W;
    lane = vlane = lane_;
    const int PSZ = (H + 2) * PW, MSZ = PSZ + PW + 3;   // wave_map_elems
    map = reinterpret_cast<T*>(smem) + (size_t)wave * MSZ;
    for (int i = lane; i < MSZ; i += 64) map[i] = T(0);   // halo stays zero for the whole kernel
    off0 = (lane / W + 1) * PW + lane % W + 1;
    rstep = (64 / W) * PW;
    if (!EXACT) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int px = lane + 64 * i;
        off_tab[i] = px < HW ? (px / W + 1) * PW + px % W + 1 : PSZ + 1;   // pixels past the image: the dummy slot
      }
    }
  }
  __device__ __forceinline__ int off(int i) const { return EXACT ? off0 + i * rstep : off_tab[EXACT ? 0 : i]; }
  __device__ __forceinline__ int pix(int i) const { return EXACT ? vlane + 64 * i : min(vlane + 64 * i, HW - 1); }   // pixel a lane loads from
  __device__ __forceinline__ bool own(int i) const { return EXACT || lane + 64 * i < HW; }
  // The lane and off0 re-read as opaque values (the tangent kernel: the lane once per pair, off0 before every box sum): the
  // per-pixel addresses derived from them are then recomputed where they are used (an integer add each) instead of staying
  // alive, about a hundred registers for 16 pixels, beside the state for the whole kernel.
  __device__ __forceinline__ void reread_lane() { asm volatile("" : "+v"(vlane)); }
  __device__ __forceinline__ void reread_off0() { asm volatile("" : "+v"(off0)); }
  // this layer's input into the map; the previous layer's tap reads were issued before (in-order LDS of one wave)
  __device__ __forceinline__ void publish(const T (&v)[NP]) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < NP; ++i) map[off(i)] = v[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // the nine taps of pixel i, row stride pw
  __device__ __forceinline__ T taps(int i, int pw) const {
    const T* r1 = map + off(i) - 1;   // left neighbour; the rows above and below are one add each, the taps immediates
    const T* r0 = r1 - pw;
    const T* r2 = r1 + pw;
    return ((r0[0] + r0[1]) + (r0[2] + r1[0])) + ((r1[1] + r1[2]) + (r2[0] + r2[1])) + r2[2];
  }
  // v <- 3x3 box sum of v
  __device__ __forceinline__ void box(T (&v)[NP]) {
    publish(v);
    int pw = PW;
    asm volatile("" : "+s"(pw));
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      v[i] = taps(i, pw);
      if (NP > 4 && (i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
};

// K0 of a pair, k[i] = x_a[pix(i)] . x_b[pix(i)] / C: channel loop outside, pixel loop inside, so the 2 KB loads of a batch of
// one channel are in flight together (the phase is pure load latency).  SCHED: the batches are kept apart.
template <int KB, bool SCHED, typename T, int NP, typename Pix>
__device__ __forceinline__ void load_k0(const T* xa, const T* xb, int C, T inv_c, Pix pix, T (&k)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) k[i] = T(0);
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int i0 = 0; i0 < NP; i0 += KB) {
      T va[KB], vb[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        va[j] = xa[pix(i0 + j) * C + c];
        vb[j] = xb[pix(i0 + j) * C + c];
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) k[i0 + j] = fma(va[j], vb[j], k[i0 + j]);
      if (SCHED) __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) k[i] *= inv_c;
}

// Activation step of a pair at one pixel: kt = the pre-activation covariance, rr = r_n r_m of the per-image factor tables
// (ReLU: 1 / sqrt(q_n q_m), 0 where a variance is 0; erf: 1 / sqrt((1 + 2 q_n)(1 + 2 q_m))).  FAST_RCP: one Newton step.
template <typename T, int ACT, bool FAST_RCP = false>
__device__ __forceinline__ T act_value(T kt, T rr) {
  if (ACT == 0) {
    const T ss = rr > T(0) ? T(1.0 / (2.0 * nngp::kPi)) * (FAST_RCP ? rcp_fast(rr) : rcp_any<T>(rr)) : T(0);
    return nngp::relu_map<T, false>(kt, rr, ss).k;
  }
  return nngp::erf_map<T, false>(kt, rr, T(0)).k;
}
// ... with its derivatives: k = the value, dA = d k / d kt, tq = the pair factor of the variance-side terms (cnn_grad.hip:
// d k / d q_i = tq ra_i^2).
template <typename T, int ACT>
__device__ __forceinline__ void act_factors(T kt, T rr, T& k, T& dA, T& tq) {
  if (ACT == 0) {
    const T c = nngp::clamp1(kt * rr);
    const T ca = fabs(c);
    const T as = nngp::asin_abs(ca, c * c);
    const T s1 = nngp::fast_sqrt((T(1) - ca) * (T(1) + ca));
    const T pm = T(nngp::kPi / 2) + copysign(as, c);
    const T sp = rr > T(0) ? rcp_any<T>(rr) : T(0);           // sqrt(q_n q_m)
    dA = pm * T(1.0 / (2.0 * nngp::kPi));
    tq = s1 * sp * T(1.0 / (4.0 * nngp::kPi));
    k = sp * fma(pm, c, s1) * T(1.0 / (2.0 * nngp::kPi));
  } else {
    const T sv = nngp::clamp1(T(2) * kt * rr);
    const T sa = fabs(sv);
    const T as = nngp::asin_abs(sa, sv * sv);
    const T rden = nngp::fast_rsqrt(fmax((T(1) - sa) * (T(1) + sa), sizeof(T) == 8 ? T(1e-300) : T(1e-30)));
    dA = T(4.0 / nngp::kPi) * rr * rden;
    tq = T(-2.0 / nngp::kPi) * sv * rden;
    k = T(2.0 / nngp::kPi) * copysign(as, sv);
  }
}

// Flatten (mean over the hw pixels) + last Dense of pair (n, m) from the lanes' partial sums; the exact diagonal; the mirror.
template <typename Args, typename T>
__device__ __forceinline__ void store_pair(const Args& a, int64_t n, int64_t m, T s, int hw, int lane) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) {
    T v = (T)a.prog.lw2 * s / (T)hw;
    if (a.symmetric && n == m) v = a.diag[n];
    a.out[n * a.ldo + m] = v;
    if (a.symmetric && a.mirror && n != m) a.out[m * a.ldo + n] = v;
  }
}

// ---------------------------------------------------------------- per image (one workgroup, fp64 padded maps, zero halo)
// map[centre of p] = |x[p]|^2 / C
template <typename T>
__device__ __forceinline__ void q0_into_map(const T* __restrict__ x_img, int HW, int W, int PW, int C, double* map) {
  for (int px = threadIdx.x; px < HW; px += blockDim.x) {
    const T* xp = x_img + (int64_t)px * C;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)xp[c] * (double)xp[c];
    map[(px / W + 1) * PW + px % W + 1] = s / C;
  }
}
// 3x3 window sum; c = the top-left of the window in the padded map
__device__ __forceinline__ double box9(const double* c, int PW) {
  return c[0] + c[1] + c[2] + c[PW] + c[PW + 1] + c[PW + 2] + c[2 * PW] + c[2 * PW + 1] + c[2 * PW + 2];
}
// The activation on the diagonal at pre-activation variance qt: ra = the pair kernels' table entry (ReLU: 1/sqrt(qt), 0 where
// qt <= 0; erf: 1/sqrt(1 + 2 qt)), qa = the variance after the activation, dq = d qa / d qt.
struct DiagAct { double ra, qa, dq; };
__device__ __forceinline__ DiagAct diag_act(int act, double qt) {
  DiagAct o;
  if (act == 0) {
    o.ra = qt > 0.0 ? 1.0 / sqrt(qt) : 0.0;
    o.qa = 0.5 * qt;
    o.dq = 0.5;
  } else {
    const double t = 1.0 + 2.0 * qt;
    o.ra = 1.0 / sqrt(t);
    o.qa = (2.0 / nngp::kPi) * asin(2.0 * qt / t);
    o.dq = (4.0 / nngp::kPi) / (t * sqrt(1.0 + 4.0 * qt));   // d/dq (2/pi) asin(2q / (1 + 2q))
  }
  return o;
}
// scale * (mean of the map's h x w pixels): tree reduction of a 256-thread workgroup in red[256]
__device__ __forceinline__ double block_mean(const double* map, int h, int w, int PW, double scale, double* red) {
  double s = 0.0;
  for (int px = threadIdx.x; px < h * w; px += 256) s += map[(px / w + 1) * PW + px % w + 1];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return scale * red[0] / (h * w);
}

// ---------------------------------------------------------------- host
// The argument checks the conv entry points share; max_pixels = the largest image of the caller's pair kernel.
inline int conv_check(smn_ctx* ctx, const char* who, int dtype, int act, int layers, int64_t n, int64_t H, int64_t W, int64_t C,
                      int max_pixels) {
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "%s: bad dtype %d", who, dtype);
  if (act != SMN_ACT_RELU && act != SMN_ACT_ERF) return smn_fail(ctx, SMN_EINVAL, "%s: Unsupported act %d", who, act);
  if (n <= 0 || H <= 0 || W <= 0 || C <= 0 || layers < 0) return smn_fail(ctx, SMN_EINVAL, "%s: bad sizes", who);
  if (H * W > max_pixels)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: H*W = %lld > %d pixels", who, (long long)(H * W), max_pixels);
  return SMN_OK;
}

// Workgroups of 256 threads of `kern` the device holds at once (0: the query failed).
template <typename K>
int64_t resident_blocks(smn_ctx* ctx, K kern, size_t lds) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu <= 0) return 0;
  return (int64_t)ctx->num_cu * per_cu;
}

// Pair order (PairWalk).  Every pair streams two images' inputs and factor tables (56 KB in f64 for 32x32x3, 4 layers); in the
// plain order the waves in flight touch ~8k different images, far beyond the 4 MB L2 of an XCD, and the f64 kernel spent 75 % of
// its wave cycles waiting on those loads (VALU busy 49 %, rocprofv3 PMC).  Tiled order: the grid is exactly the resident
// set (a multiple of 64 workgroups, so a tile is a whole number of 32-pair rows), workgroup b runs on XCD b % 8 (round-robin
// dispatch), and the workgroups of one XCD walk tiles of tile_bn x 32 pairs together -- one pair per wave per tile -- so an
// XCD's L2 holds the tile_bn + 32 images its waves are reading.  Taken once there are >= 64 tiles per XCD, i.e. from 256 pairs
// per resident workgroup on, and the grid fits max_blocks; *blocks and *tile_bn are left alone otherwise.
inline void tiled_pair_grid(int64_t resident, int64_t npairs, int64_t max_blocks, int64_t* blocks, int* tile_bn) {
  const int64_t g = resident / 64 * 64;
  if (g >= 64 && g <= max_blocks && npairs >= 64 * 8 * (g / 8) * 4) {
    *blocks = g;
    *tile_bn = (int)(g / 64);
  }
}

}  // namespace smn_cnn

// Dynamic LDS of the per-image pass (cnn.hip conv_q_kernel): two padded fp64 maps and the 256 doubles of its reduction.
inline size_t conv_q_lds_bytes(int64_t H, int64_t W) { return (2 * (size_t)(H + 2) * (size_t)(W + 2) + 256) * sizeof(double); }
// The per-image pass of smn_kernel_cnn alone (cnn.hip conv_q_kernel, plain pixel order): r_d [n][layers][H W] = the factor
// tables the pair kernels multiply, diag_d [n] = K(x_i, x_i) of the Flatten kernel; both of `dtype`.  The caller has checked
// that conv_q_lds_bytes(H, W) fits the LDS.  smn_kernel_conv_diag (kind 0) is this call; cnn_pool.hip reads the same tables.
int cnn_tables(smn_ctx* ctx, int dtype, const smn_cnn::ConvProg& p, const void* x_d, int64_t n, void* r_d, void* diag_d);
