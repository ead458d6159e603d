// cnn.hip — conv-NNGP kernel of experiments/nt_kernels.py:34-45:
//     L x [Conv(1 ch, 3x3, stride 1, SAME, W_std=w, b_std=b); act];  Flatten;  Dense(last_w, b=0)
// (neural_tangents stax.Conv / Flatten).  Because there is no pooling before
// Flatten only same-pixel covariances are needed: for an image pair (n, m) the state is one H x W map
//     K0[h,w] = sum_c x1[n,h,w,c] x2[m,h,w,c] / C
//     K <- w^2 * (3x3 zero-padded box SUM of K) / 9 + b^2 ;  K <- act(K; q1[n,h,w], q2[m,h,w])   (per pixel)
//     out[n,m] = last_w^2 * mean_hw K
// The N^2 * H * W per-pixel kernel entries can never be materialised (C3: 819 GB in fp64), so each
// wave carries one pair's map through all layers on chip: the map lives in LDS with a zero halo
// (ping-pong between layers), lanes own pixels, the 3x3 stencil is 9 LDS reads.  The per-image
// pre-activation variance maps q~_l[n,h,w] (the same stencil recursion on the diagonal) are computed
// once per image by conv_q_kernel and streamed from L2.  VALU-bound by construction (a 9-tap sum and
// an asin per pixel, pair and layer); no MFMA: there is no GEMM here to find.
// The wave's LDS map, the K0 phase, the activation step, the epilogue, the pair order and the per-image helpers are
// cnn_pairs.hpp's, shared with the tangent, reverse-mode and WideResnet kernels.
#include <type_traits>

#include "cnn_pairs.hpp"
#include "internal.hpp"
#include "nngp_math.hpp"

namespace {

using namespace smn_cnn;

// One workgroup per image: Q[img][l][p] = pre-activation variance of layer l at pixel p,
// diag[img] = last_w^2 * mean_p q_L (the exact K(img, img)).
// R is what the pair kernel multiplies (like the r table of the MLP build); ONE table, because the pair kernel is
// bound by streaming these tables out of L2, not by its arithmetic:
//   ReLU: r = 1/sqrt(q~) (0 where q~ <= 0); the second factor s_i s_j = sqrt(q_i q_j)/(2 pi) = 1/(2 pi r_i r_j)
//   erf:  r = 1/sqrt(1 + 2 q~)
// (A second table s = sqrt(q~ / 2 pi), so that s_i s_j is one multiplication instead of 1 / (2 pi r_i r_j) with a reciprocal, a
// Newton step and a select, was tried in round 3: 6 vector instructions fewer per pixel and layer, but 64 more registers for the
// table vectors of a layer -- 2 waves per SIMD instead of 3 -- and the kernel build went from 572 to 1003 ms.  Not kept.)
// patch44 != 0 (32x32 images, conv_pair44_kernel): R is written in the order that kernel's lanes read it -- for layer l the
// vectors [j = 4-pixel patch row r x vector v][lane = patch (py, px)][16 bytes], so one load instruction of a wave is 1 KB of
// consecutive bytes -- and xperm receives the image in the same order ([vector of a patch row][lane][16 bytes], a patch
// row being 4 pixels x C channels).  Gathered patch rows straight from the [pixel][channel] image cost the pair kernel 44 %
// of its time (6x the cache-line look-ups: profiles/r03_cnn_phase_timing.txt).
template <typename T>
__device__ __forceinline__ int64_t patch44_index(int px, int vec_elems) {   // pixel -> element index inside one layer's table
  const int row = px >> 5, col = px & 31;
  const int lane = (row >> 2) * 8 + (col >> 2), r = row & 3, c = col & 3;
  const int rv = 4 / vec_elems;                                              // vectors per patch row
  return ((int64_t)(r * rv + c / vec_elems) * 64 + lane) * vec_elems + c % vec_elems;
}
template <typename T>
__global__ void __launch_bounds__(256) conv_q_kernel(const T* __restrict__ x, int64_t n, ConvProg p,
                                                     T* __restrict__ R, T* __restrict__ diag, int patch44, T* __restrict__ xperm) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H = p.H, W = p.W, HW = H * W, PW = W + 2, PSZ = (H + 2) * PW;
  double* m0 = reinterpret_cast<double*>(smem);   // padded map, double for the diagonal
  double* m1 = m0 + PSZ;
  const int64_t img = blockIdx.x;
  for (int i = threadIdx.x; i < 2 * PSZ; i += blockDim.x) m0[i] = 0.0;
  __syncthreads();
  q0_into_map(x + img * HW * p.C, HW, W, PW, p.C, m0);
  __syncthreads();
  double* cur = m0;
  double* nxt = m1;
  for (int l = 0; l < p.layers; ++l) {
    for (int px = threadIdx.x; px < HW; px += blockDim.x) {
      const int h = px / W, w = px % W;
      const double qt = p.w2 * box9(cur + h * PW + w, PW) / 9.0 + p.b2;
      const DiagAct d = diag_act(p.act, qt);
      const int64_t ti = (img * p.layers + l) * HW + (patch44 ? patch44_index<T>(px, 16 / (int)sizeof(T)) : (int64_t)px);
      R[ti] = (T)d.ra;
      nxt[(h + 1) * PW + w + 1] = d.qa;
    }
    __syncthreads();
    double* t = cur; cur = nxt; nxt = t;
  }
  if (patch44 && xperm) {
    // element e' = c4 * C + ch of patch row r of lane `lane` lives in vector (r * XV + e' / VEC), slot e' % VEC
    constexpr int VEC = 16 / (int)sizeof(T);
    const int C = p.C, XV = 4 * C / VEC;
    for (int i = threadIdx.x; i < HW * C; i += blockDim.x) {
      const int px = i / C, ch = i % C;
      const int row = px >> 5, col = px & 31;
      const int lane = (row >> 2) * 8 + (col >> 2), r = row & 3, e = (col & 3) * C + ch;
      xperm[img * HW * C + ((int64_t)(r * XV + e / VEC) * 64 + lane) * VEC + e % VEC] = x[img * HW * C + i];
    }
  }
  const double k = block_mean(cur, H, W, PW, p.lw2, m0 + 2 * PSZ);   // 256 doubles of scratch behind the two maps
  if (threadIdx.x == 0) diag[img] = (T)k;
}

constexpr int kMaxPix = 64;   // pixels per lane (H*W <= 4096)

// 4 waves per workgroup, each wave walks its own list of image pairs (PairWalk) with ONE padded map private to it
// (WaveMap) -- half the LDS of a ping-pong pair, twice the waves per CU to cover the latency of the table loads and of
// the f64 chains.  NP = pixels per lane (compile-time bound): padded-map offsets are computed once per kernel, not per layer.
#ifndef SMN_CNN_K0_BATCH
#define SMN_CNN_K0_BATCH 16   // pixels whose K0 channel loads are issued together: the phase is pure load latency
#endif                        // (4 -> 16: fp64 +12 %, fp32 +5 %, profiles/r01f_cnn_k0_batch_ab.txt)
constexpr int KB0 = SMN_CNN_K0_BATCH;
#ifndef SMN_CNN_OCC_F32
#define SMN_CNN_OCC_F32 2   // f32 wants the registers (ILP over its pixels) more than the waves: 4 spills and loses 27 %
#endif
#ifndef SMN_CNN_OCC_F64
#define SMN_CNN_OCC_F64 4   // workgroups per CU the f64 form is compiled for (128 VGPRs, 9 spilled doubles; 2 / 3: -6 %)
#endif

template <typename T>
constexpr int pair_occ(int np, bool exact) {   // workgroups per CU a form is compiled for (and launched at)
  return np > 16 ? 1 : np <= 4 ? 4 : !exact ? 2 : sizeof(T) == 8 ? SMN_CNN_OCC_F64 : SMN_CNN_OCC_F32;
}
template <typename T, int ACT, int NP, bool EXACT>
__global__ void __launch_bounds__(256, pair_occ<T>(NP, EXACT)) conv_pair_kernel(PairArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvProg& p = a.prog;
  const int HW = p.H * p.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  WaveMap<T, NP, EXACT> wm(smem, p.H, p.W, lane, wave);
  auto pix = [&](int i) { return wm.pix(i); };
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / p.C);
  // (the fp64 16-pixel exact form lives on 128 VGPRs: a batch of 16 spills there and costs 20 %)
  constexpr int KB = (sizeof(T) == 8 && EXACT && NP == 16) ? 4 : (KB0 < NP ? KB0 : NP);
  PairWalk<T> walk(a, wave);
  int64_t n, m;
  while (walk.next(n, m)) {
    T val[NP];
    load_k0<KB, true>(a.x1 + n * HW * p.C, a.x2 + m * HW * p.C, p.C, inv_c, pix, val);
    for (int l = 0; l < p.layers; ++l) {
      const T* r1 = a.R1 + (n * p.layers + l) * HW;
      const T* r2 = a.R2 + (m * p.layers + l) * HW;
      wm.publish(val);
#pragma unroll
      for (int i = 0; i < NP; ++i) {   // the taps fused with the activation, not wm.box(): one value per pixel to keep
        const T rr = r1[pix(i)] * r2[pix(i)];
        val[i] = act_value<T, ACT>(fma(w2_9, wm.taps(i, wm.PW), b2), rr);
      }
    }
    T s = T(0);
#pragma unroll
    for (int i = 0; i < NP; ++i) s += wm.own(i) ? val[i] : T(0);
    store_pair(a, n, m, s, HW, lane);
  }
}

// ---------------------------------------------------------------- 32 x 32 images (CIFAR: BASELINE.json's C3)
// The 3x3 box sum without LDS.  Lane l holds column l & 31 of rows 2i + (l >> 5), i = 0..15, so
//   horizontal:  the neighbours of a pixel are the same register of lanes l -+ 1 (DPP wave_shr / wave_shl; the image
//                border columns are masked by a per-lane 0/1 factor folded into the add),
//   vertical:    v_permlane32_swap turns the register of row pair i into E_i = row 2i and O_i = row 2i+1, each in ALL
//                lanes; a lower lane (row 2i) adds O_{i-1} + E_i + O_i, an upper lane (row 2i+1) E_i + O_i + E_{i+1}.
// No map, no halo, no LDS instruction in the layer loop: what is left to wait for are the factor-table loads.
template <typename T>
__device__ __forceinline__ T dpp_lane(T v, bool left);
template <>
__device__ __forceinline__ float dpp_lane<float>(float v, bool left) {
  const int x = __float_as_int(v);
  return __int_as_float(left ? __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false)     // wave_shr:1: lane l-1
                             : __builtin_amdgcn_update_dpp(0, x, 0x130, 0xf, 0xf, false));   // wave_shl:1: lane l+1
}
template <>
__device__ __forceinline__ double dpp_lane<double>(double v, bool left) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  if (left)
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false));
  return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, false));
}
// e = the lower half-wave's values in all lanes, o = the upper half-wave's (scratch/dpp_probe: permlane32_swap(x, x))
__device__ __forceinline__ void rows32(float h, float& e, float& o) {
  const int x = __float_as_int(h);
  const auto p = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  e = __int_as_float((int)p[0]);
  o = __int_as_float((int)p[1]);
}
__device__ __forceinline__ void rows32(double h, double& e, double& o) {
  const int lo = __double2loint(h), hi = __double2hiint(h);
  const auto pl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto ph = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  e = __hiloint2double((int)ph[0], (int)pl[0]);
  o = __hiloint2double((int)ph[1], (int)pl[1]);
}

#ifndef SMN_CNN32_OCC
#define SMN_CNN32_OCC 2
#endif
template <typename T, int ACT>
__global__ void __launch_bounds__(256, SMN_CNN32_OCC) conv_pair32_kernel(PairArgs<T> a) {
  constexpr int NP = 16, HW = 1024, KB = KB0 < NP ? KB0 : NP;
  const ConvProg& p = a.prog;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31;
  const bool upper = lane >= 32;
  const T ml = col > 0 ? T(1) : T(0), mr = col < 31 ? T(1) : T(0);
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / p.C);
  PairWalk<T> walk(a, wave);
  int64_t n, m;
  while (walk.next(n, m)) {
    T val[NP];
    load_k0<KB, true>(a.x1 + n * HW * p.C, a.x2 + m * HW * p.C, p.C, inv_c, [&](int i) { return lane + 64 * i; }, val);
    for (int l = 0; l < p.layers; ++l) {
      const T* r1 = a.R1 + (n * p.layers + l) * HW + lane;
      const T* r2 = a.R2 + (m * p.layers + l) * HW + lane;
      T e[NP], o[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const T h = fma(ml, dpp_lane<T>(val[i], true), fma(mr, dpp_lane<T>(val[i], false), val[i]));
        rows32(h, e[i], o[i]);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const T above = i > 0 ? o[i - 1] : T(0);        // row 2i - 1, for the lower lanes
        const T below = i + 1 < NP ? e[i + 1] : T(0);   // row 2i + 2, for the upper lanes
        const T bs = (e[i] + o[i]) + (upper ? below : above);
        const T rr = r1[64 * i] * r2[64 * i];   // (all 32 loads of the layer issued up front: 5 % slower, registers)
        val[i] = act_value<T, ACT>(fma(w2_9, bs, b2), rr);
      }
    }
    T s = T(0);
#pragma unroll
    for (int i = 0; i < NP; ++i) s += val[i];
    store_pair(a, n, m, s, HW, lane);
  }
}

// conv_pair44_kernel — 32x32 images, one wave per image pair, a 4x4 PATCH of pixels per lane (round 3).
// conv_pair32_kernel keeps one pixel row pair per half-wave and moves every pixel's value to its neighbours (two DPP moves
// and a v_permlane32_swap per pixel and layer, 18 of its 65 vector instructions per pixel and layer, f64:
// profiles/r03_cnn_instruction_budget.txt).  With lane (py, px) = (lane >> 3, lane & 7) holding rows 4 py .. 4 py + 3 x columns
// 4 px .. 4 px + 3, the separable 3 + 3 box sum runs inside the lane's registers: per layer and lane 48 additions for 16 pixels and
// 16 halo values from the four neighbouring lanes, fetched by ds_bpermute_b32 (the LDS crossbar: no LDS memory, no vector-ALU
// instruction).  Border patches multiply their missing halo by a 0 / 1 factor folded into the addition (an fma).  The loads
// are whole 16-byte vectors as well: a patch row is 4 consecutive pixels, so its C channels and its factor-table entries
// are contiguous -- and fully coalesced: conv_q_kernel writes the factor tables and a copy of the images in exactly the order the
// lanes read them ([vector of a patch row][lane][16 bytes]).  One reciprocal step less for 1 / (r_i r_j) (v_rcp_f64 + one Newton
// step: 2^-50, against 2 steps).  (A degree-12 J(c), 1.1e-13 and 5 fused multiply-adds fewer, measured no gain: 579 against 572 ms.)
typedef float cnn_f32x4 __attribute__((ext_vector_type(4)));
typedef double cnn_f64x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ T lane_fetch(T v, int src_lane_bytes);
template <>
__device__ __forceinline__ float lane_fetch<float>(float v, int sb) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(sb, __float_as_int(v)));
}
template <>
__device__ __forceinline__ double lane_fetch<double>(double v, int sb) {
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(sb, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(sb, __double2loint(v)));
}

template <typename T, int ACT, int C>
__global__ void __launch_bounds__(256, SMN_CNN32_OCC) conv_pair44_kernel(PairArgs<T> a) {
  constexpr int HW = 1024, VEC = 16 / sizeof(T);
  constexpr int XV = 4 * C / VEC;          // 16-byte vectors of one patch row of an input image (4 pixels x C channels)
  constexpr int RV = 4 / VEC;              // ... of one patch row of a factor table (4 pixels); 1 (f32: 4 per vector) or 2
  static_assert((4 * C) % VEC == 0 && 4 % VEC == 0, "patch rows are whole 16-byte vectors");
  using vec_t = typename std::conditional<sizeof(T) == 8, cnn_f64x2, cnn_f32x4>::type;
  const ConvProg& p = a.prog;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int py = lane >> 3, px = lane & 7;
  const T ml = px > 0 ? T(1) : T(0), mr = px < 7 ? T(1) : T(0), mt = py > 0 ? T(1) : T(0), mb = py < 7 ? T(1) : T(0);
  const int sl = 4 * (px > 0 ? lane - 1 : lane), sr = 4 * (px < 7 ? lane + 1 : lane);     // ds_bpermute source lanes (x 4 bytes)
  const int st = 4 * (py > 0 ? lane - 8 : lane), sb = 4 * (py < 7 ? lane + 8 : lane);
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / C);
  PairWalk<T> walk(a, wave);
  int64_t n, m;
#ifdef SMN_CNN_TIMING   // wave 0 of workgroup 0: s_memtime cycles per phase, summed over its pairs
  long long tc[4] = {0, 0, 0, 0}, tp = __builtin_readcyclecounter();
  int npair = 0;
#define CT(i) do { const long long n_ = __builtin_readcyclecounter(); tc[i] += n_ - tp; tp = n_; } while (0)
#else
#define CT(i)
#endif
  while (walk.next(n, m)) {
    CT(3);
    const T* xa = a.x1 + n * HW * C + lane * VEC;    // a.x1 / a.x2: the patch-order copies made by conv_q_kernel
    const T* xb = a.x2 + m * HW * C + lane * VEC;
    T val[4][4];
    {
      vec_t va[4][XV], vb[4][XV];            // all loads of the pair's inputs in flight at once
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int v = 0; v < XV; ++v) {
          va[r][v] = *reinterpret_cast<const vec_t*>(xa + (r * XV + v) * 64 * VEC);
          vb[r][v] = *reinterpret_cast<const vec_t*>(xb + (r * XV + v) * 64 * VEC);
        }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          T s = T(0);
#pragma unroll
          for (int ch = 0; ch < C; ++ch) {
            const int e = c * C + ch;
            s = fma(va[r][e / VEC][e % VEC], vb[r][e / VEC][e % VEC], s);
          }
          val[r][c] = s * inv_c;
        }
    }
    asm volatile("" : "+v"(val[0][0]));
    CT(0);
    for (int l = 0; l < p.layers; ++l) {
      const T* r1 = a.R1 + (n * p.layers + l) * HW + lane * VEC;
      const T* r2 = a.R2 + (m * p.layers + l) * HW + lane * VEC;
      vec_t t1[4][RV], t2[4][RV];            // factor tables: requested first, used last
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int v = 0; v < RV; ++v) {
          t1[r][v] = *reinterpret_cast<const vec_t*>(r1 + (r * RV + v) * 64 * VEC);
          t2[r][v] = *reinterpret_cast<const vec_t*>(r2 + (r * RV + v) * 64 * VEC);
        }
      // horizontal 3-sums; the halo columns come from the lanes left and right
      T hl[4], hr[4], h[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hl[r] = lane_fetch<T>(val[r][3], sl);
        hr[r] = lane_fetch<T>(val[r][0], sr);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T s01 = val[r][0] + val[r][1], s23 = val[r][2] + val[r][3];
        h[r][1] = s01 + val[r][2];
        h[r][2] = val[r][1] + s23;
        h[r][0] = fma(ml, hl[r], s01);
        h[r][3] = fma(mr, hr[r], s23);
      }
      // the table products of the 16 pixels, formed once the loads have landed: 8 vectors per table die here
      T rr[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) rr[r][c] = t1[r][c / VEC][c % VEC] * t2[r][c / VEC][c % VEC];
      // vertical 3-sums; the halo rows come from the lanes above and below
      T ht[4], hb[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ht[c] = lane_fetch<T>(h[3][c], st);
        hb[c] = lane_fetch<T>(h[0][c], sb);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const T s01 = h[0][c] + h[1][c], s23 = h[2][c] + h[3][c];
        const T b1 = s01 + h[2][c], b2_ = h[1][c] + s23;
        const T b0 = fma(mt, ht[c], s01), b3 = fma(mb, hb[c], s23);
        T bs[4] = {b0, b1, b2_, b3};
#ifdef SMN_CNN_TIMING
        if (c == 0) { asm volatile("" : "+v"(bs[0])); CT(1); }
#endif
#pragma unroll
        for (int r = 0; r < 4; ++r) val[r][c] = act_value<T, ACT, true>(fma(w2_9, bs[r], b2), rr[r][c]);
      }
    }
    asm volatile("" : "+v"(val[0][0]));
    CT(2);
#ifdef SMN_CNN_TIMING
    ++npair;
#endif
    T s = T(0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) s += val[r][c];
    store_pair(a, n, m, s, HW, lane);
  }
#ifdef SMN_CNN_TIMING
  if (threadIdx.x == 0 && blockIdx.x == 0 && npair > 0)
    printf("conv_pair44 wg0 wave0: %d pairs; cycles per pair: K0 (x loads + products) %lld, box sums of %d layers (incl. waiting for the halo) %lld, activation maps %lld, reduce/store/next %lld\n",
           npair, tc[0] / npair, p.layers, tc[1] / npair, tc[2] / npair, tc[3] / npair);
#endif
#undef CT
}

// Launch one form of the pair kernel, in the tiled pair order where tiled_pair_grid takes it.
template <typename T, typename K>
int launch_pair_form(smn_ctx* ctx, K kern, PairArgs<T> a, int64_t blocks, size_t lds) {
  if (lds > 0)
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  tiled_pair_grid(resident_blocks(ctx, kern, lds), a.npairs, INT64_MAX, &blocks, &a.tile_bn);
  ProfScope ps(ctx, PROF_BUILD, ctx->stream);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, a);
  return SMN_OK;
}

template <typename T, int ACT>
int launch_pairs(smn_ctx* ctx, const PairArgs<T>& a, int64_t blocks, size_t lds, int64_t hw) {
  // register-only stencil, no LDS: fp64 by default (+2 ... +11 % with growing N; the fp32 LDS-map kernel is VALU-bound at
  // 72 % busy and 5 % FASTER than its register form: profiles/r01f_cnn_fast32_ab.txt)
  if (a.prog.H == 32 && a.prog.W == 32 && sizeof(T) == 8) {
    // a 4x4 patch per lane where the patch rows are whole vectors (1 or 3 channels: MNIST- / CIFAR-shaped inputs)
    // (cnn_t made the same choice: the tables and a.x1 / a.x2 are in patch order then)
    if (a.prog.C == 3) return launch_pair_form<T>(ctx, conv_pair44_kernel<T, ACT, 3>, a, blocks, 0);
    if (a.prog.C == 1) return launch_pair_form<T>(ctx, conv_pair44_kernel<T, ACT, 1>, a, blocks, 0);
    return launch_pair_form<T>(ctx, conv_pair32_kernel<T, ACT>, a, blocks, 0);
  }
#define PAIR_CASE(NP)                                                                                         \
  if (hw <= 64 * NP) {                                                                                        \
    if (hw == 64 * NP && 64 % a.prog.W == 0)                                                                  \
      return launch_pair_form<T>(ctx, conv_pair_kernel<T, ACT, NP, true>, a, blocks, lds);                    \
    return launch_pair_form<T>(ctx, conv_pair_kernel<T, ACT, NP, false>, a, blocks, lds);                     \
  }
  PAIR_CASE(4)
  PAIR_CASE(16)
  PAIR_CASE(kMaxPix)
#undef PAIR_CASE
  return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_cnn: H*W > %d", 64 * kMaxPix);
}

// THE launch of the per-image pass.  No profiling scope and no launch check of its own: the callers bracket one or two of them.
template <typename T>
int launch_conv_q(smn_ctx* ctx, const ConvProg& p, const void* x, int64_t n, T* R, T* diag, bool patch44, T* xperm) {
  const size_t lds_q = conv_q_lds_bytes(p.H, p.W);
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(conv_q_kernel<T>), lds_q));
  hipLaunchKernelGGL(conv_q_kernel<T>, dim3((unsigned)n), dim3(256), lds_q, ctx->stream, static_cast<const T*>(x), n, p, R, diag,
                     patch44 ? 1 : 0, patch44 ? xperm : static_cast<T*>(nullptr));
  return SMN_OK;
}

template <typename T>
int cnn_t(smn_ctx* ctx, int act, int layers, double w, double b, double lw, const void* x1, int64_t n1,
          const void* x2, int64_t n2, int64_t H, int64_t W, int64_t C, int fill, void* out, int64_t ldk) {
  const bool sym = x2 == nullptr;
  if (sym) n2 = n1;
  const ConvProg p = make_prog(act, layers, H, W, C, w, b, lw);
  const int64_t HW = H * W;
  const size_t lds_p = wave_map_lds_bytes<T>(H, W);
  if (conv_q_lds_bytes(H, W) > 160 * 1024 || lds_p > 160 * 1024)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_cnn: image %lldx%lld too large for the on-chip pair map", (long long)H, (long long)W);
  // tables: R1 [n1][L][HW], diag1 [n1] (+ R2, diag2); patch order + patch-order copies of the inputs for conv_pair44_kernel
  const bool patch44 = H == 32 && W == 32 && (C == 1 || C == 3) && sizeof(T) == 8;
  const size_t qn1 = (size_t)n1 * (size_t)(layers > 0 ? layers : 1) * HW, qn2 = sym ? 0 : (size_t)n2 * (size_t)(layers > 0 ? layers : 1) * HW;
  const size_t xn1 = patch44 ? (size_t)n1 * HW * C : 0, xn2 = (patch44 && !sym) ? (size_t)n2 * HW * C : 0;
  void* tv = nullptr;
  SMN_TRY(smn_workspace(ctx, 1, sizeof(T) * (qn1 + qn2 + (size_t)n1 + (size_t)n2 + xn1 + xn2) + 64, &tv));
  T* R1 = static_cast<T*>(tv);
  T* R2 = sym ? R1 : R1 + qn1;
  T* d1 = R1 + qn1 + qn2;
  T* d2 = d1 + n1;
  T* xp1 = reinterpret_cast<T*>((reinterpret_cast<uintptr_t>(d2 + n2) + 15) & ~(uintptr_t)15);   // 16-byte aligned
  T* xp2 = sym ? xp1 : xp1 + xn1;
  {
    ProfScope ps(ctx, PROF_PREP, ctx->stream);
    SMN_TRY(launch_conv_q<T>(ctx, p, x1, n1, R1, d1, patch44, xp1));
    if (!sym) SMN_TRY(launch_conv_q<T>(ctx, p, x2, n2, R2, d2, patch44, xp2));
  }
  SMN_CHECK_LAUNCH(ctx);
  PairArgs<T> a;
  a.x1 = static_cast<const T*>(x1); a.x2 = sym ? a.x1 : static_cast<const T*>(x2);
  if (patch44) { a.x1 = xp1; a.x2 = xp2; }
  a.R1 = R1; a.R2 = R2; a.diag = d1; a.n1 = n1; a.n2 = n2;
  a.symmetric = sym ? 1 : 0; a.mirror = (sym && fill == SMN_FILL_FULL) ? 1 : 0;
  a.prog = p; a.out = static_cast<T*>(out); a.ldo = ldk;
  a.npairs = sym ? n1 * (n1 + 1) / 2 : n1 * n2;
  int64_t blocks = (a.npairs + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;   // persistent-ish: waves stride over the pair list
  a.tile_bn = 0;
  SMN_TRY(act == SMN_ACT_RELU ? (launch_pairs<T, 0>(ctx, a, blocks, lds_p, HW)) : (launch_pairs<T, 1>(ctx, a, blocks, lds_p, HW)));
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

template <typename T>
int cnn_diag_t(smn_ctx* ctx, int act, int layers, double w, double b, double lw, const void* x, int64_t n, int64_t H, int64_t W,
               int64_t C, void* diag) {
  const ConvProg p = make_prog(act, layers, H, W, C, w, b, lw);
  if (conv_q_lds_bytes(H, W) > 160 * 1024)
    return smn_fail(ctx, SMN_ENOTSUP, "smn_kernel_conv_diag: image %lldx%lld too large for the on-chip map", (long long)H, (long long)W);
  void* tv = nullptr;   // the factor tables the pass writes beside the diagonal: scratch here
  SMN_TRY(smn_workspace(ctx, 1, sizeof(T) * (size_t)n * (size_t)(layers > 0 ? layers : 1) * (size_t)(H * W) + 64, &tv));
  return cnn_tables(ctx, sizeof(T) == 8 ? SMN_F64 : SMN_F32, p, x, n, tv, diag);
}

}  // namespace

int cnn_tables(smn_ctx* ctx, int dtype, const smn_cnn::ConvProg& p, const void* x_d, int64_t n, void* r_d, void* diag_d) {
  return by_dtype(dtype, [&](auto e) {
    using T = decltype(e);
    {
      ProfScope ps(ctx, PROF_PREP, ctx->stream);
      SMN_TRY(launch_conv_q<T>(ctx, p, x_d, n, static_cast<T*>(r_d), static_cast<T*>(diag_d), false, static_cast<T*>(nullptr)));
    }
    SMN_CHECK_LAUNCH(ctx);
    return (int)SMN_OK;
  });
}

int cnn_diag(smn_ctx* ctx, int dtype, int act, int layers, double w, double b, double lw, const void* x_d, int64_t n,
             int64_t H, int64_t W, int64_t C, void* diag_d) {
  SMN_TRY(conv_check(ctx, "smn_kernel_conv_diag", dtype, act, layers, n, H, W, C, 64 * kMaxPix));
  return by_dtype(dtype, [&](auto e) {
    return cnn_diag_t<decltype(e)>(ctx, act, layers, w, b, lw, x_d, n, H, W, C, diag_d);
  });
}

extern "C" int smn_kernel_cnn(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                              double last_w_std, const void* x1_d, int64_t n1, const void* x2_d, int64_t n2, int64_t H,
                              int64_t W, int64_t C, int fill, void* nngp_d, int64_t ldk) {
  if (!ctx || !x1_d || !nngp_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(conv_check(ctx, "smn_kernel_cnn", dtype, act, num_hiddens, n1, H, W, C, 64 * kMaxPix));
  if (x2_d && n2 <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_kernel_cnn: bad sizes");
  if (x2_d) SMN_CHECK_LD(ctx, "smn_kernel_cnn", ldk, n2);
  else SMN_CHECK_LD(ctx, "smn_kernel_cnn", ldk, n1);
  return by_dtype(dtype, [&](auto e) {
    return cnn_t<decltype(e)>(ctx, act, num_hiddens, w_std, b_std, last_w_std, x1_d, n1, x2_d, n2, H, W, C, fill, nngp_d, ldk);
  });
}
