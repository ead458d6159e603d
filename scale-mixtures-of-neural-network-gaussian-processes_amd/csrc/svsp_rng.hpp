// svsp_rng.hpp — the counter-based generator of the sparse variational classifier (layout: include/smnngp.h), shared by the
// evaluation head (svsp.hip) and the training head (svsp_train.hip): one variate is a pure function of
// (seed, point, class, draw, df).  Device code only; include inside an anonymous namespace.
#pragma once

// ---------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC'11)
struct U4 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
    c = U4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

constexpr uint32_t kStudentStream = 0x80000000u;   // counter word 3 of the Student-t stream (the normal stream has 0 there)
constexpr int kStudentBlocks = 32;                 // 2 tries per block: 64 tries, (1 - pi/4)^64 = 1e-43 left

template <typename T>
struct Real;
template <>
struct Real<float> {
  // uniform in (0, 1) from the top 23 bits, in (-1, 1) from the top 24: odd multiples of 2^-24 below 1 in magnitude, which
  // fp32 holds exactly, formed by ONE fused multiply-add (integer < 2^24 exact, one rounding that has nothing to round): never
  // 0, never +-1
  static __device__ __forceinline__ float unit(uint32_t a) { return __fmaf_rn((float)(a >> 9), 0x1p-23f, 0x1p-24f); }
  static __device__ __forceinline__ float sym(uint32_t a) { return __fmaf_rn((float)(a >> 8), 0x1p-23f, 0x1p-24f - 1.0f); }
  static __device__ __forceinline__ float exp_(float x) { return expf(x); }
  static __device__ __forceinline__ float log_(float x) { return logf(x); }
  static __device__ __forceinline__ float expm1_(float x) { return expm1f(x); }
  static __device__ __forceinline__ float sqrt_(float x) { return sqrtf(x); }
  static __device__ __forceinline__ void sincos2pi(float rev, float& s, float& c) {   // v_sin / v_cos take revolutions
    s = __builtin_amdgcn_sinf(rev);
    c = __builtin_amdgcn_cosf(rev);
  }
};
template <>
struct Real<double> {
  static __device__ __forceinline__ double unit(uint32_t a) { return ((double)a + 0.5) * 0x1p-32; }
  static __device__ __forceinline__ double sym(uint32_t a) { return ((double)a + 0.5) * 0x1p-31 - 1.0; }
  static __device__ __forceinline__ double exp_(double x) { return exp(x); }
  static __device__ __forceinline__ double log_(double x) { return log(x); }
  static __device__ __forceinline__ double expm1_(double x) { return expm1(x); }
  static __device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
  static __device__ __forceinline__ void sincos2pi(double rev, double& s, double& c) { sincospi(2.0 * rev, &s, &c); }
};

// Box-Muller: two words -> two standard normal variates
template <typename T>
__device__ __forceinline__ void normal_pair(uint32_t a, uint32_t b, T& z0, T& z1) {
  const T r = Real<T>::sqrt_(T(-2) * Real<T>::log_(Real<T>::unit(a)));
  T s, c;
  Real<T>::sincos2pi(Real<T>::unit(b), s, c);
  z0 = r * c;
  z1 = r * s;
}

// Bailey's polar method (Math. Comp. 62, 1994): (u, v) uniform in the unit disc, w = u^2 + v^2:
//   t = u sqrt(df (w^(-2/df) - 1) / w)  ~  Student-t(df).
// A bounded loop: kStudentBlocks blocks of two tries; a variate none of whose 64 tries fell into the disc is 0.
template <typename T>
__device__ __forceinline__ T student_t(uint32_t k0, uint32_t k1, uint32_t draw, uint32_t point, uint32_t cls, T df) {
  T res = T(0);
  bool done = false;
  for (int blk = 0; blk < kStudentBlocks; ++blk) {
    const U4 r = philox4x32_10(U4{draw, point, cls, kStudentStream | (uint32_t)blk}, k0, k1);
    const uint32_t wa[2] = {r.x, r.z}, wb[2] = {r.y, r.w};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const T u = Real<T>::sym(wa[i]), v = Real<T>::sym(wb[i]);
      const T w = fma(u, u, v * v);
      if (!done && w <= T(1) && w > T(0)) {   // (w > 0 always: u, v are never 0)
        res = u * Real<T>::sqrt_(df * Real<T>::expm1_(T(-2) / df * Real<T>::log_(w)) / w);
        done = true;
      }
    }
    if (done) break;
  }
  return res;
}

// The four variates of classes 4 g .. 4 g + 3 of (point, draw).  Classes >= C get 0.
template <typename T>
__device__ __forceinline__ void draw4(uint32_t k0, uint32_t k1, uint32_t draw, uint32_t point, int g, int C, T df, T z[4]) {
  if (df > T(0)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = 4 * g + k < C ? student_t<T>(k0, k1, draw, point, (uint32_t)(4 * g + k), df) : T(0);
  } else {
    const U4 r = philox4x32_10(U4{draw, point, (uint32_t)g, 0u}, k0, k1);
    normal_pair<T>(r.x, r.y, z[0], z[1]);
    normal_pair<T>(r.z, r.w, z[2], z[3]);
  }
}

// Bailey's variate together with its derivative in df at fixed (u, v) (acceptance does not depend on df):
//   t = u sqrt(df e / w),  e = w^(-2/df) - 1 = expm1(-2 ln w / df)
//   dt/ddf = t/2 [1/df + (2 ln w / df^2) (e + 1) / e];  the bracket's second term tends to -1/df as w -> 1 (e -> 0): then t = 0
//   and the product is 0, which the e == 0 branch returns instead of 0/0.
template <typename T>
__device__ __forceinline__ T student_t_ddf(uint32_t k0, uint32_t k1, uint32_t draw, uint32_t point, uint32_t cls, T df, T& dt) {
  T res = T(0);
  dt = T(0);
  bool done = false;
  for (int blk = 0; blk < kStudentBlocks; ++blk) {
    const U4 r = philox4x32_10(U4{draw, point, cls, kStudentStream | (uint32_t)blk}, k0, k1);
    const uint32_t wa[2] = {r.x, r.z}, wb[2] = {r.y, r.w};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const T u = Real<T>::sym(wa[i]), v = Real<T>::sym(wb[i]);
      const T w = fma(u, u, v * v);
      if (!done && w <= T(1) && w > T(0)) {
        const T lw = Real<T>::log_(w);
        const T e = Real<T>::expm1_(T(-2) / df * lw);
        res = u * Real<T>::sqrt_(df * e / w);   // the expression of student_t: the same bits
        dt = e == T(0) ? T(0) : res * T(0.5) * (T(1) / df + (T(2) * lw / (df * df)) * (e + T(1)) / e);
        done = true;
      }
    }
    if (done) break;
  }
  return res;
}
