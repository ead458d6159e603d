// draws.hip — joint posterior function draws of the exact models (SPR / MultiSPR.sample_posterior):
//   smn_rng_chi2     the chi-square mixing variates, one per draw (counter layout: include/smnngp.h)
//   smn_mvn_draws    out[s,t,c] = mean[t,c] + r_s sum_{k<=t} L[t,k] xi[k,c,s]  from a finished lower factor L
//
// The product is the hot path: out[(c,s), t] = sum_k Z[(c,s), k] L[t, k] is an NT product on the MFMA tile engine of
// gemm_nt.hpp (its LDS image, fragment reads and accumulator map), but its A operand Z [C S, T] never exists in memory: every
// K-step's A tile is generated straight into the LDS image, one Philox block + two Box-Muller pairs per (draw, point) giving
// the four classes 4g .. 4g+3 the counter layout ties together.  Rows of the product are therefore ordered
//   m = (g S + s) 4 + j,  class c = 4g + j
// so that one block fills four adjacent rows; the rows of classes >= C (C not a multiple of 4) are computed and not stored.
// A column tile of 128 points t0 .. t0+127 only runs the K-steps up to its last row (triangular work); inside them L is read
// through a mask k <= t < T, so the strict upper triangle of l_d is never touched and no alignment is asked of it.
// The order of the sum over k is the tile engine's and depends on T alone; nothing is accumulated across workgroups.
#include <cmath>

#include "gemm_nt.hpp"
#include "internal.hpp"

namespace {

#include "svsp_rng.hpp"

constexpr uint32_t kChi2Stream = 0xC0000000u;   // counter word 3 of the chi-square stream (normal: 0, Student-t: 0x80000000 | k)
constexpr int kChi2Tries = 32;

// chi2(df) = 2 Gamma(df / 2) by Marsaglia & Tsang (ACM TOMS 26, 2000), one Philox block per try: (r0, r1) -> the normal
// variate (Box-Muller, cos branch), r2 -> the acceptance uniform, r3 -> the boost uniform of a shape below 1.
__device__ double chi2_variate(uint32_t k0, uint32_t k1, uint32_t s, double df) {
  const double a = 0.5 * df;
  const bool boost = a < 1.0;
  const double d = (boost ? a + 1.0 : a) - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double res = df;   // no try accepted (probability below 1e-40)
  for (int k = 0; k < kChi2Tries; ++k) {
    const U4 r = philox4x32_10(U4{s, 0u, 0u, kChi2Stream | (uint32_t)k}, k0, k1);
    double x, unused;
    normal_pair<double>(r.x, r.y, x, unused);
    const double t = 1.0 + c * x;
    if (t > 0.0) {
      const double v = t * t * t;
      if (log(Real<double>::unit(r.z)) < 0.5 * x * x + d - d * v + d * log(v)) {
        res = 2.0 * d * v;
        if (boost) res *= pow(Real<double>::unit(r.w), 1.0 / a);
        break;
      }
    }
  }
  return res;
}

__global__ void __launch_bounds__(256) chi2_kernel(uint32_t k0, uint32_t k1, double df, int64_t S, double* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < S) out[s] = chi2_variate(k0, k1, (uint32_t)s, df);
}

// r_s = sqrt(shape df / g_s), formed in fp64 and rounded to T once
template <typename T>
__global__ void __launch_bounds__(256) draw_scale_kernel(uint32_t k0, uint32_t k1, double df, double shape, int64_t S,
                                                         const double* __restrict__ mix, T* __restrict__ r) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double g = mix ? mix[s] : chi2_variate(k0, k1, (uint32_t)s, df);
  r[s] = (T)sqrt(shape * df / g);
}

template <typename T>
using DrawTile = TileNT<T, 128, 128, 2>;

template <typename T>
struct DrawArgs {
  const T* mean; const T* l; const T* noise; const T* r; T* out;
  int64_t ldl, Tn, S, M;   // M = 4 ceil(C / 4) S rows of the product
  int C;
  uint32_t k0, k1, point0;
  int l_vec;               // l_d and ldl allow 16-byte loads
};

template <typename T, bool GIVEN>
__global__ void __launch_bounds__(256) mvn_draws_kernel(DrawArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Tile = DrawTile<T>;
  using M = typename Tile::M;
  using vec_t = typename Tile::vec_t;
  constexpr int BK = M::BK, VEC = M::VEC, ROWB = Tile::ROWB;
  static_assert(Tile::BM == 128 && Tile::BN == 128, "the fill below is written for 256 threads over 128 x 128");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t Tn = a.Tn, S = a.S;
  const int64_t m0 = (int64_t)blockIdx.x * Tile::BM;
  const int64_t t0 = (int64_t)(gridDim.y - 1 - blockIdx.y) * Tile::BN;   // the longest K-loops start first
  const int64_t kend = Tn < t0 + Tile::BN ? Tn : t0 + Tile::BN;          // one past the last column any row of this tile reads
  const int nk = (int)((kend + BK - 1) / BK);

  // A: thread = (row quad, 16-byte chunk): rows 4 quad .. 4 quad + 3 are the classes 4g .. 4g+3 of draw s
  const int quad = tid >> 3, chunk = tid & 7;
  const int64_t mq = m0 + 4 * quad;
  const bool qvalid = mq < a.M;
  const int64_t gs = mq >> 2;
  const int g = qvalid ? (int)(gs / S) : 0;
  const int64_t s = qvalid ? gs - (int64_t)g * S : 0;
  int apos[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = 4 * quad + j;
    apos[j] = row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4);
  }
  // B: thread = (row of 32, chunk), four rows 32 apart: the staging map of TileNT::mainloop
  const int lrow = tid >> 3;
  const int bpos = Tile::A_BYTES + lrow * ROWB + ((chunk ^ ((lrow >> 1) & 7)) << 4);

  auto fill = [&](char* stage, int kt) {
    const int64_t kb = (int64_t)kt * BK + chunk * VEC;   // first k of this thread's chunk
    vec_t va[4];
    if (!qvalid) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) va[j][e] = T(0);
    } else if (GIVEN) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          va[j][e] = (4 * g + j < a.C && kb + e < Tn) ? a.noise[((kb + e) * a.C + 4 * g + j) * S + s] : T(0);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        T z[4];
        // (points past T - 1 meet zeros of L; their index may wrap, their variates are finite all the same)
        draw4<T>(a.k0, a.k1, (uint32_t)s, a.point0 + (uint32_t)(kb + e), g, a.C, T(0), z);
#pragma unroll
        for (int j = 0; j < 4; ++j) va[j][e] = z[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<vec_t*>(stage + apos[j]) = va[j];

    // whole K-step at or below the diagonal of every row, all rows inside the matrix, aligned: 16-byte loads
    const bool interior = a.l_vec && (int64_t)kt * BK + BK - 1 <= t0 && t0 + Tile::BN <= Tn;
#pragma unroll
    for (int p = 0; p < Tile::PB; ++p) {
      const int64_t t = t0 + lrow + 32 * p;
      vec_t vb;
      if (interior) {
        vb = *reinterpret_cast<const vec_t*>(a.l + t * a.ldl + kb);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) vb[e] = (t < Tn && kb + e <= t) ? a.l[t * a.ldl + kb + e] : T(0);
      }
      *reinterpret_cast<vec_t*>(stage + bpos + 32 * p * ROWB) = vb;
    }
  };

  Tile tile;
  tile.zero();
  fill(smem, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    // the other stage was last read in step kt - 1, which ended with a barrier
    if (kt + 1 < nk) fill(smem + ((kt + 1) & 1) * Tile::STAGE, kt + 1);
    tile.compute(smem + (kt & 1) * Tile::STAGE, lane, wr, wc);
    __syncthreads();
  }

  tile.for_each([&](int m, int n, int i, int lr, int lc) {
    const int64_t mm = m0 + lr, t = t0 + lc;
    if (mm >= a.M || t >= Tn) return;
    const int64_t q = mm >> 2;
    const int64_t gg = q / S, ss = q - gg * S;
    const int c = 4 * (int)gg + (int)(mm & 3);
    if (c >= a.C) return;
    const T v = tile.acc[m][n][i];
    const T mu = a.mean[t * a.C + c];
    a.out[(ss * Tn + t) * a.C + c] = a.r ? fma(a.r[ss], v, mu) : mu + v;
  });
}

template <typename T>
int mvn_draws_t(smn_ctx* ctx, const void* mean, const void* l, int64_t ldl, int64_t Tn, int C, int64_t S, double df, double shape,
                uint64_t seed, int64_t point0, const void* noise, const void* mix, void* out) {
  using Tile = DrawTile<T>;
  hipStream_t st = ctx->stream;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  DrawArgs<T> a;
  a.mean = static_cast<const T*>(mean); a.l = static_cast<const T*>(l); a.noise = static_cast<const T*>(noise);
  a.r = nullptr; a.out = static_cast<T*>(out);
  a.ldl = ldl; a.Tn = Tn; a.S = S; a.M = 4 * (int64_t)((C + 3) / 4) * S;
  a.C = C; a.k0 = k0; a.k1 = k1; a.point0 = (uint32_t)point0;
  a.l_vec = (reinterpret_cast<uintptr_t>(l) % 16 == 0 && (ldl * sizeof(T)) % 16 == 0) ? 1 : 0;
  const int64_t mt = (a.M + Tile::BM - 1) / Tile::BM, nt = (Tn + Tile::BN - 1) / Tile::BN;
  if (mt > 0x7fffffff || nt > 65535)
    return smn_fail(ctx, SMN_EINVAL, "smn_mvn_draws: %lld x %lld tiles do not fit one launch", (long long)mt, (long long)nt);
  if (df > 0.0) {
    void* wv = nullptr;
    SMN_TRY(smn_workspace(ctx, 11, sizeof(T) * (size_t)S, &wv));
    hipLaunchKernelGGL(draw_scale_kernel<T>, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, k0, k1, df, shape, S,
                       static_cast<const double*>(mix), static_cast<T*>(wv));
    SMN_CHECK_LAUNCH(ctx);
    a.r = static_cast<const T*>(wv);
  }
  const dim3 grid((unsigned)mt, (unsigned)nt);
  if (noise) {
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(mvn_draws_kernel<T, true>), Tile::LDS_BYTES));
    hipLaunchKernelGGL((mvn_draws_kernel<T, true>), grid, dim3(256), Tile::LDS_BYTES, st, a);
  } else {
    SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(mvn_draws_kernel<T, false>), Tile::LDS_BYTES));
    hipLaunchKernelGGL((mvn_draws_kernel<T, false>), grid, dim3(256), Tile::LDS_BYTES, st, a);
  }
  SMN_CHECK_LAUNCH(ctx);
  SMN_HIP(ctx, hipStreamSynchronize(st));
  return SMN_OK;
}

}  // namespace

extern "C" int smn_rng_chi2(smn_ctx* ctx, uint64_t seed, double df, int64_t S, void* out_d) {
  if (!ctx || !out_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (!(df > 0.0) || std::isinf(df)) return smn_fail(ctx, SMN_EINVAL, "smn_rng_chi2: df must be positive and finite");
  if (S < 1 || S > ((int64_t)1 << 32)) return smn_fail(ctx, SMN_EINVAL, "smn_rng_chi2: 1 <= S <= 2^32 (the draw is a 32-bit counter word)");
  hipLaunchKernelGGL(chi2_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)seed, (uint32_t)(seed >> 32),
                     df, S, static_cast<double*>(out_d));
  SMN_CHECK_LAUNCH(ctx);
  return SMN_OK;
}

extern "C" int smn_mvn_draws(smn_ctx* ctx, int dtype, const void* mean_d, const void* l_d, int64_t ldl, int64_t T, int64_t C,
                             int64_t S, double df, double shape, uint64_t seed, int64_t point0, const void* noise_d,
                             const void* mix_d, void* out_d) {
  if (!ctx || !mean_d || !l_d || !out_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  if (dtype != SMN_F32 && dtype != SMN_F64) return smn_fail(ctx, SMN_EINVAL, "bad dtype %d", dtype);
  if (T < 1 || C < 1 || S < 1) return smn_fail(ctx, SMN_EINVAL, "smn_mvn_draws: T, C and S must be at least 1");
  if (C > SMN_SVSP_MAX_CLASSES) return smn_fail(ctx, SMN_ENOTSUP, "smn_mvn_draws: at most %d outputs", SMN_SVSP_MAX_CLASSES);
  if (df != df || (df > 0.0 && std::isinf(df))) return smn_fail(ctx, SMN_EINVAL, "smn_mvn_draws: df is NaN or infinite");
  if (df > 0.0 && !(shape > 0.0)) return smn_fail(ctx, SMN_EINVAL, "smn_mvn_draws: shape must be positive when df > 0");
  if (point0 < 0 || T > ((int64_t)1 << 32) || point0 + T > ((int64_t)1 << 32) || S > ((int64_t)1 << 32))
    return smn_fail(ctx, SMN_EINVAL, "smn_mvn_draws: bad sizes (point indices and draws are 32-bit counter words)");
  SMN_CHECK_LD(ctx, "smn_mvn_draws", ldl, T);
  return by_dtype(dtype, [&](auto e) {
    return mvn_draws_t<decltype(e)>(ctx, mean_d, l_d, ldl, T, (int)C, S, df, shape, seed, point0, noise_d, mix_d, out_d);
  });
}
