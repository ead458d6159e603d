// cnn_pool.hip — conv-NNGP kernel with global average pooling in front of the read-out:
//     L x [Conv(1 ch, 3x3, stride 1, SAME, W_std=w, b_std=b); act];  GlobalAvgPool;  Dense(last_w, b=0)
// (neural_tangents stax.Conv / stax.GlobalAvgPool / stax.Dense; the Flatten sibling is cnn.hip).  The pooled read-out needs the
// covariance of EVERY pixel p of image n with EVERY pixel q of image m: with P = H W pixels
//     K0[p,q]  = sum_c x1[n,p,c] x2[m,q,c] / C
//     K~[p,q]  = w^2/9 sum_{d in 3x3} K[p+d, q+d] + b^2          (a term is 0 when p+d or q+d is outside the image)
//     K[p,q]   = act(K~[p,q]; q~_n[p], q~_m[q])
//     out[n,m] = last_w^2 sum_{p,q} K_L[p,q] / P^2
// P^2 entries per pair and layer where cnn.hip has P.  q~_n[p] = K~_nn[p,p] obeys the same-pixel recursion, so the per-image
// factor tables are conv_q_kernel's, unchanged (cnn_tables).
//
// Decomposition.  The shift d moves p and q together, so the offset D = q - p is fixed under the conv: for every D in
// (-H,H) x (-W,W) the slice S_D[p] = K[p, p+D] is an independent 2-D map over the rectangle where both pixels are inside, and its
// layer step is the zero-padded box sum OF THAT RECTANGLE.  The (2H-1)(2W-1) rectangles are grouped four at a time into P units of
// exactly P entries each: unit (a, b), 0 <= a < H, 0 <= b < W, pairs pixel (h, w) of image n with pixel ((h+a) mod H, (w+b) mod W)
// of image m -- a cyclic shift, whose four quadrants (rows below / from H-a, columns below / from W-b) are the slices
// D = (a | a-H, b | b-W).  A unit is therefore the sibling's per-wave problem on the full H x W map: lanes own pixels lane + 64 i,
// the map lives in LDS with a zero halo, the stencil is nine LDS reads -- with one zero WALL row and one zero wall column
// between the quadrants, so that no tap crosses from one slice into another.  The padded map is (H+3) x (W+3); image row h sits
// in map row h + 1 (h < H-a) or h + 2, the wall in map row H-a+1 (a = 0: the wall is the bottom halo), columns alike.  Moving
// from one unit to the next, only the new wall row and column are zeroed: every other cell of the interior is a pixel of the
// new unit and is overwritten by its first publish.
//
// Sums.  A unit's P values are added per lane in fp64 (pixel order), across the wave by a fixed butterfly, and written to
// part[pair][unit]; pool_reduce_kernel adds the P partial sums of a pair in an order fixed by (H, W) alone.  No atomics: the bits
// of out[n,m] are a function of the two images, the hyper-parameters and (H, W, C) only -- not of n1, n2, fill, ldk, the pair's
// position, the grid or the number of passes the pair list is cut into (workspace budget: smn_debug_batch_bytes).
// Every wave walks the (pair, unit) list with the stride of the grid, so the P units of a single pair spread over the chip.
//
// The diagonal pair (n, n) of a symmetric build runs through the same kernel.  Its unit (0, 0) is the same-pixel slice, whose
// entries ARE the per-image variances: there the activation is the per-image recursion's (ReLU: q~/2; erf: (2/pi) asin(2q~/(1+2q~)))
// instead of the pair map at c = 1.
#include "cnn_pairs.hpp"
#include "internal.hpp"
#include "nngp_math.hpp"

namespace {

using namespace smn_cnn;

enum { POOL_CROSS = 0, POOL_LOWER = 1, POOL_DIAG = 2 };

template <typename T>
struct PoolArgs {
  const T* x1; const T* x2; const T* R1; const T* R2;
  int64_t n2; int mode, mirror;
  ConvProg prog;
  int64_t pair0, npairs;   // this pass: pairs [pair0, pair0 + npairs) of the pair list
  double* part;            // [npairs][H W] unit sums
  T* out; int64_t ldo;
};

template <typename T>
__device__ __forceinline__ void pool_pair(const PoolArgs<T>& a, int64_t pr, int64_t& n, int64_t& m) {
  if (a.mode == POOL_CROSS) {
    // pr / n2 by a double division and one correction step (pr < 2^53), as tri_decode takes its root: the emulated 64-bit
    // integer division costs several times as many instructions, once per unit
    n = (int64_t)((double)pr / (double)a.n2);
    m = pr - n * a.n2;
    if (m < 0) {
      --n;
      m += a.n2;
    } else if (m >= a.n2) {
      ++n;
      m -= a.n2;
    }
  } else if (a.mode == POOL_LOWER) {
    tri_decode(pr, n, m);
  } else {
    n = m = pr;
  }
}

// the activation of the same-pixel slice of a diagonal pair: the per-image recursion (diag_act of cnn_pairs.hpp), in T
template <typename T, int ACT>
__device__ __forceinline__ T act_same_pixel(T qt) {
  if (ACT == 0) return T(0.5) * qt;
  return nngp::erf_map<T, false>(qt, rcp_any<T>(fma(T(2), qt, T(1))), T(0)).k;
}

// workgroups per CU a form is compiled for: the 16-pixel forms want the registers (at 3 the fp32 form spills 80 words a lane)
constexpr int pool_occ(int np) { return np <= 4 ? 4 : 2; }

// blockDim.x / 64 waves per workgroup (4; fewer where four maps do not fit the LDS), each with ONE padded map of its own.
template <typename T, int ACT, int NP>
__global__ void __launch_bounds__(256, pool_occ(NP)) pool_pair_kernel(PoolArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvProg& p = a.prog;
  const int H = p.H, W = p.W, HW = H * W, PW = W + 3, PH = H + 3, PSZ = PH * PW, MSZ = PSZ + PW + 3;
  const int lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the walk below runs on the scalar unit
  T* map = reinterpret_cast<T*>(smem) + (size_t)wave * MSZ;
  for (int i = lane; i < MSZ; i += 64) map[i] = T(0);   // the outer halo and the dummy slot's surroundings stay zero
  int hw[NP];   // (h << 16) | w of pixel lane + 64 i (clamped to the last pixel past the image)
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int px = min(lane + 64 * i, HW - 1);
    hw[i] = ((px / W) << 16) | (px % W);
  }
  const T w2_9 = (T)(p.w2 / 9.0), b2 = (T)p.b2;
  const T inv_c = (T)(1.0 / p.C);
  const int C = p.C, L = p.layers;
  // unit u = pl * HW + su of this pass, u = first, first + stride, ...: (pl, su) advance by (stride / HW, stride % HW) with a
  // carry, so the 64-bit divisions are made once per kernel and not once per unit (7 - 14 % of the 8x8 build:
  // profiles/r25_cnn_pool.txt)
  const int64_t first = (int64_t)blockIdx.x * nwave + wave, stride = (int64_t)gridDim.x * nwave;
  const int64_t step_pl = stride / HW;
  const int step_su = (int)(stride - step_pl * HW);
  int64_t pl = first / HW;
  int su = (int)(first - pl * HW);
  while (pl < a.npairs) {
    const int64_t u = pl * HW + su;
    const int sa = (int)((unsigned)su / (unsigned)W), sb = su - sa * W;
    const int hs = H - sa, ws = W - sb;   // rows below hs pair with row + sa, the others with row + sa - H; columns alike
    int64_t n, m;
    pool_pair(a, a.pair0 + pl, n, m);
    const bool same = a.mode != POOL_CROSS && n == m && su == 0;
    // the walls of this unit (in-order LDS of one wave: the previous unit's tap reads were issued before)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < PW; i += 64) map[(hs + 1) * PW + i] = T(0);
    for (int i = lane; i < PH; i += 64) map[i * PW + ws + 1] = T(0);
    unsigned off[NP], qp[NP];   // (unsigned: a table load is scalar base + 32-bit lane offset, not a 64-bit address per pixel)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int h = hw[i] >> 16, w = hw[i] & 0xffff;
      const bool lo_h = h < hs, lo_w = w < ws;
      off[i] = lane + 64 * i < HW ? (h + (lo_h ? 1 : 2)) * PW + w + (lo_w ? 1 : 2) : PSZ + 1;   // past the image: the dummy slot
      qp[i] = (h + sa - (lo_h ? 0 : H)) * W + w + sb - (lo_w ? 0 : W);
    }
    T val[NP];
    {
      const T* xa = a.x1 + n * HW * C;
      const T* xb = a.x2 + m * HW * C;
#pragma unroll
      for (int i = 0; i < NP; ++i) val[i] = T(0);
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int i = 0; i < NP; ++i) val[i] = fma(xa[(unsigned)(min(lane + 64 * i, HW - 1) * C + c)], xb[qp[i] * C + c], val[i]);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) val[i] *= inv_c;
    }
    for (int l = 0; l < L; ++l) {
      const T* r1 = a.R1 + (n * L + l) * HW;
      const T* r2 = a.R2 + (m * L + l) * HW;
      // The row stride re-read as an opaque scalar per layer (WaveMap::box of cnn_pairs.hpp does the same): left loop-invariant,
      // three row addresses per pixel stay alive across the layer loop.  Without it the 16-pixel forms take 256 VGPRs and spill
      // 112 (ReLU) / 176 (erf) bytes per lane in fp64 against 251 / 255 VGPRs and 0 / 28 bytes, and the fp32 4-pixel forms drop
      // from 5 to 4 waves per SIMD (profiles/r25_cnn_pool.txt).  An empty statement: no instruction is named.
      int pw = PW;
      asm volatile("" : "+s"(pw));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < NP; ++i) map[off[i]] = val[i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (same) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const T* t1 = map + off[i] - 1;
          const T* t0 = t1 - pw;
          const T* t2 = t1 + pw;
          const T bs = ((t0[0] + t0[1]) + (t0[2] + t1[0])) + ((t1[1] + t1[2]) + (t2[0] + t2[1])) + t2[2];
          val[i] = act_same_pixel<T, ACT>(fma(w2_9, bs, b2));
        }
      } else {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const T rr = r1[(unsigned)min(lane + 64 * i, HW - 1)] * r2[qp[i]];
          const T* t1 = map + off[i] - 1;
          const T* t0 = t1 - pw;
          const T* t2 = t1 + pw;
          const T bs = ((t0[0] + t0[1]) + (t0[2] + t1[0])) + ((t1[1] + t1[2]) + (t2[0] + t2[1])) + t2[2];
          val[i] = act_value<T, ACT>(fma(w2_9, bs, b2), rr);
        }
      }
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) s += lane + 64 * i < HW ? (double)val[i] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) a.part[u] = s;
    pl += step_pl;
    su += step_su;
    if (su >= HW) {
      su -= HW;
      ++pl;
    }
  }
}

// One workgroup per pair: out = last_w^2 (sum of the pair's P unit sums) / P^2, thread t adding units t, t + 256, ... in
// turn and the 256 threads by a tree -- an order fixed by P alone.
template <typename T>
__global__ void __launch_bounds__(256) pool_reduce_kernel(PoolArgs<T> a) {
  __shared__ double red[256];
  const int HW = a.prog.H * a.prog.W;
  const int64_t pl = blockIdx.x;
  const double* part = a.part + pl * HW;
  double s = 0.0;
  for (int k = threadIdx.x; k < HW; k += 256) s += part[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int64_t n, m;
    pool_pair(a, a.pair0 + pl, n, m);
    const T v = (T)(a.prog.lw2 * red[0] / ((double)HW * (double)HW));
    if (a.mode == POOL_DIAG) {
      a.out[n] = v;
    } else {
      a.out[n * a.ldo + m] = v;
      if (a.mirror && n != m) a.out[m * a.ldo + n] = v;
    }
  }
}

// The form of the pair kernel for one call, chosen and prepared once whatever the number of passes: the kernel, its workgroup
// (64 x waves threads, `lds` bytes of dynamic LDS, allowed here) and the workgroups the device holds at once.
template <typename T>
struct PoolForm {
  void (*kern)(PoolArgs<T>);
  int waves; size_t lds; int64_t resident;
};
template <typename T, int ACT>
void (*pool_kernel_for(int64_t hw))(PoolArgs<T>) {
  return hw <= 64 ? pool_pair_kernel<T, ACT, 1> : hw <= 256 ? pool_pair_kernel<T, ACT, 4> : pool_pair_kernel<T, ACT, 16>;
}
template <typename T>
int pool_form(smn_ctx* ctx, int act, int64_t hw, int waves, size_t lds, PoolForm<T>* f) {
  f->kern = act == SMN_ACT_RELU ? pool_kernel_for<T, 0>(hw) : pool_kernel_for<T, 1>(hw);
  f->waves = waves;
  f->lds = lds;
  SMN_TRY(smn_allow_lds(ctx, reinterpret_cast<const void*>(f->kern), lds));
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f->kern, 64 * waves, lds) != hipSuccess || per_cu <= 0) per_cu = 1;
  f->resident = (int64_t)ctx->num_cu * per_cu;
  return SMN_OK;
}

constexpr size_t kPoolPartBytes = (size_t)256 << 20;   // partial sums of one pass (or smn_debug_batch_bytes, if smaller)

// mode POOL_CROSS: out [n1, n2] (ld = ldo);  POOL_LOWER: x2 = x1, pairs m <= n, mirrored when `mirror`;  POOL_DIAG: out [n1]
template <typename T>
int cnn_pool_t(smn_ctx* ctx, const char* who, int mode, int act, int layers, double w, double b, double lw, const void* x1,
               int64_t n1, const void* x2, int64_t n2, int64_t H, int64_t W, int64_t C, int mirror, void* out, int64_t ldk) {
  const bool cross = mode == POOL_CROSS;
  const ConvProg p = make_prog(act, layers, H, W, C, w, b, lw);
  const int64_t HW = H * W;
  const size_t msz = (size_t)(H + 3) * (W + 3) + (size_t)(W + 3) + 3;
  int waves = 4;
  while (waves > 1 && waves * msz * sizeof(T) > 160 * 1024) waves >>= 1;
  const size_t lds = waves * msz * sizeof(T);
  if (lds > 160 * 1024 || conv_q_lds_bytes(H, W) > 160 * 1024)
    return smn_fail(ctx, SMN_ENOTSUP, "%s: image %lldx%lld too large for the on-chip map", who, (long long)H, (long long)W);
  PoolForm<T> form;
  SMN_TRY(pool_form<T>(ctx, act, HW, waves, lds, &form));
  const int64_t npairs = cross ? n1 * n2 : mode == POOL_LOWER ? n1 * (n1 + 1) / 2 : n1;
  size_t budget = ctx->batch_bytes < kPoolPartBytes ? ctx->batch_bytes : kPoolPartBytes;
  int64_t per_pass = (int64_t)(budget / ((size_t)HW * sizeof(double)));
  if (per_pass < 1) per_pass = 1;
  if (per_pass > npairs) per_pass = npairs;
  // workspace: R1 [n1][L][HW], R2, the per-image pass's own diagonals (not used here), then the partial sums
  const size_t lt = (size_t)(layers > 0 ? layers : 1);
  const size_t qn1 = (size_t)n1 * lt * HW, qn2 = cross ? (size_t)n2 * lt * HW : 0;
  const size_t tab = (sizeof(T) * (qn1 + qn2 + (size_t)n1 + (cross ? (size_t)n2 : 0)) + 63) & ~(size_t)63;
  void* tv = nullptr;
  SMN_TRY(smn_workspace(ctx, 1, tab + (size_t)per_pass * HW * sizeof(double), &tv));
  T* R1 = static_cast<T*>(tv);
  T* R2 = cross ? R1 + qn1 : R1;
  T* d1 = R1 + qn1 + qn2;
  T* d2 = d1 + n1;
  const int dtype = sizeof(T) == 8 ? SMN_F64 : SMN_F32;
  SMN_TRY(cnn_tables(ctx, dtype, p, x1, n1, R1, d1));
  if (cross) SMN_TRY(cnn_tables(ctx, dtype, p, x2, n2, R2, d2));
  PoolArgs<T> a;
  a.x1 = static_cast<const T*>(x1); a.x2 = cross ? static_cast<const T*>(x2) : a.x1;
  a.R1 = R1; a.R2 = R2; a.n2 = cross ? n2 : n1; a.mode = mode; a.mirror = mirror;
  a.prog = p; a.part = reinterpret_cast<double*>(static_cast<char*>(tv) + tab);
  a.out = static_cast<T*>(out); a.ldo = ldk;
  for (int64_t p0 = 0; p0 < npairs; p0 += per_pass) {
    a.pair0 = p0;
    a.npairs = npairs - p0 < per_pass ? npairs - p0 : per_pass;
    int64_t blocks = (a.npairs * HW + form.waves - 1) / form.waves;
    if (blocks > form.resident) blocks = form.resident;   // the units cost the same: one resident set, every wave strides the list
    {
      ProfScope ps(ctx, PROF_BUILD, ctx->stream);
      hipLaunchKernelGGL(form.kern, dim3((unsigned)blocks), dim3(64 * form.waves), form.lds, ctx->stream, a);
    }
    SMN_CHECK_LAUNCH(ctx);   // (before the reduction is queued on its output)
    {
      ProfScope ps(ctx, PROF_BUILD, ctx->stream);
      hipLaunchKernelGGL(pool_reduce_kernel<T>, dim3((unsigned)a.npairs), dim3(256), 0, ctx->stream, a);
    }
    SMN_CHECK_LAUNCH(ctx);
  }
  return SMN_OK;
}

}  // namespace

extern "C" int smn_kernel_cnn_pool(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                   double last_w_std, const void* x1_d, int64_t n1, const void* x2_d, int64_t n2, int64_t H,
                                   int64_t W, int64_t C, int fill, void* nngp_d, int64_t ldk) {
  if (!ctx || !x1_d || !nngp_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(conv_check(ctx, "smn_kernel_cnn_pool", dtype, act, num_hiddens, n1, H, W, C, SMN_CNN_POOL_MAX_PIXELS));
  if (fill != SMN_FILL_FULL && fill != SMN_FILL_LOWER) return smn_fail(ctx, SMN_EINVAL, "smn_kernel_cnn_pool: bad fill %d", fill);
  if (x2_d && n2 <= 0) return smn_fail(ctx, SMN_EINVAL, "smn_kernel_cnn_pool: bad sizes");
  if (x2_d) SMN_CHECK_LD(ctx, "smn_kernel_cnn_pool", ldk, n2);
  else SMN_CHECK_LD(ctx, "smn_kernel_cnn_pool", ldk, n1);
  return by_dtype(dtype, [&](auto e) {
    return cnn_pool_t<decltype(e)>(ctx, "smn_kernel_cnn_pool", x2_d ? POOL_CROSS : POOL_LOWER, act, num_hiddens, w_std, b_std,
                                   last_w_std, x1_d, n1, x2_d, n2, H, W, C, (!x2_d && fill == SMN_FILL_FULL) ? 1 : 0, nngp_d, ldk);
  });
}

extern "C" int smn_kernel_cnn_pool_diag(smn_ctx* ctx, int dtype, int act, int num_hiddens, double w_std, double b_std,
                                        double last_w_std, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                        void* diag_d) {
  if (!ctx || !x_d || !diag_d) return SMN_EINVAL;
  SMN_ENTER(ctx);
  SMN_TRY(conv_check(ctx, "smn_kernel_cnn_pool_diag", dtype, act, num_hiddens, n, H, W, C, SMN_CNN_POOL_MAX_PIXELS));
  return by_dtype(dtype, [&](auto e) {
    return cnn_pool_t<decltype(e)>(ctx, "smn_kernel_cnn_pool_diag", POOL_DIAG, act, num_hiddens, w_std, b_std, last_w_std, x_d, n,
                                   nullptr, n, H, W, C, 0, diag_d, 1);
  });
}
