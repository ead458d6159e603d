// r10: what does a run of R consecutive MFMAs on the SAME accumulator cost?  (sibling of scratch/r04/mfma_f64/mfma_forms.hip,
// which measured independent chains only.)  16 accumulators per wave, operands pinned in registers, no memory traffic; one loop
// iteration is 64 MFMAs in every variant:
//   R = 1   acc0 acc1 ... acc15, four times over            (an accumulator is rewritten every 16 MFMAs)
//   R = 2   acc0 acc0 acc1 acc1 ... acc15 acc15, twice over  (runs of two: what Mfma<double>::mma issues)
//   R = 4   acc0 x4, acc1 x4, ... acc15 x4                   (runs of four: what Mfma<float>::mma issues)
// f32 v_mfma_f32_16x16x4_f32 and f64 v_mfma_f64_16x16x4_f64, at 1, 2 and 4 waves per SIMD (WPS workgroups of 4 waves per CU,
// the launch bound asks for that residency and the host prints what the runtime grants).  16 f64 accumulators are 128 VGPRs,
// which leaves no room at 4 waves per SIMD (128 VGPRs per wave): that line runs 8 accumulators and says so.
// The MFMAs are compiler builtins (so the hazard recogniser inserts whatever wait states the hardware needs) with a
// sched_barrier after each one, which pins the order as written; check with
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only mfma_chain_probe.hip
// that the loop holds 64 MFMAs in the intended order and no accumulator copies.
// Build: hipcc --offload-arch=gfx950 -O3 -o mfma_chain_probe mfma_chain_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Op;
template <> struct Op<float> {
  using acc_t = f32x4;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <> struct Op<double> {
  using acc_t = f64x4;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};

template <typename T, int R, int NACC, int WPS>
__global__ void __launch_bounds__(256, WPS < 2 ? 2 : WPS) k(   // (bound 1: the compiler moves the accumulators to AGPRs and copies them)
T* out, long long* clk, int iters, T a0, T b0) {
  using acc_t = typename Op<T>::acc_t;
  T a = a0 + T(threadIdx.x % 7) * T(1e-3), b = b0 - T(threadIdx.x % 5) * T(1e-3);
  asm volatile("" : "+v"(a), "+v"(b));
  acc_t acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j) acc[j] = acc_t{T(0), T(0), T(0), T(0)};
  const long long c0 = __builtin_readcyclecounter(), r0 = wall_clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int pass = 0; pass < 64 / (NACC * R); ++pass)
#pragma unroll
      for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          acc[j] = Op<T>::mma(a, b, acc[j]);
          __builtin_amdgcn_sched_barrier(0);
        }
  }
  const long long c1 = __builtin_readcyclecounter(), r1 = wall_clock64();
  T s = T(0);
#pragma unroll
  for (int j = 0; j < NACC; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  if (s == T(12345.678)) out[0] = s;
  if (threadIdx.x == 0) { clk[2 * blockIdx.x] = c1 - c0; clk[2 * blockIdx.x + 1] = r1 - r0; }
}

int main() {
  hipDeviceProp_t p; CHK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  void* d; long long* clk;
  CHK(hipMalloc(&d, 64)); CHK(hipMalloc(&clk, sizeof(long long) * 2 * cus * 8));
  hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  printf("device: %s, %d CUs; cycle table: v_mfma_f32_16x16x4_f32 32 cycles per SIMD to issue, v_mfma_f64_16x16x4_f64 64\n", p.gcnArchName, cus);
  printf("%-6s %-3s %-4s %-9s %-9s %9s %9s %7s   %s\n", "type", "R", "acc", "waves/SIMD", "resident", "ms", "TFLOP/s", "MHz", "cycles per MFMA per SIMD");
  auto run = [&](auto tsel, auto rsel, auto nsel, auto wsel, int iters) -> int {
    using T = typename decltype(tsel)::type;
    constexpr int R = decltype(rsel)::value, NACC = decltype(nsel)::value, WPS = decltype(wsel)::value;
    auto kern = k<T, R, NACC, WPS>;
    int resident = 0;
    CHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, 256, 0));
    const int grid = cus * WPS;
    for (int rep = 0; rep < 3; ++rep) {
      CHK(hipEventRecord(e0));
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, (T*)d, clk, iters, T(1.0001), T(0.9999));
      CHK(hipGetLastError());
      CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
      float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
      if (rep < 2) continue;
      std::vector<long long> h(2 * grid);
      CHK(hipMemcpy(h.data(), clk, sizeof(long long) * 2 * grid, hipMemcpyDeviceToHost));
      std::vector<double> mhz(grid);
      for (int i = 0; i < grid; ++i) mhz[i] = h[2 * i + 1] > 0 ? 100.0 * (double)h[2 * i] / (double)h[2 * i + 1] : 0.0;
      std::sort(mhz.begin(), mhz.end());
      const double nmfma_simd = 64.0 * iters * WPS;               // MFMAs one SIMD issues in the launch
      const double tf = nmfma_simd * 2048.0 * 4.0 * cus / (ms * 1e-3) / 1e12, clkm = mhz[grid / 2];
      printf("%-6s %-3d %-4d %-10d %-9d %9.3f %9.2f %7.0f   %6.1f\n", sizeof(T) == 8 ? "f64" : "f32", R, NACC, WPS, std::min(resident, WPS), ms, tf, clkm,
             ms * 1e-3 * clkm * 1e6 / nmfma_simd);
    }
    return 0;
  };
  using F = std::common_type<float>; using D = std::common_type<double>;
  using std::integral_constant;
#define ROW(TS, N, W, IT)                                                                                   \
  if (run(TS{}, integral_constant<int, 1>{}, integral_constant<int, N>{}, integral_constant<int, W>{}, IT)) return 1; \
  if (run(TS{}, integral_constant<int, 2>{}, integral_constant<int, N>{}, integral_constant<int, W>{}, IT)) return 1; \
  if (run(TS{}, integral_constant<int, 4>{}, integral_constant<int, N>{}, integral_constant<int, W>{}, IT)) return 1;
  ROW(F, 16, 1, 8000)
  ROW(F, 16, 2, 4000)
  ROW(F, 16, 4, 2000)
  ROW(D, 16, 1, 4000)
  ROW(D, 16, 2, 2000)
  ROW(D, 8, 4, 1000)    // 8 accumulators: 16 f64 accumulators do not fit 4 waves per SIMD
  return 0;
}
