// wf_windgen_kernels.hip — the two kernels of the wind generator extension (include/wfwindgen.h: DEFINITION).  They store the
// same bits: the same operations in the same order on every (farm, tick); which one runs is the host's choice
// (wf_windgen_abi.hip).  The series is tick-major, [T][B]: row u is the contiguous [B] array a tick hands to wf_set_wind.
// Row 0 (tick 0) is read, not written: the reset draw's kernel or the caller's upload filled it.  Indices are size_t: T B may
// pass 2^31.  No private segment in either (tests/test_windgen.py compiles them and checks).
//
//   wf_windgen_kernel        ONE THREAD PER FARM walks the farm's ticks u = 1 .. T - 1: the recursion is serial in u, and its
//                            state — the two latents, tick 0, the ramp rate — stays in registers.  Every tick takes two Philox
//                            blocks (the deviates of streams 4 and 5, ext/wf_deviate.h), two multiply-add pairs, a clip and
//                            an fmod, and stores one speed and one direction; the lanes of a wave write consecutive doubles
//                            of row u: whole 512-byte lines per wave and row.  Blocks of one wave, no LDS.  The least work
//                            per (farm, tick), but a thread's T - 1 ticks are one dependent chain of about 2 x 10 Philox
//                            rounds each: a small batch (4096 farms are 64 waves on 256 compute units) waits for that chain.
//   wf_windgen_tiled_kernel  A BLOCK OF 256 THREADS PER 64 FARMS, in tiles of 32 ticks; the recursion is serial in u, the draws are
//                            not.  Per tile: (1) every thread draws the deviates of 8 (farm, tick) pairs into LDS, [tick][farm],
//                            consecutive lanes on consecutive doubles; (2) the first wave, a lane per farm, walks the tile:
//                            two LDS reads, the two multiply-add pairs, and the latents written back in place; (3) every
//                            thread clips / wraps 8 latents and stores them, a wave on 64 consecutive doubles of one row.  The
//                            serial chain per tick shrinks to the walk's four dependent operations.  32 KiB of LDS, three
//                            barriers per tile, all in block-uniform control flow (the trip counts are kernel arguments).
//
// -ffp-contract=off: every product and sum is one rounding, in the order the definition writes them; tests/windgen_ref.py
// restates them in NumPy and the device reproduces its bits.
#include <hip/hip_runtime.h>

#include "../ext/wf_deviate.h"
#include "wf_windgen.h"

#define WF_WINDGEN_BLOCK 64

__global__ __launch_bounds__(WF_WINDGEN_BLOCK) void wf_windgen_kernel(const WfWindgenArgs a) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t B = (size_t)a.B;
  if (b >= B) return;
  const double S0 = a.ws[b], D0 = a.wd[b];
  unsigned r[4];
  philox4x32_10(a.seed, (unsigned long long)b, 3u, r);
  const double rate = a.wd_ramp * (2.0 * u01(r[0], r[1]) - 1.0);
  const unsigned long long hi = (unsigned long long)b << 32;
  double x = S0, y = D0;
  size_t e = b;
  for (int u = 1; u < a.T; ++u) {
    e += B;
    const double zs = wf_deviate(a.seed, hi | (unsigned)u, 4u);
    const double zd = wf_deviate(a.seed, hi | (unsigned)u, 5u);
    x = (x + a.ws_revert * (S0 - x)) + a.ws_sigma * zs;
    const double m = D0 + rate * (double)u;
    y = (y + a.wd_revert * (m - y)) + a.wd_sigma * zd;
    double d = fmod(y, 360.0);
    if (d < 0.0) d += 360.0;
    a.ws[e] = fmin(fmax(x, a.ws_lo), a.ws_hi);
    a.wd[e] = d;
  }
}

#define WF_WINDGEN_FARMS 64
#define WF_WINDGEN_TICKS 32
#define WF_WINDGEN_THREADS 256

__global__ __launch_bounds__(WF_WINDGEN_THREADS) void wf_windgen_tiled_kernel(const WfWindgenArgs a) {
  __shared__ double zs[WF_WINDGEN_TICKS][WF_WINDGEN_FARMS], zd[WF_WINDGEN_TICKS][WF_WINDGEN_FARMS];
  const int tid = threadIdx.x;
  const size_t B = (size_t)a.B;
  const size_t b0 = (size_t)blockIdx.x * WF_WINDGEN_FARMS;
  // the walkers: lane f of the first wave keeps farm b0 + f's state
  const bool walker = tid < WF_WINDGEN_FARMS && b0 + tid < B;
  double S0 = 0.0, D0 = 0.0, rate = 0.0, x = 0.0, y = 0.0;
  if (walker) {
    const size_t b = b0 + tid;
    S0 = a.ws[b]; D0 = a.wd[b];
    unsigned r[4];
    philox4x32_10(a.seed, (unsigned long long)b, 3u, r);
    rate = a.wd_ramp * (2.0 * u01(r[0], r[1]) - 1.0);
    x = S0; y = D0;
  }
  for (int u0 = 1; u0 < a.T; u0 += WF_WINDGEN_TICKS) {  // (block-uniform)
    const int nt = a.T - u0 < WF_WINDGEN_TICKS ? a.T - u0 : WF_WINDGEN_TICKS;
    const int n = nt * WF_WINDGEN_FARMS;
    for (int i = tid; i < n; i += WF_WINDGEN_THREADS) {
      const int k = i / WF_WINDGEN_FARMS, f = i % WF_WINDGEN_FARMS;
      const size_t b = b0 + f;
      if (b < B) {
        const unsigned long long ctr = ((unsigned long long)b << 32) | (unsigned)(u0 + k);
        zs[k][f] = wf_deviate(a.seed, ctr, 4u);
        zd[k][f] = wf_deviate(a.seed, ctr, 5u);
      }
    }
    __syncthreads();
    if (walker) {
      for (int k = 0; k < nt; ++k) {
        x = (x + a.ws_revert * (S0 - x)) + a.ws_sigma * zs[k][tid];
        const double m = D0 + rate * (double)(u0 + k);
        y = (y + a.wd_revert * (m - y)) + a.wd_sigma * zd[k][tid];
        zs[k][tid] = x;
        zd[k][tid] = y;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += WF_WINDGEN_THREADS) {
      const int k = i / WF_WINDGEN_FARMS, f = i % WF_WINDGEN_FARMS;
      const size_t b = b0 + f;
      if (b < B) {
        const size_t e = (size_t)(u0 + k) * B + b;
        double d = fmod(zd[k][f], 360.0);
        if (d < 0.0) d += 360.0;
        a.ws[e] = fmin(fmax(zs[k][f], a.ws_lo), a.ws_hi);
        a.wd[e] = d;
      }
    }
    __syncthreads();  // (the tile is drawn over next)
  }
}

extern "C" hipError_t wfk_launch_windgen(const WfWindgenArgs* a, int tiled, hipStream_t s) {
  if (a->B <= 0 || a->T <= 1) return hipSuccess;
  if (tiled) {
    const unsigned blocks = (unsigned)(((size_t)a->B + WF_WINDGEN_FARMS - 1) / WF_WINDGEN_FARMS);
    hipLaunchKernelGGL(wf_windgen_tiled_kernel, dim3(blocks), dim3(WF_WINDGEN_THREADS), 0, s, *a);
  } else {
    const unsigned blocks = (unsigned)(((size_t)a->B + WF_WINDGEN_BLOCK - 1) / WF_WINDGEN_BLOCK);
    hipLaunchKernelGGL(wf_windgen_kernel, dim3(blocks), dim3(WF_WINDGEN_BLOCK), 0, s, *a);
  }
  return hipGetLastError();
}
extern "C" hipError_t wfk_windgen_func_attributes(int kernel, hipFuncAttributes* a) {
  if (kernel == 0) return hipFuncGetAttributes(a, (const void*)wf_windgen_kernel);
  if (kernel == 1) return hipFuncGetAttributes(a, (const void*)wf_windgen_tiled_kernel);
  return hipErrorInvalidValue;
}
