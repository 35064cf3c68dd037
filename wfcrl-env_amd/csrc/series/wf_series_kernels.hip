// wf_series_kernels.hip — the one kernel of the series extension (include/wfseries.h).
//
//   wf_series_window_kernel  ONE THREAD PER (farm, h): entry h of the farm's window is series row
//                            (start[b] + min(tick0 + h, T - 1)) % T.  The tick and the row are formed in 64-bit, so no T, start
//                            or horizon wraps an int; the output index is a size_t.  Consecutive threads write consecutive
//                            (speed, direction) pairs: plain vector-memory stores, whole lines per wave.  A shared series is T
//                            doubles read by every thread: it stays in cache.  A series per farm (a wind generator's,
//                            include/wfwindgen.h: tick-major, no start rows, no wrap) is read at row * row_stride +
//                            farm * farm_stride, a size_t: T B elements may pass 2^31.
#include <hip/hip_runtime.h>

#include "wf_series.h"

__global__ __launch_bounds__(256) void wf_series_window_kernel(const WfSeriesWindowArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)a.n * (size_t)a.H) return;
  const int f = (int)(i / (size_t)a.H), h = (int)(i - (size_t)f * a.H);
  const int b = a.farms ? a.farms[f] : f;
  long long u = (long long)a.tick0 + h;
  u = u < (long long)a.T - 1 ? u : (long long)a.T - 1;
  const long long row = a.start ? ((long long)a.start[b] + u) % (long long)a.T : u;
  const size_t e = (size_t)row * a.row_stride + (size_t)b * a.farm_stride;
  a.wind[2 * i] = a.s_ws[e];  // (two 8-byte stores: a caller's array need not be 16-byte aligned)
  a.wind[2 * i + 1] = a.s_wd[e];
}

extern "C" hipError_t wfk_launch_series_window(const WfSeriesWindowArgs* a, hipStream_t s) {
  const size_t n = (size_t)a->n * (size_t)a->H;
  hipLaunchKernelGGL(wf_series_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_series_func_attributes(int kernel, hipFuncAttributes* a) {
  if (kernel != 0) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, (const void*)wf_series_window_kernel);
}
