// wf_grad_kernels.hip — the kernels around the step kernel that make yaw sensitivities — the power Jacobian and its
// vector-Jacobian product as central difference quotients — run on the device (include/wfgrad.h).  The farm solve is the
// existing wf_step on the object's evaluator handle; these two kernels are the glue, so that a whole run is enqueued
// without a host read:
//
//   wf_grad_layout_kernel  once per chunk: the evaluator's [C][R][N] yaw block — row 0 the yaw as given, rows 2 i + 1 and
//                          2 i + 2 with entry i moved to y+_i / y-_i (clipped in float64, rounded once) —, every row's wind
//                          from the parent's device wind, and the divisors d[C][N].  ONE WAVE PER ROW, lanes over turbines
//                          in a loop: a row's N floats are contiguous, so every store is a whole line.
//   wf_grad_reduce_kernel  once per chunk, after the step: power, gradient and Jacobian of the chunk's farms.  A block owns a
//                          TILE of T turbines i of one slot.  Their 2 T perturbed rows are contiguous in the evaluator's power
//                          block: they are staged in LDS with coalesced loads (consecutive threads on consecutive floats), the
//                          P+ rows and the P- rows in two arrays of odd row stride.  Then thread k < T forms S_i of its
//                          turbine — sum_j c_j (P+_j - P-_j) over j in caller order in float64, one LDS row each, no bank
//                          conflict — while ALL threads write the tile's [T][N] Jacobian rows, consecutive threads on
//                          consecutive j: the N^2 doubles of a farm, its largest stream, leave in whole lines.
//
// T is what 32 KiB of LDS holds (50 turbines at N = 80, 24 at N = 165, the whole farm below N = 45); there is no
// size-dependent second path.  Trip counts are run-time values (no unrolled register arrays): no private segment, no spill,
// no out-of-line call (tests/test_grad.py reads the metadata).  The library is built with -ffp-contract=off: a product and a
// sum stay two roundings, as in the NumPy restatement.
#include <hip/hip_runtime.h>

#include "wf_grad.h"

namespace {

// the perturbed yaws (include/wfgrad.h): float64, clipped, rounded once
__device__ __forceinline__ float gr_plus(float y, double h, double hi) {
  double p = (double)y + h;
  p = p > hi ? hi : p;
  return (float)p;
}
__device__ __forceinline__ float gr_minus(float y, double h, double lo) {
  double m = (double)y - h;
  m = m < lo ? lo : m;
  return (float)m;
}

}  // namespace

__global__ __launch_bounds__(256) void wf_grad_layout_kernel(const WfGradLayoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int N = a.N, R = 2 * N + 1;
  if (e >= a.sl.C * R) return;
  const int slot = e / R, row = e - slot * R;
  if (lane == 0) {
    const int b = wf_slot_farm(a.sl, slot);
    a.ews[e] = a.ws[(size_t)b * a.wind_stride];
    a.ewd[e] = a.wd[(size_t)b * a.wind_stride];
  }
  const float* __restrict__ src = a.yaw_in ? a.yaw_in + (size_t)(slot < a.sl.n_slots ? slot : 0) * N : nullptr;
  float* __restrict__ out = a.yaw + (size_t)e * N;
  const int ti = row > 0 ? (row - 1) >> 1 : -1;  // the turbine this row moves
  const bool up = (row & 1) != 0;                // rows 2 i + 1: y+, rows 2 i + 2: y-
  for (int t = lane; t < N; t += 64) {
    const float y = src ? src[t] : 0.0f;
    float v = y;
    if (t == ti) v = up ? gr_plus(y, a.h, a.hi) : gr_minus(y, a.h, a.lo);
    out[t] = v;
    if (row == 0) a.d[(size_t)slot * N + t] = (double)gr_plus(y, a.h, a.hi) - (double)gr_minus(y, a.h, a.lo);
  }
}

__global__ __launch_bounds__(256) void wf_grad_reduce_kernel(const WfGradReduceArgs a, int T, int stride, int n_tiles) {
  extern __shared__ float gr_lds[];
  float* plus = gr_lds;                // [T][stride] P of rows 2 i + 1
  float* minus = gr_lds + T * stride;  // [T][stride] P of rows 2 i + 2
  float* cl = minus + T * stride;      // [N] the cotangent row
  const int tid = threadIdx.x, nth = blockDim.x;
  const int N = a.N, R = 2 * N + 1;
  const int slot = blockIdx.x / n_tiles, tile = blockIdx.x - slot * n_tiles;
  const int i0 = tile * T;
  int nt = N - i0;
  nt = nt > T ? T : nt;
  const float* __restrict__ blk = a.power_ev + (size_t)slot * R * N;
  const size_t row0 = (size_t)slot * N;
  if (tile == 0 && a.power)
    for (int t = tid; t < N; t += nth) a.power[row0 + t] = blk[t];
  if (!a.gradient && !a.jacobian) return;  // (block-uniform)
  const float* __restrict__ src = blk + (size_t)(1 + 2 * i0) * N;
  const int n_load = 2 * nt * N;
  for (int q = tid; q < n_load; q += nth) {
    const int r = q / N, t = q - r * N;
    ((r & 1) ? minus : plus)[(r >> 1) * stride + t] = src[q];
  }
  if (a.gradient)
    for (int t = tid; t < N; t += nth) cl[t] = a.cot ? a.cot[row0 + t] : 1.0f;
  __syncthreads();
  const double* __restrict__ dv = a.d + row0 + i0;
  if (a.gradient && tid < nt) {
    const float* pp = plus + tid * stride;
    const float* pm = minus + tid * stride;
    double sum = 0.0;
    for (int j = 0; j < N; ++j) sum += (double)cl[j] * ((double)pp[j] - (double)pm[j]);
    const double d = dv[tid];
    a.gradient[row0 + i0 + tid] = d > 0.0 ? sum / d : 0.0;
  }
  if (a.jacobian) {
    double* __restrict__ jac = a.jacobian + (row0 + i0) * N;
    const int n_store = nt * N;
    for (int q = tid; q < n_store; q += nth) {
      const int k = q / N, j = q - k * N;
      const double d = dv[k];
      jac[q] = d > 0.0 ? ((double)plus[k * stride + j] - (double)minus[k * stride + j]) / d : 0.0;
    }
  }
}

extern "C" hipError_t wfk_launch_grad_layout(const WfGradLayoutArgs* a, hipStream_t s) {
  const int n = a->sl.C * (2 * a->N + 1);
  hipLaunchKernelGGL(wf_grad_layout_kernel, dim3((n + 3) / 4), dim3(256), 0, s, *a);
  return hipGetLastError();
}
extern "C" hipError_t wfk_launch_grad_reduce(const WfGradReduceArgs* a, hipStream_t s) {
  const int N = a->N, stride = N | 1;
  int T = 4096 / stride;  // turbines per tile: two [T][stride] float arrays in 32 KiB of LDS, at most a turbine per thread
  T = T < 1 ? 1 : (T > N ? N : T);
  const int n_tiles = (N + T - 1) / T;
  const int threads = 2 * T * N <= 512 ? 64 : 256;  // a small farm's tile (T = N <= 16) is a few hundred floats: one wave
  const size_t lds = sizeof(float) * (2 * (size_t)T * stride + N);
  hipLaunchKernelGGL(wf_grad_reduce_kernel, dim3(a->n_slots * n_tiles), dim3(threads), lds, s, *a, T, stride, n_tiles);
  return hipGetLastError();
}
extern "C" hipError_t wfk_grad_func_attributes(int kernel, hipFuncAttributes* a) {
  const void* fn[WF_GRAD_KERNELS] = {(const void*)wf_grad_layout_kernel, (const void*)wf_grad_reduce_kernel};
  if (kernel < 0 || kernel >= WF_GRAD_KERNELS) return hipErrorInvalidValue;
  return hipFuncGetAttributes(a, fn[kernel]);
}
