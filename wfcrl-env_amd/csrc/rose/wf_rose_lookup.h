// wf_rose_lookup.h — the yaw-table look-up of include/wfrose.h as a device function: the ONE definition the kernels of the rose
// extension (wf_rose_kernels.hip: the lay-out of table cases, the look-up-table policy) and of the rollout extension
// (rollout/wf_rollout_kernels.hip: the controllers' targets) compile.  Steps 1-3 (reduction of the direction, the two
// brackets and their weights) depend on the wind alone and are formed once per wind; steps 4-5 (the table entries, LINEAR or
// NEAREST, one rounding to float32) once per turbine.  The library is built with -ffp-contract=off: a product and a sum stay
// two roundings, as in the NumPy restatement (tests/rose_ref.py).
#pragma once
#include <hip/hip_runtime.h>

#include "wf_rose.h"

namespace {

struct RoseBracket {
  int k, k1, j, j1;
  double fd, fs;
};

// number of axis nodes <= v (the axis is ascending): binary search, the same in every lane of a wave
__device__ __forceinline__ int rose_count_le(const double* __restrict__ ax, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ax[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// steps 1-3 of the look-up (include/wfrose.h)
__device__ __forceinline__ RoseBracket rose_bracket(const WfRoseTable& tb, double ws, double wd) {
  RoseBracket b;
  double w = fmod(wd, 360.0);
  if (w < 0.0) w += 360.0;
  const int Dt = tb.Dt, St = tb.St;
  if (Dt == 1) {
    b.k = 0; b.k1 = 0; b.fd = 0.0;
  } else {
    int k = rose_count_le(tb.twd, Dt, w) - 1;
    if (k < 0) { w += 360.0; k = Dt - 1; }
    if (k == Dt - 1) {
      const double x0 = tb.twd[Dt - 1], x1 = tb.twd[0] + 360.0;
      b.k = k; b.k1 = 0; b.fd = (w - x0) / (x1 - x0);
    } else {
      const double x0 = tb.twd[k], x1 = tb.twd[k + 1];
      b.k = k; b.k1 = k + 1; b.fd = (w - x0) / (x1 - x0);
    }
  }
  double v = ws;
  const double s_lo = tb.tws[0], s_hi = tb.tws[St - 1];
  v = v < s_lo ? s_lo : v;
  v = v > s_hi ? s_hi : v;
  int j = rose_count_le(tb.tws, St, v) - 1;
  j = j < 0 ? 0 : j;  // (a NaN speed: stay inside the table)
  const int j1 = j + 1 < St ? j + 1 : St - 1;
  b.j = j; b.j1 = j1;
  b.fs = j1 > j ? (v - tb.tws[j]) / (tb.tws[j1] - tb.tws[j]) : 0.0;
  return b;
}

// steps 4-5 for turbine t
__device__ __forceinline__ float rose_lookup(const WfRoseTable& tb, const RoseBracket& b, int t, int N) {
  const float* __restrict__ T = tb.T;
  const size_t St = (size_t)tb.St;
  if (tb.interp == WF_ROSE_NEAREST) {
    const int kd = b.fd > 0.5 ? b.k1 : b.k, js = b.fs > 0.5 ? b.j1 : b.j;
    return T[((size_t)kd * St + js) * N + t];
  }
  const double t00 = (double)T[((size_t)b.k * St + b.j) * N + t], t01 = (double)T[((size_t)b.k * St + b.j1) * N + t];
  const double t10 = (double)T[((size_t)b.k1 * St + b.j) * N + t], t11 = (double)T[((size_t)b.k1 * St + b.j1) * N + t];
  const double lo = (1.0 - b.fs) * t00 + b.fs * t01;
  const double hi = (1.0 - b.fs) * t10 + b.fs * t11;
  return (float)((1.0 - b.fd) * lo + b.fd * hi);
}

// the table of a slot: picked by comparison with constant indices, so that the by-value argument stays in the kernel-argument
// segment (indexing it with a run-time value would copy it to a private segment)
#define ROSE_PICK(tab, slot) ((slot) == 1 ? (tab)[1] : (slot) == 2 ? (tab)[2] : (slot) == 3 ? (tab)[3] : (tab)[0])
static_assert(WF_ROSE_SLOTS == 4, "ROSE_PICK names every slot");

}  // namespace
