// wf_ext_kernels.h — the device side the extensions share (yawopt/, robust/, grad/): which farm a chunk's slot works on,
// a visit's candidate grid, and the visit order of a slot's turbines.  The per-extension headers build their kernels'
// argument structs from these; wf_ext.h is the host side.
#pragma once
#include <hip/hip_runtime.h>

#include "../wf_f64_math.h"

// which farm a slot works on: farms[base + s] (or base + s without a list), s = slot for the chunk's own slots, 0 beyond
struct WfSlots {
  const int* farms;  // device copy of the caller's list, or null
  int base;          // first entry of the chunk in the list
  int n_slots;       // farms of this chunk (<= C)
  int C;             // slots of the evaluator
};

// One visit's candidate grid: value of candidate j (0-based) around the incumbent `inc` (include/wfyawopt.h)
//   mode 0 (pass 0)   a + j b                 a = lo, b = h_0
//   mode 1 (refine)   (inc - a) + (j + 1) b   a = h_{p-1}, b = 2 h_{p-1} / (K_p + 1)
// clipped to [lo, hi] in float64, rounded once to float32.
struct WfGrid {
  int s;     // position in the visit order, -1 = no such visit
  int mode, K;
  double a, b;
};

// the order kernels' arguments (WfYawoptOrderArgs and WfRobustOrderArgs derive from it: the kernels keep their names)
struct WfOrderArgs {
  WfSlots sl;
  const double *lx, *ly;  // [N] layout, caller's order
  double xc, yc;          // centre of rotation [A.1-1]
  const double* wd;       // the parent's wind directions (the nominal ones)
  int wind_stride;        // 0 shared, 1 per farm
  int N;
  int* order;             // [C][N]: caller index of the s-th turbine a slot visits
};

#define WF_ORDER_MAX_N 256

__device__ __forceinline__ int wf_slot_farm(const WfSlots& sl, int slot) {
  const int s = sl.base + (slot < sl.n_slots ? slot : 0);
  return sl.farms ? sl.farms[s] : s;
}

// candidate j of a visit's grid around `inc`.  The library is built with -ffp-contract=off: a product and a sum stay two
// roundings, as in the NumPy restatement.
__device__ __forceinline__ float wf_grid_candidate(const WfGrid& g, double inc, int j, double lo, double hi) {
  double c = g.mode == 0 ? g.a + (double)j * g.b : (inc - g.a) + (double)(j + 1) * g.b;
  c = c < lo ? lo : c;
  c = c > hi ? hi : c;
  return (float)c;
}

// Each slot's visit order, upstream to downstream: the float64 rotation and stable rank sort of wf_geometry_kernel /
// wf_probe_state_kernel.  One workgroup per slot, one thread per turbine; sx is the block's __shared__ double[WF_ORDER_MAX_N].
__device__ __forceinline__ void wf_visit_order(const WfOrderArgs& a, double* sx) {
  const int N = a.N, t = threadIdx.x, slot = blockIdx.x;
  const int b = wf_slot_farm(a.sl, slot);
  // wd % 360, rotation about the bounding-box centre [A.1]: the arithmetic of wf_geometry_kernel
  double wdm = fmod(a.wd[(size_t)b * a.wind_stride], 360.0);
  if (wdm < 0.0) wdm += 360.0;
  double dev = fmod(wdm - 270.0, 360.0);
  if (dev < 0.0) dev += 360.0;
  dev = fmod(dev + 360.0, 360.0);
  double ca, sa;
  sincos_any(dev * (M_PI / 180.0), sa, ca);
  double xr = 0.0;
  if (t < N) {
    const double xo = a.lx[t] - a.xc, yo = a.ly[t] - a.yc;
    xr = xo * ca - yo * sa + a.xc;
    sx[t] = xr;
  }
  __syncthreads();
  if (t < N) {
    int rank = 0;
    for (int u = 0; u < N; ++u) {
      const double xu = sx[u];
      rank += (xu < xr) || (xu == xr && u < t);
    }
    a.order[(size_t)slot * N + rank] = t;
  }
}
