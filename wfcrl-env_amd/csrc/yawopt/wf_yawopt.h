// wf_yawopt.h — what the two translation units of the yaw-optimiser extension (include/wfyawopt.h) share: the arguments of
// the three kernels of wf_yawopt_kernels.hip and their launchers, called by wf_yawopt_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K_max + 1 candidate rows: evaluator farm e = slot R + row, so a slot's yaw
// block [R][N] (and its power block) is contiguous and the chunk's blocks are one contiguous array — what the evaluator's
// wf_step reads and writes.  Row 0 is the incumbent, rows 1 .. K the candidates, rows K+1 .. R-1 copies of the incumbent
// (a pass with fewer candidates than K_max).  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm
// and write no output.
#pragma once
#include <hip/hip_runtime.h>

#define WF_YAWOPT_ROWS_MAX 32  // K_0 <= 31 candidates + the incumbent

// which farm a slot works on: farms[base + s] (or base + s without a list), s = slot for the chunk's own slots, 0 beyond
struct WfYawoptSlots {
  const int* farms;  // device copy of the caller's list, or null
  int base;          // first entry of the chunk in the list
  int n_slots;       // farms of this chunk (<= C)
  int C;             // slots of the evaluator
};

struct WfYawoptOrderArgs {
  WfYawoptSlots sl;
  const double *lx, *ly;  // [N] layout, caller's order
  double xc, yc;          // centre of rotation [A.1-1]
  const double* wd;       // the parent's wind directions
  int wind_stride;        // 0 shared, 1 per farm
  int N;
  int* order;             // [C][N]: caller index of the s-th turbine a slot visits
};

struct WfYawoptWindArgs {
  WfYawoptSlots sl;
  const double *ws, *wd;  // the parent's wind, one per farm
  int R;
  double *ews, *ewd;      // [C R] each farm's wind repeated over its rows
};

// One visit's candidate grid: value of candidate j (0-based) around the incumbent `inc`
//   mode 0 (pass 0)   a + j b                 a = lo, b = h_0
//   mode 1 (refine)   (inc - a) + (j + 1) b   a = h_{p-1}, b = 2 h_{p-1} / (K_p + 1)
// clipped to [lo, hi] in float64, rounded once to float32.
struct WfYawoptGrid {
  int s;     // position in the visit order, -1 = no such visit
  int mode, K;
  double a, b;
};

struct WfYawoptAdvanceArgs {
  WfYawoptSlots sl;
  int N, R;
  double lo, hi;
  WfYawoptGrid prev, next;  // the visit whose powers are in `power` (prev.s < 0: none, initialise from yaw0) / the one to lay out
  int first;                // prev is the run's first visit: its incumbent power is power_init
  const int* order;         // [C][N]
  const float* power;       // [C][R][N] the evaluator's output for prev
  float* yaw;               // [C][R][N] the evaluator's input for next
  float* best;              // [C][N] best yaw so far
  const float* yaw0;        // [n_slots][N] rows of this chunk, or null = zeros
  float *out_yaw, *out_power, *out_init;  // rows of this chunk: [n_slots][N], [n_slots], [n_slots]; written when next.s < 0 / first
};

extern "C" hipError_t wfk_launch_yawopt_order(const WfYawoptOrderArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_yawopt_wind(const WfYawoptWindArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_yawopt_advance(const WfYawoptAdvanceArgs* a, hipStream_t s);
