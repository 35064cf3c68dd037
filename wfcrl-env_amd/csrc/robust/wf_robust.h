// wf_robust.h — what the two translation units of the robust extension (include/wfrobust.h) share: the arguments of the
// five kernels of wf_robust_kernels.hip and their launchers, called by wf_robust_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R candidate rows and M members: evaluator farm e = (slot R + row) M + member, so a
// slot's yaw block [R][M][N] (and its power block, and its [R][M] row sums) is contiguous and the chunk's blocks are one
// contiguous array — what the evaluator's wf_step reads and writes.  Row 0 is the incumbent, rows 1 .. K the candidates,
// rows K+1 .. R-1 copies of the incumbent (a pass with fewer candidates than K_max); wf_robust_evaluate has R = 1.  Slots
// beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfrobust.h"

#define WF_ROBUST_ROWS_MAX 32  // K_0 <= 31 candidates + the incumbent

// which farm a slot works on: farms[base + s] (or base + s without a list), s = slot for the chunk's own slots, 0 beyond
struct WfRobustSlots {
  const int* farms;  // device copy of the caller's list, or null
  int base;          // first entry of the chunk in the list
  int n_slots;       // farms of this chunk (<= C)
  int C;             // slots of the evaluator
};

// the member set, device arrays
struct WfRobustMembers {
  const double* delta;  // [M] degrees
  const double* w;      // [M] normalised weights
  int M, frame;
};

struct WfRobustOrderArgs {
  WfRobustSlots sl;
  const double *lx, *ly;  // [N] layout, caller's order
  double xc, yc;          // centre of rotation [A.1-1]
  const double* wd;       // the parent's wind directions (the NOMINAL ones)
  int wind_stride;        // 0 shared, 1 per farm
  int N;
  int* order;             // [C][N]: caller index of the s-th turbine a slot visits
};

struct WfRobustLayoutArgs {
  WfRobustSlots sl;
  WfRobustMembers mb;
  const double *ws, *wd;  // the parent's wind
  int wind_stride;        // 0 shared, 1 per farm
  int R, N;
  double *ews, *ewd;      // [C R M] every row's wind: ws, wd + delta[m]
  int write_yaw;          // wf_robust_evaluate (R == 1): also the rows' yaw, from yaw_in
  const float* yaw_in;    // [n_slots][N] rows of this chunk, or null = zeros
  float* yaw;             // [C M][N]
};

struct WfRobustRowsumArgs {
  int n_rows, N;       // C R M rows
  const float* power;  // [n_rows][N] the evaluator's output
  double* rowsum;      // [n_rows] farm power of every row
};

// One visit's candidate grid: value of candidate j (0-based) around the incumbent `inc` (include/wfyawopt.h)
//   mode 0 (pass 0)   a + j b                 a = lo, b = h_0
//   mode 1 (refine)   (inc - a) + (j + 1) b   a = h_{p-1}, b = 2 h_{p-1} / (K_p + 1)
// clipped to [lo, hi] in float64, rounded once to float32.
struct WfRobustGrid {
  int s;     // position in the visit order, -1 = no such visit
  int mode, K;
  double a, b;
};

struct WfRobustAdvanceArgs {
  WfRobustSlots sl;
  WfRobustMembers mb;
  int N, R;
  double lo, hi;
  WfRobustGrid prev, next;  // the visit whose row sums are in `rowsum` (prev.s < 0: none, initialise from yaw0) / the one to lay out
  int first;                // prev is the run's first visit: its incumbent's E is power_init
  const int* order;         // [C][N]
  const double* rowsum;     // [C][R][M] farm power of prev's rows
  float* yaw;               // [C][R][M][N] the evaluator's input for next
  float* best;              // [C][N] best (nominal) yaw so far
  const float* yaw0;        // [n_slots][N] rows of this chunk, or null = zeros
  float *out_yaw, *out_power, *out_init;  // rows of this chunk: [n_slots][N], [n_slots], [n_slots]; written when next.s < 0 / first
};

struct WfRobustExpectArgs {
  WfRobustSlots sl;
  WfRobustMembers mb;
  int N;
  const float* power;    // [C][M][N]
  const double* rowsum;  // [C][M]
  double* expected;      // rows of this chunk [n_slots], or null
  double* turbine;       // [n_slots][N], or null
  float* member;         // [n_slots][M], or null
};

extern "C" hipError_t wfk_launch_robust_order(const WfRobustOrderArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_robust_layout(const WfRobustLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_robust_rowsum(const WfRobustRowsumArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_robust_advance(const WfRobustAdvanceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_robust_expect(const WfRobustExpectArgs* a, hipStream_t s);
extern "C" hipError_t wfk_robust_func_attributes(int kernel, hipFuncAttributes* a);
