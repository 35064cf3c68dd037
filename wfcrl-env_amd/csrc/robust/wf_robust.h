// wf_robust.h — what the two translation units of the robust extension (include/wfrobust.h) share: the arguments of the
// five kernels of wf_robust_kernels.hip and their launchers, called by wf_robust_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R candidate rows and M members: evaluator farm e = (slot R + row) M + member, so a
// slot's yaw block [R][M][N] (and its power block, and its [R][M] row sums) is contiguous and the chunk's blocks are one
// contiguous array — what the evaluator's wf_step reads and writes.  Row 0 is the incumbent, rows 1 .. K the candidates,
// rows K+1 .. R-1 copies of the incumbent (a pass with fewer candidates than K_max); wf_robust_evaluate has R = 1.  Slots
// beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output.
// The slots (WfSlots), the candidate grid (WfGrid), the order kernel's arguments and what the advance kernel shares with the
// yaw optimiser's (WfAdvanceArgs) are ext/wf_ext_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfrobust.h"
#include "../ext/wf_ext_kernels.h"

#define WF_ROBUST_ROWS_MAX 32  // K_0 <= 31 candidates + the incumbent

// the member set, device arrays
struct WfRobustMembers {
  const double* delta;  // [M] degrees
  const double* w;      // [M] normalised weights
  int M, frame;
};

struct WfRobustOrderArgs : WfOrderArgs {};  // (wd: the NOMINAL directions)

struct WfRobustLayoutArgs {
  WfSlots sl;
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

struct WfRobustAdvanceArgs : WfAdvanceArgs {  // (yaw: [C][R][M][N])
  WfRobustMembers mb;
  const double* rowsum;  // [C][R][M] farm power of prev's rows
};

struct WfRobustExpectArgs {
  WfSlots sl;
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
