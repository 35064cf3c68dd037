// wf_yawopt.h — what the two translation units of the yaw-optimiser extension (include/wfyawopt.h) share: the arguments of
// the three kernels of wf_yawopt_kernels.hip and their launchers, called by wf_yawopt_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K_max + 1 candidate rows: evaluator farm e = slot R + row, so a slot's yaw
// block [R][N] (and its power block) is contiguous and the chunk's blocks are one contiguous array — what the evaluator's
// wf_step reads and writes.  Row 0 is the incumbent, rows 1 .. K the candidates, rows K+1 .. R-1 copies of the incumbent
// (a pass with fewer candidates than K_max).  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm
// and write no output.
// The slots (WfSlots), the candidate grid (WfGrid), the order kernel's arguments and what the advance kernel shares with the
// robust search's (WfAdvanceArgs) are ext/wf_ext_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "../ext/wf_ext_kernels.h"

#define WF_YAWOPT_ROWS_MAX 32  // K_0 <= 31 candidates + the incumbent

struct WfYawoptOrderArgs : WfOrderArgs {};

struct WfYawoptWindArgs {
  WfSlots sl;
  const double *ws, *wd;  // the parent's wind, one per farm
  int R;
  double *ews, *ewd;      // [C R] each farm's wind repeated over its rows
};

struct WfYawoptAdvanceArgs : WfAdvanceArgs {
  const float* power;  // [C][R][N] the evaluator's output for prev
};

extern "C" hipError_t wfk_launch_yawopt_order(const WfYawoptOrderArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_yawopt_wind(const WfYawoptWindArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_yawopt_advance(const WfYawoptAdvanceArgs* a, hipStream_t s);
