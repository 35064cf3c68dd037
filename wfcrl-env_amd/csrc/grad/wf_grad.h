// wf_grad.h — what the two translation units of the gradient extension (include/wfgrad.h) share: the arguments of the two
// kernels of wf_grad_kernels.hip and their launchers, called by wf_grad_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = 2 N + 1 rows: evaluator farm e = slot R + row, so a slot's yaw block [R][N]
// (and its power block) is contiguous and the chunk's blocks are one contiguous array — what the evaluator's wf_step reads
// and writes.  Row 0 is the yaw as given, row 2 i + 1 has y_i -> y+_i, row 2 i + 2 has y_i -> y-_i.  Slots beyond the
// chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfgrad.h"
#include "../ext/wf_ext_kernels.h"

struct WfGradLayoutArgs {
  WfSlots sl;
  const double *ws, *wd;  // the parent's wind
  int wind_stride;        // 0 shared, 1 per farm
  int N;
  double h, lo, hi;       // step and bounds [deg]
  const float* yaw_in;    // [n_slots][N] rows of this chunk, or null = zeros
  float* yaw;             // [C][R][N] the evaluator's input
  double *ews, *ewd;      // [C R] every row's wind
  double* d;              // [C][N] the divisors d_i = (double)y+_i - (double)y-_i
};

struct WfGradReduceArgs {
  int n_slots, N;
  const float* power_ev;  // [C][R][N] the evaluator's output
  const double* d;        // [C][N]
  const float* cot;       // [n_slots][N] rows of this chunk, or null = ones
  float* power;           // rows of this chunk [n_slots][N], or null
  double* gradient;       // [n_slots][N], or null
  double* jacobian;       // [n_slots][N][N], or null
};

extern "C" hipError_t wfk_launch_grad_layout(const WfGradLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_grad_reduce(const WfGradReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_grad_func_attributes(int kernel, hipFuncAttributes* a);
