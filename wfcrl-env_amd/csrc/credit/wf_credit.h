// wf_credit.h — what the two translation units of the credit extension (include/wfcredit.h) share: the arguments of the two
// kernels of wf_credit_kernels.hip and their launchers, called by wf_credit_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = 1 + N K rows: evaluator farm e = slot R + row, so a slot's yaw block [R][N] (and
// its power block [R][N] and load block [R][N][4]) is contiguous and the chunk's blocks are one contiguous array — what the
// evaluator's wf_step reads and writes.  Row 0 is the base yaw, row 1 + i K + k has entry i replaced by alternative (i, k).
// Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output (WfSlots:
// ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfcredit.h"
#include "../ext/wf_ext_kernels.h"

// the parent's env: parameters by value, state by (read-only) pointer (ext/wf_ext_kernels.h)
typedef WfEnvView WfCreditEnv;

struct WfCreditLayoutArgs {
  WfSlots sl;
  const double *ws, *wd;  // the parent's wind
  int wind_stride;        // 0 shared, 1 per farm
  const double* wind;     // [n_slots][2] (speed, direction) rows of this chunk that replace it (include/wfseries.h), or null
  int N, K;
  WfCreditEnv env;
  int base_kind, alt_kind;  // WF_CREDIT_YAW / WF_CREDIT_ACTION
  const float* base;        // [n_slots][N] rows of this chunk, or null = the env's yaw state
  const float* alt;         // [n_slots][N][K] rows of this chunk, or null = hold / zero yaw (K == 1)
  float* yaw;               // [C][R][N] the evaluator's input
  double *ews, *ewd;        // [C R] every row's wind
};

struct WfCreditReduceArgs {
  WfSlots sl;
  int N, K;
  const double* ws;       // the parent's wind speed ...
  int wind_stride;
  const double* ws_prev;  // ... or [B] the speed the next env step normalises by (null: the current one)
  float load_coef;
  const float* yaw_ev;    // [C][R][N] the evaluator's input (which alternative has the base entry's bits)
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  double* reward;         // rows of this chunk [n_slots][R], or null
  double* farm_power;     // [n_slots][R], or null
  double* difference;     // [n_slots][N][K], or null
};

extern "C" hipError_t wfk_launch_credit_layout(const WfCreditLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_credit_reduce(const WfCreditReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_credit_func_attributes(int kernel, hipFuncAttributes* a);
