// wf_lookahead.h — what the two translation units of the lookahead extension (include/wflookahead.h) share: the arguments of
// the two kernels of wf_lookahead_kernels.hip and their launchers, called by wf_lookahead_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K H rows: evaluator farm e = slot R + row, row = k H + h, so a slot's yaw block
// [K][H][N] (and its power block and load block [K][H][N][4]) is contiguous and the chunk's blocks are one contiguous array —
// what the evaluator's wf_step reads and writes.  Row (k, h) holds the yaw after step h of sequence k, under wind h.  Slots
// beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wflookahead.h"
#include "../ext/wf_ext_kernels.h"

struct WfLookaheadLayoutArgs {
  WfSlots sl;
  const double *ws, *wd;  // the parent's wind
  int wind_stride;        // 0 shared, 1 per farm
  int N, K, H;
  WfEnvView env;          // the parent's env: the state is read, never written
  const float* actions;   // [n_slots][K][H][N] blocks of this chunk
  const double* wind;     // [n_slots][H][2] (speed, direction) of this chunk, or null = the parent's wind held
  float* yaw;             // [C][R][N] the evaluator's input
  double *ews, *ewd;      // [C R] every row's wind
  float* final_yaw;       // [n_slots][K][N] of this chunk, or null
};

// the reduce kernel is the shared returns body (ext/wf_ext_kernels.h: wf_sequence_returns) and takes its arguments
struct WfLookaheadReduceArgs : WfReturnsReduceArgs {};

extern "C" hipError_t wfk_launch_lookahead_layout(const WfLookaheadLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_lookahead_reduce(const WfLookaheadReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_lookahead_func_attributes(int kernel, hipFuncAttributes* a);
