// wf_rollout.h — what the two translation units of the rollout extension (include/wfrollout.h) share: the arguments of the
// two kernels of wf_rollout_kernels.hip and their launchers, called by wf_rollout_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K H rows, as the lookahead extension's (lookahead/wf_lookahead.h): evaluator
// farm e = slot R + row, row = k H + h, so a slot's yaw block [K][H][N] is contiguous.  Row (k, h) holds the yaw after step h
// of controller k, under wind h.  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no
// output (WfSlots: ext/wf_ext_kernels.h).  The brackets of a slot — one per (k, h): the table look-up's steps 1-3 at the
// filtered wind — lie in a scratch block of the object's, [C][R] records of 32 bytes in global memory (K H of them exceed
// LDS at the limits).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfrollout.h"
#include "../ext/wf_ext_kernels.h"
#include "../rose/wf_rose.h"

// a (k, h)'s bracket as the lay-out kernel's two phases hand it over: the look-up's four indices and two weights
struct WfRolloutBracket {
  int k, k1, j, j1;
  double fd, fs;
};

struct WfRolloutLayoutArgs {
  WfSlots sl;
  const double *ws, *wd;   // the parent's wind
  int wind_stride;         // 0 shared, 1 per farm
  int N, K, H;
  WfEnvView env;           // the parent's env: the state is read, never written
  WfRoseTable tab[WF_ROSE_SLOTS];  // the rose object's tables
  const int* c_slot;       // [K] the controllers (device copies)
  const double* c_alpha;   // [K]
  const float* c_deadband; // [K]
  const int* c_lead;       // [K]
  const double* wind;      // [n_slots][H][2] (speed, direction) of this chunk, or null = the parent's wind held
  const double* filter0;   // [n_slots][K][2] of this chunk, or null = the farm's current wind
  WfRolloutBracket* brk;   // [C][R] scratch: phase A writes (the filtered wind, then its bracket), phase B reads
  float* yaw;              // [C][R][N] the evaluator's input
  double *ews, *ewd;       // [C R] every row's wind
  float* actions;          // [n_slots][K][H][N] of this chunk, or null
  float* final_yaw;        // [n_slots][K][N], or null
  int* gated;              // [n_slots][K], or null
  double* filter_final;    // [n_slots][K][2], or null
};

// the reduce kernel is the shared returns body (ext/wf_ext_kernels.h: wf_sequence_returns) and takes its arguments
struct WfRolloutReduceArgs : WfReturnsReduceArgs {};

extern "C" hipError_t wfk_launch_rollout_layout(const WfRolloutLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_rollout_reduce(const WfRolloutReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_rollout_func_attributes(int kernel, hipFuncAttributes* a);
