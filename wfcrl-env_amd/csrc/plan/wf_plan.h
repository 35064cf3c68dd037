// wf_plan.h — what the two translation units of the plan extension (include/wfplan.h) share: the arguments of the one kernel
// of wf_plan_kernels.hip and its launcher, called by wf_plan_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K H rows: that of the lookahead extension (lookahead/wf_lookahead.h) — evaluator
// farm e = slot R + row, row = k H + h; row (k, h) holds the yaw after step h of candidate k, under wind h.  Beside the
// evaluator's blocks a slot keeps, from launch to launch, its candidates [K][H][N], its best sequence [H][N] and its mean
// [H][N] (float32, raw actions).  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no
// output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfplan.h"
#include "../ext/wf_ext_kernels.h"

// What the launches of a run share, in DEVICE memory (uploaded once per run): the kernel reads a field where a phase needs
// it.  Passed by value instead, the 70 dwords are fetched on entry and stay in scalar registers across the staged row
// rewards, which take nearly all of them (wf_lookahead_reduce_kernel: 105 SGPRs): the compiler then spills.
struct WfPlanRun {
  int N, K, H, E, I;
  int wind_stride;        // 0 shared, 1 per farm
  float load_coef;
  double gamma;
  unsigned long long seed;
  const double *ws, *wd;  // the parent's wind
  const double* ws_prev;  // [B] the speed the next env step normalises by (null: the current one): step 0's
  WfEnvView env;          // the parent's env: the state is read, never written
  float* yaw;             // [C][R][N] the evaluator's input
  double *ews, *ewd;      // [C R] every row's wind, written by launch 0
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  float* cand;            // [C][K][H][N] the candidates of the iteration laid out last
  float *best, *mu;       // [C][H][N] the best sequence so far, the mean
  // the caller's arrays, a row (or block) per listed farm: a slot's is sl.base + slot.  Any may be null
  const double* wind;     // [n][H][2] (speed, direction), or null = the parent's wind held
  const float* mean0;     // [n][H][N], or null = zeros
  float* plan;            // [n][H][N]
  double *plan_return, *hold_return;  // [n]
  float *first_action, *final_yaw;    // [n][N]
  float* mean;            // [n][H][N]
};

// one launch: the chunk's slots, and v = 0 .. I — it reduces iteration v - 1 (v > 0), then lays out iteration v under sigma
// = sigma[v] degrees (v < I) or writes the outputs (v = I)
extern "C" hipError_t wfk_launch_plan_advance(const WfPlanRun* host, const WfPlanRun* dev, const WfSlots* sl, int v, double sigma,
                                              hipStream_t s);
extern "C" hipError_t wfk_plan_func_attributes(int kernel, hipFuncAttributes* a);
