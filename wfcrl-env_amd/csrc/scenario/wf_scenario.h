// wf_scenario.h — what the two translation units of the scenario extension (include/wfscenario.h) share: the arguments of
// the two kernels of wf_scenario_kernels.hip and their launchers, called by wf_scenario_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K M H rows: evaluator farm e = slot R + row, row = (k M + m) H + h, so a slot's
// yaw block [K][M][H][N] (and its power block and load block [K][M][H][N][4]) is contiguous and the chunk's blocks are one
// contiguous array — what the evaluator's wf_step reads and writes.  Row (k, m, h) holds the yaw after step h of sequence k,
// under member m's wind of step h.  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no
// output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfscenario.h"
#include "../ensemble/wf_ensemble.h"
#include "../ext/wf_ext_kernels.h"

struct WfScenarioLayoutArgs {
  WfSlots sl;
  WfEnsemble ens;         // the paths: seed, process, bounds, anchor, the parent's wind, M, H
  int N, K;
  WfEnvView env;          // the parent's env: the state is read, never written
  const float* actions;   // [n_slots][K][H][N] blocks of this chunk
  float* yaw;             // [C][R][N] the evaluator's input
  double *ews, *ewd;      // [C R] every row's wind
  double* wind_paths;     // [n_slots][M][H][2] of this chunk, or null
  float* final_yaw;       // [n_slots][K][N] of this chunk, or null
};

struct WfScenarioReduceArgs {
  WfSlots sl;
  int N, K, M, H;
  const double* ws;       // the parent's wind speed: step 0's normaliser (a pending prev-wind speed is not read)
  int wind_stride;
  const double* ews;      // [C R] every row's wind speed: row (k, m, h - 1)'s normalises step h >= 1
  float load_coef;
  double gamma, lam;
  int q;                  // the tail: the q lowest member returns
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  double *expected, *cvar, *score;  // rows of this chunk [n_slots][K], or null
  double* member_returns;           // [n_slots][K][M], or null
  double* rewards;                  // [n_slots][R], or null
  int* best;                        // [n_slots], or null
};

extern "C" hipError_t wfk_launch_scenario_layout(const WfScenarioLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_scenario_reduce(const WfScenarioReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_scenario_func_attributes(int kernel, hipFuncAttributes* a);
