// wf_rollscen.h — what the two translation units of the scenario-rollout extension (include/wfrollscen.h) share: the arguments
// of the kernels of wf_rollscen_kernels.hip and their launchers, called by wf_rollscen_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K M H rows: that of the scenario extension (scenario/wf_scenario.h) — evaluator
// farm e = slot R + row, row = (k M + m) H + h, so a slot's yaw block [K][M][H][N] is contiguous.  Row (k, m, h) holds the yaw
// after step h of controller k under member m, and is solved under member m's wind of tick h + 1.  Slots beyond the chunk's
// farms (a ragged last chunk) repeat slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).  The brackets of a
// slot — one per (k, m, h): the table look-up's steps 1-3 at the filtered wind — are records of 32 bytes: in the block's LDS up
// to WF_ROLLSCEN_LDS_RECORDS of them, in a scratch block of the object's, [C][R] in global memory, above (`spill`).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfrollscen.h"
#include "../ext/wf_ext_kernels.h"
#include "../rose/wf_rose.h"
#include "../scenario/wf_scenario.h"

// a (k, m, h)'s bracket as the lay-out kernel's walkers hand it to the trajectories: the look-up's four indices and two weights
struct WfRollscenBracket {
  int k, k1, j, j1;
  double fd, fs;
};

struct WfRollscenLayoutArgs {
  WfSlots sl;
  WfEnsemble ens;          // the paths: seed, process, bounds, anchor, the parent's wind, M, H
  int N, K;
  WfEnvView env;           // the parent's env: the state is read, never written
  WfRoseTable tab[WF_ROSE_SLOTS];  // the rose object's tables
  const int* c_slot;       // [K] the controllers (device copies)
  const double* c_alpha;   // [K]
  const float* c_deadband; // [K]
  const int* c_lead;       // [K]
  const double* filter0;   // [n_slots][K][2] of this chunk, or null = the farm's current wind
  int spill;               // the brackets go through brk, not LDS
  WfRollscenBracket* brk;  // [C][R] scratch (spill), or null
  float* yaw;              // [C][R][N] the evaluator's input
  double *ews, *ewd;       // [C R] every row's wind
  double* wind_paths;      // [n_slots][M][H][2] of this chunk, or null
  float* actions;          // [n_slots][K][M][H][N], or null
  float* final_yaw;        // [n_slots][K][M][N], or null
  int* gated;              // [n_slots][K][M], or null
  float* first_action;     // [n_slots][K][N], or null
};

// the reduce kernel is the scenario extension's body (scenario/wf_scenario_reduce.h) and takes its arguments, K = the controllers
struct WfRollscenReduceArgs : WfScenarioReduceArgs {};

extern "C" hipError_t wfk_launch_rollscen_layout(const WfRollscenLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_rollscen_reduce(const WfRollscenReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_rollscen_func_attributes(int kernel, hipFuncAttributes* a);
