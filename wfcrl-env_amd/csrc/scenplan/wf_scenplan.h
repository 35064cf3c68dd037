// wf_scenplan.h — what the two translation units of the scenplan extension (include/wfscenplan.h) share: the arguments of the
// two kernels of wf_scenplan_kernels.hip and their launchers, called by wf_scenplan_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K M H rows: that of the scenario extension (scenario/wf_scenario.h) — evaluator
// farm e = slot R + row, row = (k M + m) H + h; row (k, m, h) holds the yaw after step h of candidate k, under member m's wind
// of tick h + 1.  Beside the evaluator's blocks a slot keeps, from launch to launch, what a plan slot keeps (plan/wf_plan.h):
// its candidates [K][H][N], its best sequence [H][N] and its mean [H][N] (float32, raw actions); and, for the last launch's
// outputs, every candidate's member returns [K][M] and (mean, tail mean) [K][2] (float64).  Slots beyond the chunk's farms (a
// ragged last chunk) repeat slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfscenplan.h"
#include "../ensemble/wf_ensemble.h"
#include "../ext/wf_ext_kernels.h"

// the paths kernel's arguments, by value: once per chunk
struct WfScenPlanPathsArgs {
  WfSlots sl;
  WfEnsemble ens;         // the paths: scenario_seed, process, bounds, anchor, the parent's wind, M, H
  int K;
  double *ews, *ewd;      // [C R] every row's wind
  double* wind_paths;     // [n_slots][M][H][2] of this chunk, or null
};

// What the advance launches of a run share, in DEVICE memory (uploaded once per run): the kernel reads a field where a phase
// needs it (plan/wf_plan.h says why it is not passed by value).
struct WfScenPlanRun {
  int N, K, M, H, E, I;
  int q;                  // the tail: the q lowest member returns
  int wind_stride;        // 0 shared, 1 per farm
  float load_coef;
  double gamma, lam;
  unsigned long long seed;  // the planner's
  const double* ws;       // the parent's wind speed: step 0's normaliser (a pending prev-wind speed is not read)
  WfEnvView env;          // the parent's env: the state is read, never written
  float* yaw;             // [C][R][N] the evaluator's input
  const double* ews;      // [C R] every row's wind speed, written by the paths kernel: row (k, m, h - 1)'s normalises step h >= 1
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  float* cand;            // [C][K][H][N] the candidates of the iteration laid out last
  float *best, *mu;       // [C][H][N] the best sequence so far, the mean
  double* mret;           // [C][K][M] the last iteration's member returns ...
  double* stat;           // [C][K][2] ... and every candidate's (mean, tail mean)
  // the caller's arrays, a row (or block) per listed farm: a slot's is sl.base + slot.  Any may be null
  const float* mean0;     // [n][H][N], or null = zeros
  float* plan;            // [n][H][N]
  double *plan_score, *plan_expected, *plan_cvar, *hold_score;  // [n]
  double* plan_member_returns;        // [n][M]
  float *first_action, *final_yaw;    // [n][N]
  float* mean;            // [n][H][N]
};

extern "C" hipError_t wfk_launch_scenplan_paths(const WfScenPlanPathsArgs* a, hipStream_t s);
// one launch: the chunk's slots, and v = 0 .. I — it reduces iteration v - 1 (v > 0), then lays out iteration v under sigma
// = sigma[v] degrees (v < I) or writes the outputs (v = I)
extern "C" hipError_t wfk_launch_scenplan_advance(const WfScenPlanRun* host, const WfScenPlanRun* dev, const WfSlots* sl, int v, double sigma,
                                                  hipStream_t s);
extern "C" hipError_t wfk_scenplan_func_attributes(int kernel, hipFuncAttributes* a);
