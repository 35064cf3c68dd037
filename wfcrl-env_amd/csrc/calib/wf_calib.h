// wf_calib.h — what the two translation units of the calib extension (include/wfcalib.h) share: the arguments of the one kernel
// of wf_calib_kernels.hip and its launcher, called by wf_calib_abi.hip.
//
// Layout of a chunk of Cs problem SLOTS with R = S C rows: evaluator farm e = (slot S + s) C + c; row (s, c) holds condition c's
// yaw under condition c's wind and is solved under entry slot S + s of the evaluator's table of WfResolveConsts.  Beside the
// evaluator's blocks a slot keeps, from launch to launch, its candidates [S] wf_model_set, its row losses [R], its state
// (WfCalibSlot: mean, best set, starting set, losses, count of invalid candidates) and the best set's rows [C][N].  Slots
// beyond the chunk's problems (a ragged last chunk) repeat slot 0's problem and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfcalib.h"
#include "../ext/wf_ext_kernels.h"
#include "../wf_resolve.h"

static_assert(sizeof(wf_model_set) == WF_CALIB_FIELDS * sizeof(double), "a wf_model_set is WF_CALIB_FIELDS doubles, in the header's order");

// a slot's state between two launches
struct WfCalibSlot {
  wf_model_set mu, best, init;
  double best_loss, init_loss;
  int n_invalid;
};

// What the launches of a run share, in DEVICE memory (uploaded once per run, as plan/wf_plan.h: WfPlanRun).
struct WfCalibRun {
  int N, S, C, E, I;
  int fit;               // 1: wf_calib_fit; 0: wf_calib_score — the candidates are `sets`, there is no update
  int sets_stride;       // entries of `sets` a problem owns: score S or 0 (shared), fit 1 or 0
  double scale, kappa;   // kappa: the model's, for the eddy viscosity (modelset/wf_resolve_set.h)
  unsigned long long seed;
  double lo[WF_CALIB_FIELDS], hi[WF_CALIB_FIELDS];
  const wf_model_set* sets;   // device copy of the caller's sets (score) or starting sets (fit)
  // the observations, a block per problem: a slot's is sl.base + slot
  const double *ws, *wd;      // [G][C]
  const float* yaw;           // [G][C][N]
  const double *power, *weight;  // [G][C][N]; weight may be null
  // the evaluator
  float* yaw_ev;              // [Cs][R][N] its input
  double *ews, *ewd;          // [Cs R] every row's wind, written by launch 0
  const float* power_ev;      // [Cs][R][N] its output
  WfResolveConsts* tab;       // [Cs S] its table: the set-owned members are written here
  // kept from launch to launch
  wf_model_set* cand;         // [Cs][S]
  double* row_loss;           // [Cs][R]
  WfCalibSlot* state;         // [Cs]
  float* fit_rows;            // [Cs][C][N]
  // the caller's outputs, a block per problem; any may be null
  double* loss;               // [G][S]           (score)
  int* best;                  // [G]
  float* row_power;           // [G][S][C][N]
  wf_model_set *best_set, *mean;  // [G]          (fit)
  double *best_loss, *init_loss;  // [G]
  double* history;            // [G][I]
  float* fit_power;           // [G][C][N]
  int* n_invalid;             // [G]
};

// one launch: the chunk's slots, and v = 0 .. I — it reduces iteration v - 1 (v > 0), then lays out iteration v under the width
// sigma = sigma[v] (v < I) or writes the outputs (v = I)
extern "C" hipError_t wfk_launch_calib_advance(const WfCalibRun* host, const WfCalibRun* dev, const WfSlots* sl, int v, double sigma,
                                               hipStream_t s);
extern "C" hipError_t wfk_calib_func_attributes(int kernel, hipFuncAttributes* a);
