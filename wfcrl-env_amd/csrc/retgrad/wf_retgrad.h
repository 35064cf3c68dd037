// wf_retgrad.h — what the two translation units of the retgrad extension (include/wfretgrad.h) share: the arguments of the
// three kernels of wf_retgrad_kernels.hip and their launchers, called by wf_retgrad_abi.hip.
//
// Layout of a chunk of C farm SLOTS with R = K H W rows, W = 2 N + 1: evaluator farm e = slot R + row,
// row = (k H + h) W + j, so the W rows of a step — the base yaw after step h of sequence k (j = 0), turbine i moved up
// (j = 2 i + 1) and down (j = 2 i + 2) — are contiguous, and so are their powers and loads: the reduce kernel stages a step's
// rows as one block.  All rows of a step are under wind h.  Slots beyond the chunk's farms (a ragged last chunk) repeat
// slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfretgrad.h"
#include "../ext/wf_ext_kernels.h"

struct WfRetgradLayoutArgs {
  WfSlots sl;
  const double *ws, *wd;  // the parent's wind
  int wind_stride;        // 0 shared, 1 per farm
  int N, K, H;
  WfEnvView env;          // the parent's env: the state is read, never written
  double delta;           // the perturbation, degrees
  const float* actions;   // [n_slots][K][H][N] blocks of this chunk
  const double* wind;     // [n_slots][H][2] (speed, direction) of this chunk, or null = the parent's wind held
  float* yaw;             // [C][R][N] the evaluator's input
  double *ews, *ewd;      // [C R] every row's wind
  double* div;            // [C][K][H][N] the divisors d
  unsigned char* flags;   // [C][K][H][N] bit 0 = s, bit 1 = t
  float* traj;            // [n_slots][K][H][N] of this chunk, or null
  unsigned char* pass_mask;  // [n_slots][K][H][N] of this chunk, or null
  float* final_yaw;       // [n_slots][K][N] of this chunk, or null
};

struct WfRetgradReduceArgs {
  WfSlots sl;
  int N, K, H;
  const double* ws;       // the parent's wind speed ...
  int wind_stride;
  const double* ws_prev;  // ... or [B] the speed the next env step normalises by (null: the current one): step 0's
  const double* ews;      // [C R] every row's wind speed: base row (k, h - 1)'s normalises step h >= 1
  float load_coef;
  double gamma;
  const float* power_ev;  // [C][R][N] the evaluator's outputs
  const float* load_ev;   // [C][R][N][4]
  const double* div;      // [C][K][H][N]
  const unsigned char* flags;  // [C][K][H][N]
  const double* terminal; // [n_slots][K][N] of this chunk, or null = zeros
  double* returns_ev;     // [C][K] the object's own copy: the best kernel reads it
  double* returns;        // rows of this chunk [n_slots][K], or null
  double* rewards;        // [n_slots][K][H], or null
  double* farm_power;     // [n_slots][K][H], or null
  double* action_gradient;  // [n_slots][K][H][N], or null
  double* reward_gradient;  // [n_slots][K][H][N], or null
  double* state_gradient;   // [n_slots][K][N], or null
};

struct WfRetgradBestArgs {
  int n_slots, K;
  const double* returns_ev;  // [C][K]
  int* best;                 // [n_slots] of this chunk
};

extern "C" hipError_t wfk_launch_retgrad_layout(const WfRetgradLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_retgrad_reduce(const WfRetgradReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_retgrad_best(const WfRetgradBestArgs* a, hipStream_t s);
extern "C" hipError_t wfk_retgrad_func_attributes(int kernel, hipFuncAttributes* a);
