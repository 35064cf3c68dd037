// wf_polsearch.h — what the two translation units of the policy-search extension (include/wfpolsearch.h) share: the arguments of
// the two kernels of wf_polsearch_kernels.hip and their launchers, called by wf_polsearch_abi.hip.
//
// The search keeps, from launch to launch: the candidates of two iterations, cand [2][K][P] — iteration i's are block i & 1, the
// scorer reads them there, and the advance that refits from them writes iteration i + 1's into the other block, so that no
// workgroup overwrites what another still reads —; the scorer's output scores [n][K]; the tile sums [T][K], T = ceil(n / 256).
// Mean and incumbent live in the candidates (rows 1 and 0); the widths are recomputed from the elites by whoever needs them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfpolsearch.h"

#define WF_POLSEARCH_THREADS 256
#define WF_POLSEARCH_SUB 32          // list positions a tile's workgroup holds in LDS at a time: [32][K] doubles, <= 16 KiB
#define WF_POLSEARCH_ROWS 8          // candidate rows a workgroup of the advance writes: the refit is computed once per slice of 8
#define WF_POLSEARCH_PASS_BLOCKS 32  // workgroups along p per slice: a pass is 8192 elements, longer vectors take several (the walk
                                     // over the K rows is a chain of loads: with 4 it cost 0.35 ms per launch at K = 64, P = 24 912)

// What the launches of a run share: passed by value.
struct WfPolSearchRun {
  int K, P, E, I, n, T;
  double sigma_min;
  unsigned long long seed;
  const float *mean0, *sigma0;  // [P]
  float* cand;                  // [2][K][P]
  const double* scores;         // [n][K] the scorer's output of the iteration
  double* tile;                 // [T][K]
  // the caller's outputs; any may be null
  float *best_params, *mean, *sigma;     // [P]
  double *best_fitness, *init_fitness;   // [1]
  double* fitness;                       // [I][K]
  int* winner;                           // [I]
  float* candidates;                     // [I][K][P]
  float* sigma_history;                  // [I][P]
  double* farm_scores;                   // [I][n][K]
};

// iteration i's scores -> tile sums (and farm_scores[i])
extern "C" hipError_t wfk_launch_polsearch_tiles(const WfPolSearchRun* r, int i, hipStream_t s);
// launch v = 0 .. I: refits from iteration v - 1 (v > 0; v = 0 seeds from mean0, sigma0), then lays out iteration v (v < I) or
// writes the outputs (v = I)
extern "C" hipError_t wfk_launch_polsearch_advance(const WfPolSearchRun* r, int v, hipStream_t s);
extern "C" hipError_t wfk_polsearch_func_attributes(int kernel, hipFuncAttributes* a);
