// wf_polscen.h — what the two translation units of the policy-scenario extension (include/wfpolscen.h) share: the arguments of
// the three kernels of wf_polscen_kernels.hip and their launchers, called by wf_polscen_abi.hip.
//
// The run's block is the policy extension's (policy/wf_policy.h: WfPolicyRun, with M members and the chunk's path buffer), and
// the transpose, begin and advance kernels are that extension's: a chunk of C farm SLOTS holds K M rows per slot, evaluator farm
// e = (k M + m) C + slot, so that a policy's M C rows are contiguous and a tile of T consecutive rows of the advance kernel
// still belongs to one policy.  Slots beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output
// (WfSlots: ext/wf_ext_kernels.h); their paths are drawn like any other's, since their rows are solved.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfpolscen.h"
#include "../ensemble/wf_ensemble.h"
#include "../ext/wf_ext_kernels.h"
#include "../policy/wf_policy.h"

struct WfPolscenPathsArgs {
  WfSlots sl;
  WfEnsemble ens;         // the paths: seed, process, bounds, anchor, the parent's wind, M, H
  double* paths;          // [C][M][H][2] the chunk's paths: what the advance kernel reads
  double* wind_paths;     // [n_slots][M][H][2] of this chunk, or null
};

// what the two kernels after the last step need beside the run's block
struct WfPolscenReduceArgs {
  double* mret;                     // [K M C] the rows' member returns, evaluator order
  double* member_returns;           // the caller's [n][K][M], or null
  double *expected, *cvar, *score;  // the caller's [n][K], or null
  int* best;                        // the caller's [n], or null
  double lam;
  int q;                            // the tail: the q lowest member returns
};

// the returns kernel's tile: rows per workgroup, the odd strides of the reward tile, the LDS bytes
struct WfPolscenTile {
  int T, sp, sl, threads;
  size_t lds_bytes;
};
WfPolscenTile wf_polscen_tile(int N, int rows);

extern "C" hipError_t wfk_launch_polscen_paths(const WfPolscenPathsArgs* a, hipStream_t s);
// `host` is the run's block as uploaded to `dev`
extern "C" hipError_t wfk_launch_polscen_returns(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, const WfPolscenReduceArgs* x, hipStream_t s);
extern "C" hipError_t wfk_launch_polscen_stats(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, const WfPolscenReduceArgs* x, hipStream_t s);
extern "C" hipError_t wfk_polscen_func_attributes(int kernel, hipFuncAttributes* a);
