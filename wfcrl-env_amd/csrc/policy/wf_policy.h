// wf_policy.h — what the two translation units of the policy extension (include/wfpolicy.h) share: the network as the kernels
// see it, the block the four kernels of wf_policy_kernels.hip read their arguments from, the LDS plan of the advance kernel and the launchers,
// called by wf_policy_abi.hip.
//
// Layout of a chunk of C farm SLOTS with K rows each (K M under an ensemble of M members: WfPolicyRun below): evaluator farm
// e = k C + slot, so the rows of ONE policy are contiguous:
// a workgroup of the advance kernel serves a TILE of T consecutive slots of one policy — it streams that policy's weights once
// for its T rows, and its rows' power, load and local-wind blocks are contiguous [T][N] arrays.  Row (k, slot) holds, in round
// 0, the farm's current yaw under its current wind and, in round h + 1, the yaw after step h of policy k under wind h.  Slots
// beyond the chunk's farms (a ragged last chunk) repeat slot 0's farm and write no output (WfSlots: ext/wf_ext_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfpolicy.h"
#include "../ext/wf_ext_kernels.h"

// the network: widths, the offsets of every layer's weight block and bias in a parameter vector [P], what follows the layers
struct WfPolicyNet {
  int kind, L, act, fin, use_freewind, discrete;
  int P;
  int width[WF_POLICY_MAX_LAYERS + 1];  // width[0] = D, width[l + 1] = outputs of layer l
  int woff[WF_POLICY_MAX_LAYERS];       // layer l's weights at woff[l]: [out][in] as uploaded, [in][out] after the transpose
  int boff[WF_POLICY_MAX_LAYERS];       // ... and its bias [out]
  double out_scale;
};

// what a row carries from one launch to the next, beside its yaw (the evaluator's input row itself)
struct WfPolicyState {
  float* acc;     // [E][N] the accumulators
  double* ret;    // [E] the return so far
  double* disc;   // [E] g_h of the next reward to add
  int* gated;     // [E] closed gates so far
};

// the LDS of an advance block, in this order: three [T] doubles (the rows' normalisers, rewards, farm powers) and the reward
// tile pw [T][sp] + ld [T][sl] floats; then doubles x0 [MB][xs] and two activation buffers [MB][as] each; then floats obs
// [T][ds], act [T][N]; then ints ng [T].  MB is the number of network instances a pass holds: T (central: an instance is a
// row) or at most T N (shared: an instance is a turbine of a row).
struct WfPolicyPlan {
  int T, MB, threads;
  int xs, as, ds, sp, sl;
  size_t lds_bytes;
};

// What the launches of a run share, in DEVICE memory (uploaded once per run): the kernels read a field where a phase needs it.
// Passed by value instead, the block is fetched on entry and stays in scalar registers across the staged row rewards, which
// take nearly all of them: the compiler then spills (plan/wf_plan.h: WfPlanRun) — and the widths indexed by the layer would go
// to a private segment.
struct WfPolicyRun {
  WfPolicyNet net;
  WfPolicyPlan pl;
  int N, K, H;
  WfEnvView env;          // the parent's env: the state is read, never written
  const double *ws, *wd;  // the parent's wind ...
  int wind_stride;        // 0 shared, 1 per farm
  const double* ws_prev;  // ... or [B] the speed the next env step normalises by (null: the current one): step 0's
  float load_coef;
  double gamma;
  const float* params;    // [K][P] as the caller gave them
  float* wt;              // [K][P]: every weight block transposed to [in][out], every bias copied
  const double *shift, *scale;  // [D]
  float* yaw;             // [K][C][N] the evaluator's input: read (the yaw before step h), then overwritten (the yaw after it)
  const float *power_ev, *load_ev, *lws, *lwd;  // the last step's outputs: [K][C][N], [K][C][N][4], [K][C][N], [K][C][N]
  double *ews, *ewd;      // [K C] every row's wind: read (the wind the row was solved under), then — under `wind` — overwritten
  WfPolicyState st;
  // the caller's arrays, a block per listed farm: a slot's is sl.base + slot.  Any may be null
  const double* wind;     // [n][H][2] (speed, direction), or null = the parent's wind held
  double *returns, *rewards, *farm_power;  // [n][K], [n][K][H], [n][K][H]
  float *actions, *observations;           // [n][K][H][N], [n][K][H][3 N + 2]
  float* final_yaw;                        // [n][K][N]
  int *gated, *best;                       // [n][K], [n]
  // Under an ENSEMBLE (include/wfpolscen.h; wf_policy_run: M = 1, paths and first_action null): a policy has M C rows, row
  // j = m C + slot of policy k is evaluator farm k M C + j, the caller's blocks gain a member axis after K — [n][K][M]... —
  // and row (m, slot) is solved under paths[slot][m] instead of `wind`.  A tile is T consecutive rows j of one policy.
  int M;
  const double* paths;    // [C][M][H][2] the chunk's member paths (speed, direction) of tick h + 1, or null
  float* first_action;    // [n][K][N] step 0's raw action, written from member 0's rows, or null
};

// the advance kernel's tile for chunks of C slots: the rows one workgroup serves, from the LDS they need (56 KiB per block)
WfPolicyPlan wf_policy_plan(const WfPolicyNet& net, int N, int C);

// `host` is the run's block as uploaded to `dev`; round 1 .. H: the launch between step round - 1 and step round of the
// evaluator, which issues action h = round - 1
extern "C" hipError_t wfk_launch_policy_transpose(const WfPolicyRun* host, const WfPolicyRun* dev, hipStream_t s);
extern "C" hipError_t wfk_launch_policy_begin(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, hipStream_t s);
extern "C" hipError_t wfk_launch_policy_advance(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, int round, hipStream_t s);
extern "C" hipError_t wfk_launch_policy_reduce(const WfPolicyRun* host, const WfPolicyRun* dev, const WfSlots* sl, hipStream_t s);
extern "C" hipError_t wfk_policy_func_attributes(int kernel, hipFuncAttributes* a);
