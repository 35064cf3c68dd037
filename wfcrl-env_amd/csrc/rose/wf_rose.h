// wf_rose.h — what the two translation units of the rose extension (include/wfrose.h) share: the arguments of the four
// kernels of wf_rose_kernels.hip and their launchers, called by wf_rose_abi.hip.
//
// Rows of an evaluation: global row g = (d C + c) S + s — direction-major, so that neighbouring rows share a direction —
// for direction d, case c, speed s.  A chunk holds the rows [row0, row0 + n_rows) in the evaluator's farms 0 .. n_rows - 1;
// farms n_rows .. E - 1 of a ragged last chunk repeat the chunk's first row and are never read back.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfrose.h"

// one table slot, device pointers (T == null: empty)
struct WfRoseTable {
  const double *twd, *tws;
  const float* T;  // [Dt][St][N]
  int Dt, St, interp;
};

// Read access to a rose object's tables for an object created on it (rollout/): slot's device table as the kernels take it
// (T == null: empty) and the turbine count it was set for.  The pointers stay valid until the slot is set again or the rose
// object is destroyed; the work that reads them is enqueued on the same stream as wf_rose_set_table's copies.
struct wf_rose;
struct wf_handle;
namespace wfi {
WfRoseTable rose_device_table(const wf_rose* r, int slot, int* N);
wf_handle* rose_parent(const wf_rose* r);
}  // namespace wfi

struct WfRoseShape {
  int D, C, S, N;
  int row0, n_rows, E;  // this chunk
};

struct WfRoseLayoutArgs {
  WfRoseShape sh;
  const double *wd, *ws;   // the rose's axes [D], [S]
  const int* cases;        // [2][C] kind, arg
  const float* fixed_yaw;  // [n_fixed][N]
  WfRoseTable tab[WF_ROSE_SLOTS];
  double *ews, *ewd;       // [E] the rows' wind
  float* yaw;              // [E][N] the rows' yaw
};

struct WfRoseReduceArgs {
  WfRoseShape sh;
  const double *ws, *freq;  // [S], [D][S]
  double cut_in, cut_out;   // cut_out <= 0: none
  const float* power;       // [E][N] the evaluator's output
  double* rowsum;           // [E] farm power of the chunk's rows, masked
  float* condition_power;   // [C][D][S] or null
  double *acc_turbine, *acc_farm;  // [C][N], [C] partial weighted sums, carried from chunk to chunk
  int first;                // the evaluation's first chunk: the partials start from zero
};

struct WfRosePolicyArgs {
  WfRoseTable tab;
  int B, N, wind_stride;   // wind_stride 0: one wind for the batch
  const double *ws, *wd;   // the parent's wind
  const float* yaw_state;  // [B][N] the fused env's yaw
  float lo, hi, step;
  int discrete;
  float *target, *action;  // [B][N], either may be null
};

extern "C" hipError_t wfk_launch_rose_layout(const WfRoseLayoutArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_rose_rowsum(const WfRoseReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_rose_accumulate(const WfRoseReduceArgs* a, hipStream_t s);
extern "C" hipError_t wfk_launch_rose_policy(const WfRosePolicyArgs* a, hipStream_t s);
extern "C" hipError_t wfk_rose_func_attributes(int kernel, hipFuncAttributes* a);
