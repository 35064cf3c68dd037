/* wfrose.h — expected power over a wind rose and a yaw look-up-table controller on the device: the rose extension of
 * libwfstep.so (include/wfstep.h).
 *
 * Wake-steering results are quoted as expected power / AEP over a (direction x speed) frequency table, with and without
 * steering, and the baseline controller is a yaw LOOK-UP TABLE over (wind direction, wind speed), interpolated at the
 * current wind and tracked under the yaw-rate limit.  FLORIS users know the first as `get_farm_AEP(freq, yaw_angles=...)`
 * on the object the reference's FlorisInterface wraps.  This is THE PROJECT'S OWN interpolation and reduction, not FLORIS'
 * AEP routine.  PARITY UNPINNED beyond the oracle: tests/rose_ref.py restates it in NumPy over the float64 oracle.
 *
 * THE YAW TABLE.  T[Dt][St][N] float32, degrees, caller's turbine order, with a direction axis twd[Dt] (degrees, strictly
 * ascending, inside [0, 360)) and a speed axis tws[St] (m/s, strictly ascending, > 0); Dt >= 1, St >= 1.  The yaw at a wind
 * (ws, wd), in float64:
 *   1. wd is reduced to [0, 360) as wf_set_wind reduces it: fmod(wd, 360), + 360 when negative.
 *   2. direction bracket: k with twd[k] <= wd < twd[k+1], k1 = k + 1, fd = (wd - twd[k]) / (twd[k+1] - twd[k]).  The axis is
 *      CIRCULAR: between twd[Dt-1] and twd[0] + 360 the bracket is (Dt-1, 0), fd = (wd - twd[Dt-1]) / (twd[0] + 360 - twd[Dt-1]);
 *      a wd below twd[0] is treated as wd + 360 in that same bracket.  Dt == 1: constant in direction (fd = 0).
 *   3. speed bracket: ws is clamped to [tws[0], tws[St-1]]; j = the last node <= ws, j1 = min(j + 1, St - 1),
 *      fs = (ws - tws[j]) / (tws[j1] - tws[j]), or 0 when j1 == j (the top node, St == 1).
 *   4. WF_ROSE_LINEAR    (1 - fd) ((1 - fs) T[k][j] + fs T[k][j1]) + fd ((1 - fs) T[k1][j] + fs T[k1][j1]), every product and
 *                        sum rounded on its own (no fused multiply-add);
 *      WF_ROSE_NEAREST   T[fd > 0.5 ? k1 : k][fs > 0.5 ? j1 : j]: the node with the larger weight per axis, an exact half
 *                        goes to the lower index of the bracket.
 *   5. the result is rounded ONCE to float32.
 * Known weakness of LINEAR: the optimal yaw of a row flips sign where the wind crosses the row's axis, and a blend of two
 * nodes on either side passes through zero — on a row of three turbines 5 D apart the optimum is -22.5 deg at 265 deg next
 * to +25 deg at 270 deg, and half way between them the blend steers hardly at all.  That is why NEAREST exists (and why a
 * table wants direction nodes closer than the width of that flip).
 *
 * THE ROSE.  Directions wd[D], speeds ws[S] and frequencies freq[D][S] >= 0 (any scale: nothing is normalised here).  A
 * condition with ws < cut_in or ws > cut_out counts as ZERO power, like FLORIS (cut_in_wind_speed = 0.001,
 * cut_out_wind_speed = None).
 *
 * A rose object belongs to a parent handle, reads it (layout, model, wind, env parameters and yaw state, kernel choice,
 * resolve mode) and stores nothing in it; it must be destroyed BEFORE it.  Like the yaw optimiser (include/wfyawopt.h) it
 * owns an EVALUATOR: a second wf_handle on the parent's device and stream with the parent's model and layout, configured
 * through this public ABI only.  An evaluation lays the (direction, case, speed) rows out direction-major in chunks of at
 * most max_eval_farms rows (a ragged last chunk repeats its first row), and per chunk enqueues one lay-out kernel (each
 * row's wind and yaw: the look-up above for a table case), wf_set_wind_counts + wf_step on the evaluator, and two reducing
 * kernels.  The reduction is deterministic: a row's N float32 powers are added in caller order in float64, the weighted
 * sums run over (d, s) in index order in float64 by one thread per sum, a sum that spans chunks carries its partial in a
 * device buffer in chunk order; no floating-point atomics.  Two runs give identical bits, and so does another chunk size.
 * (The evaluator is a handle like any other: the first step of a new configuration times its kernel families once —
 * wf_kernel_choice::calibrate — and that one call synchronises.)
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFROSE_H
#define WFROSE_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_ROSE_SLOTS 4 /* table slots 0 .. 3 */
#define WF_ROSE_LINEAR 0
#define WF_ROSE_NEAREST 1
#define WF_ROSE_CASE_ZERO 0  /* every turbine at 0 deg; case_arg ignored */
#define WF_ROSE_CASE_FIXED 1 /* row case_arg of fixed_yaw, under every condition */
#define WF_ROSE_CASE_TABLE 2 /* the table in slot case_arg, looked up at every condition */
#define WF_ROSE_MAX_CASES 64
#define WF_ROSE_KERNELS 4

typedef struct wf_rose wf_rose;

int wf_rose_create(wf_handle* h, wf_rose** out);
int wf_rose_destroy(wf_rose* r);

/* Store a yaw table in `slot` (0 .. WF_ROSE_SLOTS - 1); the object keeps its own device copy.
 *   twd [Dt], tws [St] double;  T [Dt][St][N] float, N the parent's turbine count;  interp WF_ROSE_LINEAR / WF_ROSE_NEAREST
 * Host arrays (on_device == 0) are validated — the axes as defined above, every T finite — and the call returns after the
 * copy (it synchronises); device arrays are copied as they are, asynchronously on the parent's stream (the stream is
 * drained first only when the slot's buffers have to grow).  WF_E_INVALID: a bad slot, size, axis, value or interp. */
int wf_rose_set_table(wf_rose* r, int slot, int Dt, const double* twd, int St, const double* tws, const float* T, int interp,
                      int on_device);

/* The rose wf_rose_evaluate works on: HOST arrays, validated (wd finite, ws > 0, freq finite and >= 0), copied; synchronises.
 *   cut_in   conditions with ws < cut_in count as zero power
 *   cut_out  conditions with ws > cut_out count as zero power; <= 0: no cut-out */
int wf_rose_set_rose(wf_rose* r, int D, const double* wd, int S, const double* ws, const double* freq, double cut_in,
                     double cut_out);

/* The evaluator, with the meaning the two arguments have in wf_yawopt_config.  A new object holds strict 0, 65 536 rows.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch = rows per chunk (>= 1); <= 0: the default 65 536 */
int wf_rose_config(wf_rose* r, int strict, int max_eval_farms);

/* Evaluate n_cases yaw settings over the rose.
 *   case_kind, case_arg  [n_cases] HOST arrays (WF_ROSE_CASE_*), 1 <= n_cases <= WF_ROSE_MAX_CASES
 *   fixed_yaw            [n_fixed][N] float, n_fixed = 1 + the largest case_arg of a FIXED case; may be NULL without one
 *   weighted_power          [C] double          sum over (d, s) of freq P_farm [W], NOT normalised
 *   weighted_turbine_power  [C][N] double       the same per turbine, caller's order
 *   condition_power         [C][D][S] float     the farm power of every condition (0 for a masked one)
 * Any output pointer may be NULL.  on_device != 0: fixed_yaw and the outputs are device pointers and the call only
 * enqueues work on the parent's stream — except that it drains the stream first when a buffer has to grow, when the
 * evaluator has to be rebuilt (first run, another chunk size / strict, a parent whose layout, model or kernel choice
 * changed) and when the case list differs from the previous call's (it is uploaded from a host copy).
 * WF_E_INVALID: no rose, a bad case, a table case whose slot is empty.  WF_E_UNSUPPORTED (version 1): a parent with
 * several layouts (wf_set_layouts*) or with turbine definitions (wf_set_turbine_types). */
int wf_rose_evaluate(wf_rose* r, int n_cases, const int* case_kind, const int* case_arg, const float* fixed_yaw,
                     double* weighted_power, double* weighted_turbine_power, float* condition_power, int on_device);

/* The look-up-table controller, per farm of the parent: the table of `slot` looked up at the farm's CURRENT wind (what
 * wf_get_wind reports, read on the device).
 *   target_yaw [B][N] float  the looked-up yaw clipped to the env's (yaw_lo, yaw_hi)
 *   action     [B][N] float  what wf_env_step takes to get there from the fused env's current yaw state, under wf_env_config:
 *                            continuous: clip(target - yaw, -yaw_step, +yaw_step) in float32
 *                            discrete:   2 if target - yaw >= yaw_step / 2, 0 if <= -yaw_step / 2, else 1
 * Either pointer may be NULL.  Reads the env state, never writes it.  on_device != 0: device pointers, enqueue only.
 * WF_E_INVALID: no wind, an empty slot, no env state (wf_env_config + wf_env_reset come first).  WF_E_UNSUPPORTED as above. */
int wf_rose_policy(wf_rose* r, int slot, float* target_yaw, float* action, int on_device);

/* HIP-event milliseconds of the last wf_rose_evaluate (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the lay-out and reducing kernels.  Pointers may be NULL. */
int wf_rose_last_timing(wf_rose* r, float* total_ms, float* step_ms, float* glue_ms);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_ROSE_KERNELS][3] ints: rows wf_rose_layout_kernel, wf_rose_rowsum_kernel (whose LDS is
 * dynamic on top), wf_rose_accumulate_kernel, wf_rose_policy_kernel. */
int wf_rose_kernel_info(wf_rose* r, int* info);

const char* wf_rose_last_error(wf_rose* r);

#ifdef __cplusplus
}
#endif
#endif /* WFROSE_H */
