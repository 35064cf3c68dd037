/* wfrobust.h — wind-direction uncertainty on the device: expected power over a set of direction errors and the yaw search
 * that maximises it — the robust extension of libwfstep.so (include/wfstep.h).
 *
 * A yaw table optimised for a sharp wind direction over-steers: the measured direction is uncertain by a few degrees, the
 * optimum of a row flips sign across the row's axis, and part of the promised gain becomes a loss.  The usual remedy is to
 * maximise the EXPECTED power over a distribution of direction errors.  FLORIS users know this as `UncertaintyInterface`
 * (std_wd, pmf_res, pdf_cutoff, fix_yaw_in_relative_frame) around the object the reference's FlorisInterface wraps.  This is
 * THE PROJECT'S OWN definition, not FLORIS' routine.  PARITY UNPINNED beyond the oracle: tests/robust_ref.py restates it in
 * NumPy over the float64 oracle.
 *
 * MEMBERS.  M direction offsets delta[m] (degrees, finite, strictly ascending) with weights weight[m] >= 0 whose sum is
 * positive, 1 <= M <= WF_ROBUST_MAX_MEMBERS.  The weights are normalised once on the host in float64:
 * w[m] = weight[m] / (weight[0] + weight[1] + ...), the sum taken in index order.
 *
 * FRAME.
 *   WF_ROBUST_RELATIVE  every member is stepped with the yaw as given: the turbine follows the true wind, only the
 *                       controller's knowledge is uncertain.
 *   WF_ROBUST_FIXED     the nacelle stays where the nominal direction put it.  Yaw is the counter-clockwise rotation of the
 *                       nacelle away from the wind and wd grows clockwise, so a nacelle fixed in the ground frame meets
 *                       member m at yaw + delta[m]: the step takes (float)((double)yaw + delta[m]), rounded once.
 *
 * EXPECTED POWER of a farm at yaw row y under its nominal wind (ws, wd): E = sum_m w[m] P_m, P_m the step's per-turbine
 * `power` at (ws, wd + delta[m]) and the member's yaw, added in caller order in float64; the member sum runs in index
 * order in float64, every product and sum rounded on its own (no fused multiply-add).  The expected power of a turbine is
 * the same sum over its own float32 powers.  No floating-point atomics: two runs give identical bits.
 *
 * ROBUST SEARCH.  The coordinate search of include/wfyawopt.h, word for word — visit order from the NOMINAL direction, the
 * pass grids, clipping, an incumbent that is never clipped, strictly-greater decisions, the lowest index among equals —
 * with "farm power" replaced by E.  Bounds apply to the nominal yaw; in the FIXED frame a member's yaw may lie outside them.
 * (The float64 oracle the tests compare with is defined up to |yaw| = 45 deg: keep hi + delta[M-1] and lo + delta[0] inside.)
 *
 * An object belongs to a parent handle, reads it (layout, model, wind, kernel choice, resolve mode) and stores nothing in
 * it; it must be destroyed BEFORE it.  Like the yaw optimiser it owns EVALUATORS (one for wf_robust_evaluate, one for
 * wf_robust_optimize): further wf_handles on the parent's device and stream with the parent's model and layout, configured
 * through the public ABI only.  Evaluator farm e = (slot R + row) M + member, R = K_max + 1 candidate rows (R = 1 for
 * wf_robust_evaluate), for chunk farm slots; chunk is the largest farm count with chunk R M <= max_eval_farms and longer
 * farm lists run chunk after chunk.  Per chunk one lay-out kernel writes every row's wind (ws, wd + delta[m], read from the
 * parent's DEVICE wind); per visit one kernel adds each row's N float32 powers to one double and ONE advance kernel forms E
 * for the visit's K + 1 candidates, picks the winner and writes the next visit's [R][M][N] yaw block.  A whole run is
 * enqueued on the stream without a host round trip between its launches.  (An evaluator is a handle like any other: the
 * first step of a new configuration times its kernel families once — wf_kernel_choice::calibrate — and that one call
 * synchronises.)
 *
 * VERSION-1 LIMITS.  The evaluator is given device arrays, a wind per row, so it always runs on the ON-THE-FLY path, even
 * under a parent with one shared wind; grouping the rows by member direction to reach the pair-table path is not done.  No
 * speed uncertainty.  No wind rose under uncertainty (include/wfrose.h takes no members).  A parent with several layouts or
 * several turbine definitions is refused.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFROBUST_H
#define WFROBUST_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_ROBUST_MAX_MEMBERS 33
#define WF_ROBUST_RELATIVE 0
#define WF_ROBUST_FIXED 1
#define WF_ROBUST_MAX_PASSES 4 /* the limits of wf_yawopt_config */
#define WF_ROBUST_MAX_K0 31
#define WF_ROBUST_MAX_K 15
#define WF_ROBUST_KERNELS 5

typedef struct wf_robust wf_robust;

int wf_robust_create(wf_handle* h, wf_robust** out);
int wf_robust_destroy(wf_robust* r);

/* The member set: HOST arrays delta[M], weight[M], validated as stated above, copied; synchronises.
 * WF_E_INVALID: M outside 1..33, a delta that is not finite or not strictly ascending, a weight that is negative or not
 * finite, weights that are all zero, a frame other than WF_ROBUST_RELATIVE / WF_ROBUST_FIXED. */
int wf_robust_set_members(wf_robust* r, int M, const double* delta, const double* weight, int frame);

/* Bounds, passes and the evaluators: the limits and defaults of wf_yawopt_config — a new object holds (-25, 25), passes
 * (5, 4), strict 0, 65 536 evaluator farms.  max_eval_farms must hold one farm's rows, (K_max + 1) M (M as set at the time
 * of the call, and checked again when a run starts); <= 0: the default 65 536. */
int wf_robust_config(wf_robust* r, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms);

/* Expected power of the listed farms at a given yaw, under the wind the parent holds at the time of the call.
 *   yaw                     [n_farms][N] float, row i belongs to farms[i] (caller's turbine order), or NULL = zeros
 *   farms                   [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms
 *   expected_power          [n_farms] double        E [W]
 *   expected_turbine_power  [n_farms][N] double     the same per turbine
 *   member_power            [n_farms][M] float      P_m, rounded once
 * Any output pointer may be NULL.  on_device and the drains: as wf_robust_optimize. */
int wf_robust_evaluate(wf_robust* r, const float* yaw, int n_farms, const int* farms, double* expected_power,
                       double* expected_turbine_power, float* member_power, int on_device);

/* The robust search on the listed farms.  yaw0, farms, yaw_opt, power_opt, power_init have the meaning they have in
 * wf_yawopt_run; the two powers are E at the optimum and at yaw0, rounded once to float32.
 * on_device != 0: yaw0 and the outputs are device pointers and the call only enqueues work on the parent's stream — except
 * that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt (first run, another
 * K_max / M / max_eval_farms / strict, a parent whose layout, model or kernel choice changed) and when a `farms` list is
 * given.
 * WF_E_INVALID: no wind set, no members set, a farm index out of range, max_eval_farms below one farm's rows.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_robust_optimize(wf_robust* r, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                       float* power_init, int on_device);

/* detail != 0: the following wf_robust_optimize calls record a HIP event around EVERY launch group, so that
 * wf_robust_last_timing can split the total into step and glue time (they cost a little stream time themselves).
 * Default 0: two events per run.  wf_robust_evaluate always records its four events per chunk. */
int wf_robust_set_timing(wf_robust* r, int detail);

/* HIP-event milliseconds of the last wf_robust_optimize or wf_robust_evaluate (synchronises): from its first to its last
 * launch; of these the evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels (for an optimisation both 0
 * unless wf_robust_set_timing asked for the split).  Pointers may be NULL. */
int wf_robust_last_timing(wf_robust* r, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle of wf_robust_optimize (NULL before the first run): for introspection and for timing a plain wf_step
 * loop on the very batch the search uses (tools/robust_timing.py).  Owned by the object. */
wf_handle* wf_robust_evaluator(wf_robust* r);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_ROBUST_KERNELS][3] ints: rows wf_robust_order_kernel, wf_robust_layout_kernel,
 * wf_robust_rowsum_kernel, wf_robust_advance_kernel (the LDS of these two is dynamic on top), wf_robust_expect_kernel. */
int wf_robust_kernel_info(wf_robust* r, int* info);

const char* wf_robust_last_error(wf_robust* r);

#ifdef __cplusplus
}
#endif
#endif /* WFROBUST_H */
