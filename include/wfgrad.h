/* wfgrad.h — yaw sensitivities on the device: the Jacobian of the per-turbine power with respect to every turbine's yaw and
 * its vector-Jacobian product — the gradient extension of libwfstep.so (include/wfstep.h).
 *
 * The flow probes, the yaw optimiser, the wind rose and the robust search all answer "what is the power at this yaw?".
 * This one answers "how does the power change when turbine i turns?": analytic policy gradients through the simulator,
 * per-agent credit assignment (how much of turbine j's power is owed to turbine i's yaw), any gradient-based optimiser.
 * FLORIS' scipy yaw optimiser gets the same from 2 N sequential float64 solves per farm.  This is THE PROJECT'S OWN
 * definition, not FLORIS' routine.  PARITY UNPINNED beyond the oracle: tests/grad_ref.py restates it in NumPy over the
 * float64 oracle.  The result is the DIFFERENCE QUOTIENT at a finite step h, not an analytic or adjoint derivative of the
 * step kernels: the model has kinks (the power table's knots, the overlap count), and h says at which scale they are seen.
 *
 * INPUTS for one farm under the wind the parent handle holds: a yaw row y (float32, N turbines, caller order), a step h > 0
 * in degrees (default 1), bounds lo < hi in degrees (default -45, 45: the range the float64 oracle is defined on, see
 * include/wfrobust.h), a cotangent row c (float32, N; default all ones).
 *
 * PERTURBED YAWS, computed in float64 and rounded ONCE to float32 (the step takes float32 yaw):
 *   y+_i = (float)min((double)y_i + h, hi)        y-_i = (float)max((double)y_i - h, lo)
 * DIVISOR  d_i = (double)y+_i - (double)y-_i, the difference actually applied: one-sided at a bound by itself.  Where
 *   d_i <= 0 (a yaw outside the bounds by h or more) every sensitivity of turbine i is exactly 0.
 * EVALUATOR ROWS  R = 2 N + 1 per farm: row 0 the yaw as given, row 2 i + 1 the yaw with y_i -> y+_i, row 2 i + 2 with
 *   y_i -> y-_i; every row under the farm's own wind (ws, wd).
 * JACOBIAN [N][N] double, W/deg:  J[i][j] = ((double)P_j(row 2 i + 1) - (double)P_j(row 2 i + 2)) / d_i, P_j the step's
 *   float32 per-turbine `power`.
 * GRADIENT (the vector-Jacobian product) [N] double:  G[i] = S_i / d_i, S_i = sum_j (double)c_j ((double)P+_j - (double)P-_j),
 *   the sum over j in caller order in float64, every product and sum rounded on its own (no fused multiply-add).  With
 *   c = 1 it is d(farm power) / d(yaw_i).
 * POWER [N] float32: row 0's per-turbine power — the forward value.
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs.
 *
 * An object belongs to a parent handle, reads it (layout, model, wind, kernel choice, resolve mode) and stores nothing in
 * it; it must be destroyed BEFORE it.  Like the robust extension it owns an EVALUATOR: a further wf_handle on the parent's
 * device and stream with the parent's model and layout, configured through the public ABI only.  Evaluator farm
 * e = slot R + row for chunk farm slots; chunk is the largest farm count with chunk R <= max_eval_farms and longer farm
 * lists run chunk after chunk.  Per chunk ONE lay-out kernel writes the [chunk][R][N] yaw block, every row's wind (read from
 * the parent's DEVICE wind) and the divisors; one wf_step on the evaluator solves the rows; ONE reduce kernel forms power,
 * gradient and Jacobian from the [chunk R][N] float32 powers.  A whole run is enqueued on the stream without a host round
 * trip between its launches.  (An evaluator is a handle like any other: the first step of a new configuration times its
 * kernel families once — wf_kernel_choice::calibrate — and that one call synchronises.)
 *
 * VERSION-1 LIMITS.  The evaluator is given device arrays, a wind per row, so it always runs on the ON-THE-FLY path, even
 * under a parent with one shared wind; a farm's R rows share one direction, and reaching the pair-table path by grouping
 * them is not done.  One step h and one pair of bounds for all turbines.  No second derivatives.  A parent with several
 * layouts or several turbine definitions is refused.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFGRAD_H
#define WFGRAD_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_GRAD_KERNELS 2

typedef struct wf_grad wf_grad;

int wf_grad_create(wf_handle* h, wf_grad** out);
int wf_grad_destroy(wf_grad* g);

/* Step, bounds and the evaluator: a new object holds h = 1, (-45, 45), strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = 2 N + 1 rows (N as set at the time
 *                   of the call, and checked again when a run starts); <= 0: the default 65 536
 * WF_E_INVALID: h not finite or not positive, bounds not finite or lo >= hi, max_eval_farms below R. */
int wf_grad_config(wf_grad* g, double h, double lo, double hi, int strict, int max_eval_farms);

/* Sensitivities of the listed farms at a given yaw, under the wind the parent holds at the time of the call.
 *   yaw        [n_farms][N] float, row i belongs to farms[i] (caller's turbine order), or NULL = zeros
 *   cotangent  [n_farms][N] float, or NULL = ones
 *   farms      [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   power      [n_farms][N] float       the forward value
 *   gradient   [n_farms][N] double      G [W/deg]
 *   jacobian   [n_farms][N][N] double   J [W/deg], J[i][j] = d P_j / d yaw_i
 * Any output pointer may be NULL.
 * on_device != 0: yaw, cotangent and the outputs are device pointers and the call only enqueues work on the parent's
 * stream — except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt (first
 * run, another max_eval_farms / strict / farm count below a chunk, a parent whose layout, model or kernel choice changed)
 * and when a `farms` list is given.
 * WF_E_INVALID: no wind set, a farm index out of range, max_eval_farms below R.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_grad_run(wf_grad* g, const float* yaw, const float* cotangent, int n_farms, const int* farms, float* power,
                double* gradient, double* jacobian, int on_device);

/* detail != 0: the following wf_grad_run calls record four HIP events per chunk, so that wf_grad_last_timing can split the
 * total into step and glue time (they cost a little stream time themselves).  Default 0: two events per run. */
int wf_grad_set_timing(wf_grad* g, int detail);

/* HIP-event milliseconds of the last wf_grad_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels (both 0 unless wf_grad_set_timing asked for the
 * split).  Pointers may be NULL. */
int wf_grad_last_timing(wf_grad* g, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/grad_timing.py).  Owned by the object. */
wf_handle* wf_grad_evaluator(wf_grad* g);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_GRAD_KERNELS][3] ints: rows wf_grad_layout_kernel, wf_grad_reduce_kernel (its LDS is
 * dynamic on top). */
int wf_grad_kernel_info(wf_grad* g, int* info);

const char* wf_grad_last_error(wf_grad* g);

#ifdef __cplusplus
}
#endif
#endif /* WFGRAD_H */
