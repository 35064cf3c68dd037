/* wfyawopt.h — batched static yaw optimisation on the device: the yaw-optimiser extension of libwfstep.so (include/wfstep.h).
 *
 * Wake-steering work asks "what is the best static yaw for this wind, and how much of that gain did my agent recover?".
 * The usual answer is a coordinate search over the steady-state model (FLORIS users know one as "serial refine").  This is
 * THE PROJECT'S OWN coordinate search, in that spirit; it is not pinned to FLORIS' optimiser.
 *
 * The algorithm (tests/yawopt_ref.py restates it in NumPy over the float64 oracle):
 *   inputs   bounds lo < hi [deg]; passes K_0 .. K_{P-1}, 1 <= P <= 4, K_0 >= 2, K_0 <= 31, K_p in 1..15 for p >= 1;
 *            a start yaw0 per farm (default zeros).
 *   order    every farm visits its turbines in ascending wind-aligned x' (the float64 rotation about the layout's
 *            bounding-box centre that wf_set_wind performs), exact ties by ascending caller index.
 *   pass 0   for each turbine in visit order the candidates are c_k = lo + k h_0, h_0 = (hi - lo) / (K_0 - 1), k = 0 .. K_0-1;
 *            the INCUMBENT (the turbine's current value) is always one more candidate; every other turbine stays at its
 *            current best.
 *   pass p   with h = h_{p-1}: c_j = inc - h + (j + 1) s, s = 2 h / (K_p + 1), j = 0 .. K_p-1, plus the incumbent; h_p = s.
 *   every candidate is clipped to [lo, hi] in float64 and rounded ONCE to float32 (the step takes float32 yaw); an incumbent
 *            is never clipped (a start value outside the bounds stays until something better is found).
 *   decision a candidate replaces the incumbent only when its farm power is STRICTLY greater; among equal maxima the lowest
 *            index wins.  Farm power = the step's per-turbine `power` summed in caller order in float64.  It never decreases.
 *   Every turbine is visited in every pass (no skip heuristic): P N visits of K_p + 1 farm evaluations each.
 *
 * An optimiser object belongs to a parent handle, reads it (layout, model, wind, kernel choice, resolve mode) and stores
 * nothing in it; it must be destroyed BEFORE it.  It owns an EVALUATOR: a second wf_handle on the parent's device and stream
 * with the parent's model and layout and a batch of chunk x (K_max + 1) farms, chunk the largest farm count with
 * chunk x (K_max + 1) <= max_eval_farms; longer farm lists run chunk after chunk.  Candidate evaluation is wf_step on the
 * evaluator; a visit whose pass has fewer candidates than K_max fills the spare rows with the incumbent.  Around it, per
 * visit, ONE glue kernel sums the previous visit's powers, picks the winners and writes the next visit's yaw block; a whole
 * run is enqueued on the stream without a host round trip between its launches.  (The evaluator is a handle like any other:
 * the first step of a new configuration times its kernel families once — wf_kernel_choice::calibrate — and that one call
 * synchronises.)
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFYAWOPT_H
#define WFYAWOPT_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_YAWOPT_MAX_PASSES 4
#define WF_YAWOPT_MAX_K0 31
#define WF_YAWOPT_MAX_K 15

typedef struct wf_yawopt wf_yawopt;

int wf_yawopt_create(wf_handle* h, wf_yawopt** out);
int wf_yawopt_destroy(wf_yawopt* o);

/* Bounds, passes and the evaluator.  A new object holds (-25, 25), passes (5, 4), strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every farm in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch (>= K_max + 1); <= 0: the default 65 536
 * WF_E_INVALID: lo >= hi or not finite, n_passes outside 1..4, K_0 outside 2..31, a later K outside 1..15. */
int wf_yawopt_config(wf_yawopt* o, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms);

/* Optimise the listed farms under the wind the parent holds at the time of the call.
 *   yaw0       [n_farms][N] start, row i belongs to farms[i] (caller's turbine order), or NULL = zeros
 *   farms      [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   yaw_opt    [n_farms][N]  the best yaw found
 *   power_opt  [n_farms]     its farm power [W] as the evaluator computed it
 *   power_init [n_farms]     the farm power at yaw0
 * on_device != 0: yaw0 and the outputs are device pointers and the call only enqueues work on the parent's stream — except
 * that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt (first run, another
 * K_max / max_eval_farms / strict, a parent whose layout, model or kernel choice changed) and when a `farms` list is given.
 * WF_E_INVALID: no wind set, a farm index out of range.  WF_E_UNSUPPORTED (version 1): a parent with several layouts
 * (wf_set_layouts*) or with turbine definitions (wf_set_turbine_types). */
int wf_yawopt_run(wf_yawopt* o, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                  float* power_init, int on_device);

/* detail != 0: the following runs record a HIP event around EVERY launch, so that wf_yawopt_last_timing can split the total
 * into step and glue time (two events per visit: they cost a little stream time themselves).  Default 0: two events per run. */
int wf_yawopt_set_timing(wf_yawopt* o, int detail);

/* HIP-event milliseconds of the last wf_yawopt_run (synchronises): from its first to its last launch; of these the wf_step
 * calls on the evaluator and the glue kernels (both 0 unless wf_yawopt_set_timing asked for the split).  Pointers may be NULL. */
int wf_yawopt_last_timing(wf_yawopt* o, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very
 * batch the optimiser uses (tools/yawopt_timing.py).  Owned by the optimiser. */
wf_handle* wf_yawopt_evaluator(wf_yawopt* o);

const char* wf_yawopt_last_error(wf_yawopt* o);

#ifdef __cplusplus
}
#endif
#endif /* WFYAWOPT_H */
