/* wflookahead.h — multi-step look-ahead returns of action sequences on the device: the discounted return the env would pay
 * over the next H steps for each of K candidate action sequences — the lookahead extension of libwfstep.so
 * (include/wfstep.h).
 *
 * The env is sequential: a yaw moves at most yaw_step per step and the actuation budget then silences a turbine that has
 * moved too much, so reaching a wake-steering optimum takes several steps, the first of which lower the reward.  The credit
 * extension (include/wfcredit.h) is the ONE-step counterfactual of the reward; this one gives the n-step return of whole
 * action sequences from the current env state — what a shooting / MPPI / CEM planner, an n-step return of a candidate
 * policy or a multi-step baseline needs.  The transition (gate, increment, clip) does not depend on the wake solve, so the
 * yaw of every step of the horizon is known before any farm is solved: the K H solves of a farm are independent rows of ONE
 * batched step.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle: tests/lookahead_ref.py restates
 * it in NumPy over the float64 oracle.
 *
 * INPUTS per farm b, under the parent's wf_env_config and env state (yaw y, accumulator acc, move counter moves), which is
 * READ ONLY here:
 *   actions [n_farms][K][H][N] float32, the env's action encoding (continuous or discrete as configured), caller's turbine
 *           order; 1 <= H <= WF_LOOKAHEAD_MAX_H, K >= 1, K H <= WF_LOOKAHEAD_MAX_ROWS
 *   wind    [n_farms][H][2] double (speed, direction), the wind step h is solved under; NULL = the parent's current wind of
 *           the farm, held over the horizon — also under a parent in series mode, unless wf_lookahead_set_series
 *           (include/wfseries.h) asks for the series' coming rows, which are then read on the device
 *   gamma   double, finite, in [0, 1]
 *
 * TRAJECTORY of sequence k: start from (y, acc, moves) of the farm; for h = 0 .. H-1 the fused env step's transition, in the
 * same float32 operations in the same order:
 *   frac = acc / rate / (moves + 1) / dt, every division correctly rounded; frac >= budget zeroes the RAW action (in the
 *   discrete encoding that means "down": the reference's quirk is kept); discrete: a = (a - 1) step, continuous: a clipped to
 *   +-step; y = clip(y + a, lo, hi); acc += |a|; moves += 1.
 * EVALUATOR ROWS  R = K H per farm: row k H + h holds the yaw AFTER step h of sequence k, under wind h.
 * ROW REWARD, float64, as the credit extension forms it:  psum = the row's N float32 powers added in caller order; lsum = the
 *   absolute values of its 4 N float32 load values added in memory order;
 *     r = psum / N / 1e6 * 1e3 / (wr wr wr) - load_coef lsum / (4 N)
 *   evaluated left to right.  wr is the free-stream speed BEFORE the step: for h = 0 what the parent's next wf_env_step
 *   would normalise by — what wf_env_set_prev_wind (or a series tick) left for it, else the farm's current speed; it is NOT
 *   consumed —, for h >= 1 the speed of wind h - 1.
 * RETURN  g_0 = 1, g_h = g_{h-1} gamma;  ret = sum_h g_h r_h added in ascending h, product and sum rounded separately.
 * OUTPUTS (any may be NULL)
 *   returns    [n_farms][K] double
 *   rewards    [n_farms][K][H] double
 *   farm_power [n_farms][K][H] double (psum, W)
 *   final_yaw  [n_farms][K][N] float32, the yaw after step H - 1
 *   best       [n_farms] int, the sequence of the largest return, the lowest index among equal maxima
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs.
 *
 * ACCURACY.  A row's reward carries the step's per-turbine tolerance (1e-4 of the power in the default mode): returns of two
 * sequences closer than the sum of their bounds are not ordered reliably, and `best` may then name either.  strict != 0 solves
 * every row in float64 (validation, near-equal candidates); the default mode serves planners and training loops.
 *
 * An object belongs to a parent handle, reads it (layout, model, wind, env parameters and env state, kernel choice, resolve
 * mode) and stores nothing in it; it must be destroyed BEFORE it.  It owns an EVALUATOR: a further wf_handle on the parent's
 * device and stream.  Evaluator farm e = slot R + row; chunk is the largest farm count with chunk R <= max_eval_farms and
 * longer farm lists run chunk after chunk.  Per chunk ONE lay-out kernel walks the trajectories and writes the [chunk][R][N]
 * yaw block, every row's wind and final_yaw; wf_set_wind_counts and one wf_step on the evaluator write power and load; ONE
 * reduce kernel forms the outputs.  A whole run is enqueued without a host round trip between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator is given device arrays, a wind per row, so it always runs on the ON-THE-FLY path.  A
 * parent with several layouts or several turbine definitions is refused.  No per-turbine power of the rows.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFLOOKAHEAD_H
#define WFLOOKAHEAD_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_LOOKAHEAD_KERNELS 2
#define WF_LOOKAHEAD_MAX_H 64
#define WF_LOOKAHEAD_MAX_ROWS 4096

typedef struct wf_lookahead wf_lookahead;

int wf_lookahead_create(wf_handle* h, wf_lookahead** out);
int wf_lookahead_destroy(wf_lookahead* l);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = K H rows (checked when a run starts,
 *                   where K and H are known); <= 0: the default 65 536 */
int wf_lookahead_config(wf_lookahead* l, int strict, int max_eval_farms);

/* Look-ahead returns of the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   actions     [n_farms][K][H][N] float, block i belongs to farms[i]
 *   wind        [n_farms][H][2] double, or NULL = the parent's current wind held
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   returns, rewards, farm_power, final_yaw, best   as above; any may be NULL
 * on_device != 0: actions, wind and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_credit_run).
 * WF_E_INVALID: no wind set, no env state (wf_env_config and wf_env_reset come first), actions == NULL, H outside
 * 1 .. WF_LOOKAHEAD_MAX_H, K < 1, K H > WF_LOOKAHEAD_MAX_ROWS, gamma outside [0, 1] or not finite, a farm index out of range,
 * max_eval_farms below K H.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_lookahead_run(wf_lookahead* l, const float* actions, int K, int H, const double* wind, double gamma, int n_farms,
                     const int* farms, double* returns, double* rewards, double* farm_power, float* final_yaw, int* best,
                     int on_device);

/* detail != 0: the following wf_lookahead_run calls record four HIP events per chunk, so that wf_lookahead_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_lookahead_set_timing(wf_lookahead* l, int detail);

/* HIP-event milliseconds of the last wf_lookahead_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels (both 0 unless wf_lookahead_set_timing asked for the
 * split).  Pointers may be NULL. */
int wf_lookahead_last_timing(wf_lookahead* l, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/lookahead_timing.py).  Owned by the object. */
wf_handle* wf_lookahead_evaluator(wf_lookahead* l);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_LOOKAHEAD_KERNELS][3] ints: rows wf_lookahead_layout_kernel, wf_lookahead_reduce_kernel
 * (their LDS is dynamic). */
int wf_lookahead_kernel_info(wf_lookahead* l, int* info);

const char* wf_lookahead_last_error(wf_lookahead* l);

#ifdef __cplusplus
}
#endif
#endif /* WFLOOKAHEAD_H */
