/* wfrollout.h — closed-loop rollouts of yaw-table controllers on the device: the discounted return the env would pay over the
 * next H steps under each of K look-up-table controllers (filter, deadband, preview), from the state the env is in — the
 * rollout extension of libwfstep.so (include/wfstep.h).
 *
 * The yaw look-up table (include/wfrose.h: wf_rose_set_table, wf_rose_policy) is the industry baseline every wake-steering
 * result is held to; wf_rose_policy issues its action for ONE step.  What the table controller earns over an episode under the
 * env's own actuator — at most yaw_step per step, then the budget gate — depends on how the controller filters the wind
 * direction and how wide a deadband it holds inside.  The lookahead extension (include/wflookahead.h) scores OPEN-LOOP action
 * sequences; here the action of step h depends on the yaw state step h - 1 left, so the controller runs in the loop.  The
 * transition does not depend on the wake solve and the controller sees only the wind and the yaw state, so the yaw of every
 * step is known before any farm is solved: the K H solves of a farm are independent rows of ONE batched step, and a whole
 * tuning grid of controllers is one call.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle:
 * tests/rollout_ref.py restates it in NumPy over the float64 oracle.
 *
 * INPUTS per farm b, under the parent's wf_env_config and env state (yaw y, accumulator acc, move counter moves), which is
 * READ ONLY here:
 *   K controllers, 1 <= K <= WF_ROLLOUT_MAX_K, the same for every farm; controller k is
 *     slot[k]      int     a filled table slot of the rose object the rollout object was created on
 *     alpha[k]     double  in (0, 1], the filter's gain
 *     deadband[k]  float   >= 0, degrees
 *     lead[k]      int     0 .. WF_ROLLOUT_MAX_LEAD, the preview in steps
 *   H        the horizon, 1 <= H <= WF_ROLLOUT_MAX_H, K H <= WF_ROLLOUT_MAX_ROWS
 *   wind     [n_farms][H][2] double (speed, direction), the wind step h is solved under; NULL = the parent's current wind of
 *            the farm, held over the horizon — also under a parent in series mode, unless wf_rollout_set_series asks for the
 *            series' coming rows: the window (first = 1, H) of include/wfseries.h, read on the device
 *   filter0  [n_farms][K][2] double (speed, direction), the filter state to start from; NULL = the farm's current wind
 *   gamma    double, finite, in [0, 1]
 *
 * OBSERVATIONS.  obs[0] is the wind the parent holds; obs[j], j = 1 .. H, is the wind of step j - 1: what the env shows
 * (freewind_measurements) before step j.
 *
 * CONTROLLER k, for h = 0 .. H - 1, in this order:
 *   1. observation  o = obs[min(h + lead, H)]: lead 0 is what the env shows before step h, lead 1 the wind step h is solved
 *      under (a perfect one-step preview)
 *   2. filter, float64, every product and sum rounded on its own:
 *        fs = fs + alpha (o_s - fs);   fd = fd + alpha wrap(o_d - fd),   wrap(d) = d - 360 rint(d / 360), ties to even
 *      alpha == 1 copies the observation with no arithmetic.  No transcendental anywhere.
 *   3. target = the look-up of table `slot` at (fs, fd) (include/wfrose.h: its own reduction of the direction, bracket,
 *      LINEAR / NEAREST, one rounding to float32), clipped to the env's (yaw_lo, yaw_hi) as wf_rose_policy clips it
 *   4. the RAW action from e = target - y in float32:
 *        continuous  0 if |e| <= deadband, else e clipped to +-yaw_step
 *        discrete    1 if |e| <= deadband, else 2 if e >= yaw_step / 2, 0 if e <= -yaw_step / 2, else 1
 *      With deadband 0 this is wf_rose_policy's action.
 *   5. transition: the fused env step's, with the move counter moves + 1 + h (include/wflookahead.h: TRAJECTORY), then
 *      acc += |da|
 * EVALUATOR ROWS  R = K H per farm: row k H + h holds the yaw AFTER step h of controller k, under wind h.
 * ROW REWARD, wr, RETURN, best: those of include/wflookahead.h, word for word — r = psum / N / 1e6 * 1e3 / (wr wr wr) -
 *   load_coef lsum / (4 N) in float64 left to right; wr is the free-stream speed BEFORE the step: for h = 0 the parent's
 *   pending speed (wf_env_set_prev_wind or a series tick, read, not consumed), else the farm's current speed — in series-ahead
 *   mode the current speed —, for h >= 1 the speed of wind h - 1; g_0 = 1, g_h = g_{h-1} gamma, ret = sum_h g_h r_h in
 *   ascending h, product and sum rounded separately; best = the controller of the largest return, the lowest index among
 *   equal maxima.
 * OUTPUTS (any may be NULL)
 *   returns      [n_farms][K] double
 *   rewards      [n_farms][K][H] double
 *   farm_power   [n_farms][K][H] double (psum, W)
 *   actions      [n_farms][K][H][N] float32, the RAW actions of step 4: what wf_env_step or wf_lookahead_run would be given
 *   final_yaw    [n_farms][K][N] float32, the yaw after step H - 1
 *   gated        [n_farms][K] int, the number of (step, turbine) pairs at which the budget gate was closed
 *   filter_final [n_farms][K][2] double, the filter state after step H - 1: the next call's filter0
 *   best         [n_farms] int
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs; actions, final_yaw, gated and filter_final do not depend on the solver at all.
 *
 * ACCURACY.  As include/wflookahead.h: a row's reward carries the step's per-turbine tolerance, returns of two controllers
 * closer than the sum of their bounds are not ordered reliably; strict != 0 solves every row in float64.
 *
 * A rollout object is created on a rose object (and through it on that object's parent handle): it reads the rose object's
 * device tables and the parent (layout, model, wind, env parameters and env state, kernel choice, resolve mode) and stores
 * nothing in either; it must be destroyed BEFORE the rose object.  It owns an EVALUATOR as a lookahead object does: evaluator
 * farm e = slot R + row, chunks of the largest farm count with chunk R <= max_eval_farms.  Per chunk ONE lay-out kernel
 * walks the filters (once per controller, not per turbine), then the trajectories, and writes the [chunk][R][N] yaw block,
 * every row's wind, actions, final_yaw, gated and filter_final; wf_set_wind_counts and one wf_step on the evaluator write
 * power and load; ONE reduce kernel — the body of the lookahead extension's — forms the returns.  A whole run is enqueued
 * without a host round trip between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator always runs on the ON-THE-FLY path.  A parent with several layouts or several turbine
 * definitions is refused.  The controllers are the same for every farm.  wfstep.h and WF_ABI_VERSION are not touched by this
 * extension.
 */
#ifndef WFROLLOUT_H
#define WFROLLOUT_H

#include "wfrose.h"
#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_ROLLOUT_KERNELS 2
#define WF_ROLLOUT_MAX_K 64
#define WF_ROLLOUT_MAX_H 1024
#define WF_ROLLOUT_MAX_ROWS 4096
#define WF_ROLLOUT_MAX_LEAD 16

typedef struct wf_rollout wf_rollout;

/* `tables` is a rose object of `h` (wf_rose_create(h, ..)): the controllers' slots are its table slots */
int wf_rollout_create(wf_handle* h, wf_rose* tables, wf_rollout** out);
int wf_rollout_destroy(wf_rollout* r);

/* The evaluator, as wf_lookahead_config: strict != 0 solves every row in float64; max_eval_farms must hold one farm's
 * R = K H rows (checked when a run starts); <= 0: the default 65 536 */
int wf_rollout_config(wf_rollout* r, int strict, int max_eval_farms);

/* ahead != 0: the rows' wind is the window of the series' coming rows (include/wfseries.h, first = 1), enqueued on the device
 * in front of the lay-out into a buffer of the object's own; `wind` must then be NULL.  Default 0. */
int wf_rollout_set_series(wf_rollout* r, int ahead);

/* Rollouts of the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   slot, alpha, deadband, lead   [K] the controllers: always HOST arrays, validated
 *   wind        [n_farms][H][2] double, or NULL = the parent's current wind held
 *   filter0     [n_farms][K][2] double, or NULL = the farm's current wind
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   returns .. best   as above; any may be NULL
 * on_device != 0: wind, filter0 and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt, when the
 * controllers differ from the previous call's and when a `farms` list is given.
 * WF_E_INVALID: no wind set, no env state, a NULL controller array, K outside 1 .. WF_ROLLOUT_MAX_K, H outside
 * 1 .. WF_ROLLOUT_MAX_H, K H > WF_ROLLOUT_MAX_ROWS, a slot out of range, empty or set for another turbine count, alpha
 * outside (0, 1] or not finite, a deadband negative or not finite, a lead outside 0 .. WF_ROLLOUT_MAX_LEAD, gamma outside
 * [0, 1] or not finite, a farm index out of range, max_eval_farms below K H; in series-ahead mode a parent not in series
 * mode, a wind of the caller's own, an exhausted series.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_rollout_run(wf_rollout* r, int K, const int* slot, const double* alpha, const float* deadband, const int* lead, int H,
                   const double* wind, const double* filter0, double gamma, int n_farms, const int* farms, double* returns,
                   double* rewards, double* farm_power, float* actions, float* final_yaw, int* gated, double* filter_final,
                   int* best, int on_device);

/* detail != 0: the following wf_rollout_run calls record four HIP events per chunk, so that wf_rollout_last_timing can split
 * the total into step and glue time.  Default 0: two events per run. */
int wf_rollout_set_timing(wf_rollout* r, int detail);

/* HIP-event milliseconds of the last wf_rollout_run (synchronises), as wf_lookahead_last_timing.  Pointers may be NULL. */
int wf_rollout_last_timing(wf_rollout* r, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/rollout_timing.py).  Owned by the object. */
wf_handle* wf_rollout_evaluator(wf_rollout* r);

/* Register / LDS footprint of the kernels as the runtime reports it: info [WF_ROLLOUT_KERNELS][3] ints (vgprs, static LDS
 * bytes, private-segment bytes): rows wf_rollout_layout_kernel, wf_rollout_reduce_kernel (the latter's LDS is dynamic). */
int wf_rollout_kernel_info(wf_rollout* r, int* info);

const char* wf_rollout_last_error(wf_rollout* r);

#ifdef __cplusplus
}
#endif
#endif /* WFROLLOUT_H */
