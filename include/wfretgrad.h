/* wfretgrad.h — the gradient of look-ahead returns with respect to the action sequences that produced them, on the device:
 * d ret / d actions[k][h][i] of the H-step discounted return include/wflookahead.h defines — the retgrad extension of
 * libwfstep.so (include/wfstep.h).
 *
 * The control-side extensions form a chain: one-step power sensitivities (include/wfgrad.h), one-step reward counterfactuals
 * (include/wfcredit.h), H-step returns of given sequences (include/wflookahead.h), a zeroth-order planner over them
 * (include/wfplan.h).  This one is the first-order link: what gradient-based MPC, first-order trajectory optimisation, analytic
 * policy gradients through the simulator and a short-horizon actor-critic with a value bootstrap need.  The transition does
 * not depend on the wake solve and each step's reward depends only on the yaw after that step, so the base row of every step
 * plus a +- row per turbine suffice — H (2 N + 1) rows per sequence, all independent rows of ONE batched step — and a backward
 * sweep over the horizon carries the transition's 0/1 Jacobian.  This is THE PROJECT'S OWN definition; PARITY UNPINNED beyond
 * the oracle: tests/retgrad_ref.py restates it in NumPy over the float64 oracle.
 *
 * INPUTS per farm b, under the parent's wf_env_config and env state (yaw y, accumulator acc, move counter moves), which is
 * READ ONLY here (call it before the env step):
 *   actions  [n_farms][K][H][N] float32, CONTINUOUS encoding only, caller's turbine order; 1 <= H <= WF_RETGRAD_MAX_H, K >= 1
 *   wind     [n_farms][H][2] double (speed, direction), the wind step h is solved under; NULL = the parent's current wind of
 *            the farm, held over the horizon — also under a parent in series mode, unless wf_retgrad_set_series asks for the
 *            series' coming rows, which are then read on the device
 *   gamma    double, finite, in [0, 1]
 *   delta    double, finite, > 0: the perturbation in degrees
 *   terminal [n_farms][K][N] double, or NULL = zeros: the derivative of a caller's terminal value with respect to the final
 *            yaw (the critic's gradient in a bootstrapped return)
 *
 * TRAJECTORY of sequence k, exactly include/wflookahead.h's, in the same float32 operations in the same order: start from
 * (y, acc, moves); for h = 0 .. H-1:  frac = acc / rate / (moves + 1 + h) / dt; frac >= budget zeroes the action (the gate);
 * a = the action clipped to +-yaw_step; y = clip(y + a, lo, hi); acc += |a|.  Two PASS FLAGS are recorded per (k, h, i):
 *   t (state passes)   1 iff the clip to [lo, hi] returned y + a unchanged
 *   s (action passes)  1 iff the gate was open and the clip to +-yaw_step returned the action unchanged, AND t = 1
 * The rule is one sentence: the derivative of an operation is 1 where it returned its input unchanged, else 0.  The
 * dependence of LATER gates on acc (and through it on earlier actions) is piecewise constant: its derivative is taken as 0.
 *
 * EVALUATOR ROWS  R = K H (2 N + 1) per farm; for sequence k and step h, rows (k H + h)(2 N + 1) + j, all under wind h:
 *   j = 0        the yaw y_h after step h — the row include/wflookahead.h solves
 *   j = 2 i + 1  y_h with entry i replaced by y+ = (float)min((double)y_h[i] + delta, hi)
 *   j = 2 i + 2  y_h with entry i replaced by y- = (float)max((double)y_h[i] - delta, lo)
 * lo, hi are the env's yaw bounds.  The perturbation is include/wfgrad.h's: float64, rounded once, one-sided at a bound.  The
 * divisor is d = (double)y+ - (double)y-; where d <= 0 the quotient is exactly 0.
 * ROW REWARD, float64, exactly include/wflookahead.h's formula and orders; the +- rows of step h are normalised by the speed
 * step h's base row is normalised by — the free-stream speed BEFORE the step.
 * QUOTIENT  q[h][i] = (r(row 2 i + 1) - r(row 2 i + 2)) / d, float64.
 * BACKWARD SWEEP per (k, i), float64, every product and sum rounded on its own:  g_0 = 1, g_h = g_{h-1} gamma;
 *   lam = terminal (or 0);  for h = H-1 .. 0:  lam = g_h q[h][i] + lam;  action_gradient[h][i] = s[h][i] ? lam : 0;
 *   lam = t[h][i] ? lam : 0;  after h = 0:  state_gradient[i] = lam — the derivative with respect to the yaw the env holds now.
 * OUTPUTS (any may be NULL)
 *   returns, rewards, farm_power, final_yaw, best   the base rows', defined exactly as in include/wflookahead.h ([n_farms][K],
 *                    [n_farms][K][H], [n_farms][K][H], [n_farms][K][N] float32, [n_farms] int); returns excludes any terminal value
 *   action_gradient  [n_farms][K][H][N] double, reward units per degree
 *   reward_gradient  [n_farms][K][H][N] double, the undiscounted q: a closed-loop policy chains through its own transition
 *   state_gradient   [n_farms][K][N] double
 *   yaw              [n_farms][K][H][N] float32, the trajectory
 *   pass_mask        [n_farms][K][H][N] unsigned char: bit 0 = s, bit 1 = t
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs; yaw, final_yaw and pass_mask do not depend on the solver at all.
 *
 * WHAT THE DERIVATIVE IS.  A difference quotient at the finite step delta, as include/wfgrad.h's — the model has kinks —
 * chained through a 0/1 transition Jacobian.  A quotient carries (bound(row+) + bound(row-)) / d of the step's tolerance:
 * strict != 0 solves every row in float64.
 *
 * An object belongs to a parent handle, reads it and stores nothing in it; it must be destroyed BEFORE it.  It owns an
 * EVALUATOR as a lookahead object does: evaluator farm e = slot R + row, chunks of the largest farm count with
 * chunk R <= max_eval_farms.  Per chunk ONE lay-out kernel walks the trajectories and writes the [chunk][R][N] yaw block, the
 * divisors, the pass flags, the trajectory, every row's wind and final_yaw; wf_set_wind_counts and one wf_step on the
 * evaluator write power and load; ONE reduce kernel, a workgroup per (farm, sequence), forms the quotients, the sweep and the
 * return; a third small kernel picks `best` from the K returns of a farm in ascending k (chosen over a last-block pass in the
 * reduce kernel: no counter, no fence).  A whole run is enqueued without a host round trip between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator always runs on the ON-THE-FLY path (a wind per row).  A parent with several layouts or
 * several turbine definitions is refused, and so is one configured for the discrete encoding.  N <= WF_RETGRAD_MAX_N.  No
 * second derivatives, no derivative through the budget gate's threshold.  wfstep.h and WF_ABI_VERSION are not touched by this
 * extension.
 */
#ifndef WFRETGRAD_H
#define WFRETGRAD_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_RETGRAD_KERNELS 3
#define WF_RETGRAD_MAX_H 64
#define WF_RETGRAD_MAX_N 1024
#define WF_RETGRAD_DEFAULT_EVAL_FARMS 65536

typedef struct wf_retgrad wf_retgrad;

int wf_retgrad_create(wf_handle* h, wf_retgrad** out);
int wf_retgrad_destroy(wf_retgrad* r);

/* The evaluator: a new object holds strict 0, WF_RETGRAD_DEFAULT_EVAL_FARMS evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = K H (2 N + 1) rows (checked when a run
 *                   starts, where K and H are known); <= 0: the default */
int wf_retgrad_config(wf_retgrad* r, int strict, int max_eval_farms);

/* ahead != 0: the rows' wind is the window of the series' coming rows (include/wfseries.h, first = 1), enqueued on the device
 * in front of the lay-out into a buffer of the object's own; `wind` must then be NULL, and step 0 is normalised as the coming
 * env step will be: by the current speed.  Default 0. */
int wf_retgrad_set_series(wf_retgrad* r, int ahead);

/* Return gradients of the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   actions     [n_farms][K][H][N] float, block i belongs to farms[i]
 *   wind        [n_farms][H][2] double, or NULL = the parent's current wind held
 *   terminal    [n_farms][K][N] double, or NULL = zeros
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   returns .. pass_mask   as above; any may be NULL
 * on_device != 0: actions, wind, terminal and the outputs are device pointers and the call only enqueues work on the parent's
 * stream — except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a
 * `farms` list is given (as wf_lookahead_run).
 * WF_E_INVALID: no wind set, no env state (wf_env_config and wf_env_reset come first), actions == NULL, H outside
 * 1 .. WF_RETGRAD_MAX_H, K < 1, gamma outside [0, 1] or not finite, delta not finite or <= 0, a farm index out of range,
 * max_eval_farms below K H (2 N + 1); in series-ahead mode a parent not in series mode, a wind of the caller's own, an
 * exhausted series.
 * WF_E_UNSUPPORTED (version 1): a parent configured for the discrete encoding, with several layouts (wf_set_layouts*), with
 * turbine definitions (wf_set_turbine_types) or with more than WF_RETGRAD_MAX_N turbines. */
int wf_retgrad_run(wf_retgrad* r, const float* actions, int K, int H, const double* wind, double gamma, double delta,
                   const double* terminal, int n_farms, const int* farms, double* returns, double* rewards, double* farm_power,
                   float* final_yaw, int* best, double* action_gradient, double* reward_gradient, double* state_gradient,
                   float* yaw, unsigned char* pass_mask, int on_device);

/* detail != 0: the following wf_retgrad_run calls record four HIP events per chunk, so that wf_retgrad_last_timing can split
 * the total into step and glue time.  Default 0: two events per run. */
int wf_retgrad_set_timing(wf_retgrad* r, int detail);

/* HIP-event milliseconds of the last wf_retgrad_run (synchronises), as wf_lookahead_last_timing.  Pointers may be NULL. */
int wf_retgrad_last_timing(wf_retgrad* r, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/retgrad_timing.py).  Owned by the object. */
wf_handle* wf_retgrad_evaluator(wf_retgrad* r);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_RETGRAD_KERNELS][3] ints: rows wf_retgrad_layout_kernel, wf_retgrad_reduce_kernel (its LDS
 * is dynamic), wf_retgrad_best_kernel. */
int wf_retgrad_kernel_info(wf_retgrad* r, int* info);

const char* wf_retgrad_last_error(wf_retgrad* r);

#ifdef __cplusplus
}
#endif
#endif /* WFRETGRAD_H */
