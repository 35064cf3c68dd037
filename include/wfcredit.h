/* wfcredit.h — per-agent counterfactual rewards on the device: what the farm's reward would have been had ONE turbine done
 * something else — the credit extension of libwfstep.so (include/wfstep.h).
 *
 * The decentralised envs pay every turbine-agent the same cooperative reward; with 80 agents on one scalar, credit
 * assignment is the hard part.  The gradient extension (include/wfgrad.h) gives the local derivative of the POWER.  This one
 * gives the finite counterfactual of the REWARD, load term included: DIFFERENCE REWARDS D_i = r(a) - r(a_-i, c_i) and the
 * rows r(a_-i, a'_i) of a COMA baseline, 1 + N K farm solves per farm in one batched step.  This is THE PROJECT'S OWN
 * definition.  PARITY UNPINNED beyond the oracle: tests/credit_ref.py restates it in NumPy over the float64 oracle.
 *
 * INPUTS per farm, under the wind the parent handle holds: a BASE row [N] and K ALTERNATIVES per turbine [N][K],
 * 1 <= K <= WF_CREDIT_MAX_ALT, float32, caller's turbine order.  Each of the two is declared as
 *   WF_CREDIT_YAW     absolute yaw in degrees, used as given, or
 *   WF_CREDIT_ACTION  an action in the env's encoding under the parent's wf_env_config, turned into a yaw by the
 *                     TRANSITION below.
 * base == NULL: the fused env's current yaw state (base_kind plays no part).  alt == NULL with K == 1: the hold action
 * (0 continuous, 1 discrete) for WF_CREDIT_ACTION, zero yaw for WF_CREDIT_YAW.
 *
 * TRANSITION of turbine t of farm b, the one of the fused env step in the same float32 operations in the same order, on the
 * parent's env state (yaw y, accumulator acc, move counter moves), which is READ ONLY here:
 *   frac = acc / rate / (moves + 1) / dt, every division correctly rounded; frac >= budget zeroes the RAW action (in the
 *   discrete encoding that means "down": the reference's quirk is kept); discrete: a = (a - 1) step, continuous: a clipped to
 *   +-step; y' = clip(y + a, lo, hi).
 * WF_CREDIT_ACTION (and base == NULL) without env state is WF_E_INVALID.
 *
 * EVALUATOR ROWS  R = 1 + N K per farm: row 0 the base yaw, row 1 + i K + k the base with turbine i's entry replaced by
 *   alternative (i, k); every row under the farm's own wind (ws, wd).
 * ROW REWARD, float64:  psum = the row's N float32 powers added in caller order; lsum = the absolute values of its 4 N
 *   float32 load values added in memory order;
 *     r = psum / N / 1e6 * 1e3 / (wr wr wr) - load_coef lsum / (4 N)
 *   evaluated left to right as the float64 re-solve evaluates the env's reward.  wr is the speed the parent's next
 *   wf_env_step would normalise by: what wf_env_set_prev_wind (or a series tick) left for it, else the farm's current speed;
 *   the credit run does NOT consume it.  load_coef is the parent's (wf_env_config; 0.1 on a handle never configured).
 * OUTPUTS  reward [R] double; farm_power [R] double (psum, W); difference [N][K] double = reward[0] - reward[1 + i K + k].
 *   Where an alternative's float32 yaw has the SAME BITS as the base entry, difference is exactly 0.0 and that row's reward
 *   and farm_power are copies of row 0's: the row is still solved, but its bits are not trusted to match row 0's (another
 *   batch position may mean another kernel family, or a float64 re-solve of one of the two rows only).
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs.
 *
 * WHEN TO USE strict.  A difference is the difference of two rewards that each carry the step's per-turbine tolerance, so
 * the contract's worst-case bound on D is 2 x 1e-4 of the reward in the default mode — on a large farm as large as a typical
 * |D| itself (HornsRev1, 4 farms, K = 2: median bound 5.4e-4, median |D| 8.8e-4; against "hold" after a few steps the median
 * |D| is 1.2e-4).  The two rows' float32 errors are strongly correlated and the MEASURED error is far smaller — on those
 * farms max |D_dev - D_ref| = 6.1e-7 in the default mode (0.001 of the bound, 7e-4 of the median |D|) and 2.5e-8 strict
 * (0.009 of its bound of 2.7e-6; profiles/credit_timing.json) — but that is a measurement, not a bound, and a row that
 * alone is re-solved in float64 (a risk flag raised by one of the two yaws) loses the correlation.  Use strict != 0 (every
 * row in float64, about six times the time on HornsRev1) wherever a GUARANTEED error below |D| is needed: validation,
 * farms of tens of turbines whose |D| is below 1e-3, comparisons of near-equal differences across agents.  The default
 * mode serves training loops, small farms and coarse alternatives.
 *
 * An object belongs to a parent handle, reads it (layout, model, wind, env parameters and env state, kernel choice, resolve
 * mode) and stores nothing in it; it must be destroyed BEFORE it.  Like the gradient extension it owns an EVALUATOR: a further
 * wf_handle on the parent's device and stream.  Evaluator farm e = slot R + row; chunk is the largest farm count with
 * chunk R <= max_eval_farms and longer farm lists run chunk after chunk.  Per chunk ONE lay-out kernel writes the
 * [chunk][R][N] yaw block and every row's wind (read from the parent's DEVICE wind); wf_set_wind_counts and one wf_step on the
 * evaluator write power and load; ONE reduce kernel forms the outputs.  A whole run is enqueued without a host round trip
 * between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator is given device arrays, a wind per row, so it always runs on the ON-THE-FLY path, even
 * under a parent with one shared wind; grouping rows onto the pair-table path is not done.  No per-turbine power of the
 * alternative rows.  A parent with several layouts or several turbine definitions is refused.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFCREDIT_H
#define WFCREDIT_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_CREDIT_KERNELS 2
#define WF_CREDIT_MAX_ALT 8
#define WF_CREDIT_YAW 0
#define WF_CREDIT_ACTION 1

typedef struct wf_credit wf_credit;

int wf_credit_create(wf_handle* h, wf_credit** out);
int wf_credit_destroy(wf_credit* c);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = 1 + N K rows (checked when a run
 *                   starts, where K is known; here only against N + 1); <= 0: the default 65 536 */
int wf_credit_config(wf_credit* c, int strict, int max_eval_farms);

/* Counterfactual rewards of the listed farms, under the wind and the env state the parent holds at the time of the call.
 *   base_kind, alt_kind   WF_CREDIT_YAW or WF_CREDIT_ACTION
 *   base        [n_farms][N] float, row i belongs to farms[i], or NULL = the env's current yaw state
 *   alt         [n_farms][N][K] float, or NULL (K == 1 only) = hold / zero yaw
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   reward      [n_farms][R] double
 *   farm_power  [n_farms][R] double   [W]
 *   difference  [n_farms][N][K] double
 * Any output pointer may be NULL.
 * on_device != 0: base, alt and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_grad_run).
 * WF_E_INVALID: no wind set, K outside 1 .. WF_CREDIT_MAX_ALT, a kind that is neither, alt == NULL with K != 1, an action
 * or base == NULL without env state, a farm index out of range, max_eval_farms below R.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_credit_run(wf_credit* c, int base_kind, const float* base, int alt_kind, const float* alt, int K, int n_farms,
                  const int* farms, double* reward, double* farm_power, double* difference, int on_device);

/* detail != 0: the following wf_credit_run calls record four HIP events per chunk, so that wf_credit_last_timing can split
 * the total into step and glue time.  Default 0: two events per run. */
int wf_credit_set_timing(wf_credit* c, int detail);

/* HIP-event milliseconds of the last wf_credit_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels (both 0 unless wf_credit_set_timing asked for the
 * split).  Pointers may be NULL. */
int wf_credit_last_timing(wf_credit* c, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/credit_timing.py).  Owned by the object. */
wf_handle* wf_credit_evaluator(wf_credit* c);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_CREDIT_KERNELS][3] ints: rows wf_credit_layout_kernel, wf_credit_reduce_kernel (their
 * LDS is dynamic on top). */
int wf_credit_kernel_info(wf_credit* c, int* info);

const char* wf_credit_last_error(wf_credit* c);

#ifdef __cplusplus
}
#endif
#endif /* WFCREDIT_H */
