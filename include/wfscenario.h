/* wfscenario.h — scenario look-ahead: the returns of K candidate action sequences over an ENSEMBLE of M sampled wind futures,
 * with their mean, their tail mean and a choice, on the device — the scenario extension of libwfstep.so (include/wfstep.h).
 *
 * The look-ahead extension (include/wflookahead.h) scores action sequences under ONE wind per (farm, step): the current wind
 * held (a persistence forecast with no uncertainty) or the rows an episode is going to play (perfect foresight).  A planner
 * that knows the wind PROCESS (include/wfwindgen.h: wf_wind_process) but not its realisation scores every candidate over an
 * ensemble of futures drawn from that process and picks by expected return, or by a risk measure of it.  This extension
 * draws the ensemble on the device, lays the K M H rows of a farm out for ONE batched step and reduces them to per-member
 * returns, mean, tail mean (CVaR), a score and a choice, with no host read in between.  This is THE PROJECT'S OWN
 * definition.  PARITY UNPINNED beyond the oracle: tests/scenario_ref.py restates it in NumPy over the float64 oracle.  All
 * member-path and statistics arithmetic is float64 and every product and sum below is ONE rounding (the library is built with
 * -ffp-contract=off), so the NumPy restatement reproduces the bits of the paths and, from the device's own member returns,
 * of the statistics.
 *
 * INPUTS per listed farm b — b is the farm's index in the parent's batch, never its position in a list or a chunk — under the
 * parent's wf_env_config and env state, which is READ ONLY here:
 *   actions     [n][K][H][N] float32, the env's action encoding, caller's turbine order
 *   M           members of the ensemble
 *   process     a wf_wind_process, with the range checks of wf_windgen_generate
 *   ws_lo, ws_hi  the speed clip bounds, finite, 0 < ws_lo < ws_hi
 *   seed        64 bits
 *   gamma       double, finite, in [0, 1]
 *   tail        q in 1 .. M: the tail mean is over the q lowest member returns
 *   risk_weight lam, finite, in [0, 1]
 *   anchor      [n][2] (speed > 0, finite direction) the paths revert to, or NULL = the farm's current wind, read on the device
 *   limits      1 <= H <= WF_LOOKAHEAD_MAX_H, 1 <= M <= WF_SCENARIO_MAX_MEMBERS, K >= 1, K M H <= WF_SCENARIO_MAX_ROWS
 *
 * MEMBER PATHS.  All K sequences of a farm share its M paths (common random numbers).  (S_c, D_c) is the farm's current
 * wind, (S_a, D_a) the anchor.  The draws are Philox streams 16, 17 and 18 (csrc/wf_philox.h); NO OTHER KERNEL of the library
 * names these streams: 0 .. 2 are the reset draw and the series starts, 3 .. 5 the wind generator.  (The planner's stream is
 * its iteration number, wf_plan_run's i: only a plan of more than 16 iterations reaches 16, with counters of its own layout.)
 *   rate_m = wd_ramp * (2 * u01(r[0], r[1]) - 1),  r = philox(seed, (b << 32) | m, 16)
 *   x_0 = S_c, y_0 = D_c;  for u = 1 .. H, with z(s) = wf_deviate(seed, (b << 32) | (m * 64 + u - 1), s) (csrc/ext/wf_deviate.h):
 *     x_u = (x_{u-1} + ws_revert * (S_a - x_{u-1})) + ws_sigma * z(17)
 *     y_u = (y_{u-1} + wd_revert * ((D_a + rate_m * (double)u) - y_{u-1})) + wd_sigma * z(18)
 *     speed_u     = min(max(x_u, ws_lo), ws_hi)
 *     direction_u = fmod(y_u, 360), + 360 if negative
 *   The latent is neither clipped nor wrapped: the wind generator's rules.  A farm's paths depend on (seed, b, m, process,
 *   anchor, bounds) and its current wind alone: not on K, not on env_batch, not on a farm list or a chunk.
 *   Step h is solved under tick u = h + 1: every step of the horizon lies in the unknown future, as on the episodes where the
 *   tick precedes the step.
 *
 * TRAJECTORY of sequence k: include/wflookahead.h's, the same float32 operations; it does not depend on m.
 * EVALUATOR ROWS  R = K M H per farm: row ((k M + m) H + h) holds the yaw AFTER step h of sequence k and is solved under member
 *   m's wind of step h.
 * ROW REWARD: include/wflookahead.h's formula.  Step 0 is normalised by the farm's CURRENT speed, as in the series-ahead mode:
 *   a speed wf_env_set_prev_wind left pending is neither used nor consumed.  Step h >= 1 is normalised by member m's speed of
 *   step h - 1.
 * MEMBER RETURN  g_0 = 1, g_h = g_{h-1} gamma;  member_return[k][m] = sum_h g_h r_h added in ascending h, product and sum
 *   rounded separately (as wf_lookahead_run's return).
 * STATISTICS per sequence k:
 *   mean  = (sum_m member_return[k][m], added in ascending m) / (double)M
 *   rank of member m = the number of members j with (return_j, j) < (return_m, m) in lexicographic order: a count
 *   cvar  = (sum over ranks 0 .. q - 1 of the member returns, added in ascending rank) / (double)q
 *   score = ((1.0 - lam) * mean) + (lam * cvar)
 *   best  = the sequence of the largest score, the lowest index among equal maxima
 * OUTPUTS (any may be NULL)
 *   expected_returns [n][K] double        cvar [n][K] double        score [n][K] double
 *   member_returns   [n][K][M] double     rewards [n][K][M][H] double
 *   wind_paths       [n][M][H][2] double (speed, direction) of tick h + 1
 *   final_yaw        [n][K][N] float32, the yaw after step H - 1
 *   best             [n] int
 * The env state is read and never changed.  No floating-point atomics and no order that depends on scheduling: two runs, any
 * chunking and any farm list give identical bits from identical step outputs.
 *
 * ACCURACY: as include/wflookahead.h's — a row's reward carries the step's per-turbine tolerance; strict != 0 solves every row
 * in float64.  The tail mean is 1-Lipschitz in the sup norm of the member returns, so cvar is within the largest member bound
 * whatever the ranks do.
 *
 * An object belongs to a parent handle, reads it and stores nothing in it; it must be destroyed BEFORE it.  It owns an
 * EVALUATOR, a further wf_handle on the parent's device and stream: evaluator farm e = slot R + row; chunk is the largest
 * farm count with chunk R <= max_eval_farms, longer farm lists run chunk after chunk.  Per chunk ONE lay-out kernel draws
 * the paths, writes wind_paths, every row's wind, the [chunk][R][N] yaw block and final_yaw; wf_set_wind_counts and one
 * wf_step on the evaluator write power and load; ONE reduce kernel forms the outputs.  A whole run is enqueued without a host
 * round trip between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator always runs on the ON-THE-FLY path (a wind per row).  A parent with several layouts or
 * several turbine definitions is refused.  No per-turbine power of the rows, no caller-made paths (that is wf_lookahead_run
 * with a wind per call).  wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFSCENARIO_H
#define WFSCENARIO_H

#include "wfstep.h"
#include "wfwindgen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_SCENARIO_KERNELS 2
#define WF_SCENARIO_MAX_MEMBERS 64
#define WF_SCENARIO_MAX_ROWS 4096

typedef struct wf_scenario wf_scenario;

int wf_scenario_create(wf_handle* h, wf_scenario** out);
int wf_scenario_destroy(wf_scenario* s);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = K M H rows (checked when a run starts);
 *                   <= 0: the default 65 536 */
int wf_scenario_config(wf_scenario* s, int strict, int max_eval_farms);

/* Scenario returns of the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   actions     [n_farms][K][H][N] float, block i belongs to farms[i]
 *   anchor      [n_farms][2] double, block i belongs to farms[i], or NULL
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   the outputs as above; any may be NULL
 * on_device != 0: actions, anchor and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_lookahead_run).  A device anchor is the caller's to keep valid: only a host anchor is checked.
 * WF_E_INVALID: no wind set, no env state, actions or process NULL, H, M, K or K M H outside the limits, tail outside 1 .. M,
 * risk_weight or gamma outside [0, 1] or not finite, a process parameter outside its range, bounds that are not finite with
 * 0 < ws_lo < ws_hi, a host anchor whose speed is not > 0 or whose direction is not finite, a farm index out of range,
 * max_eval_farms below K M H.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts or with turbine definitions. */
int wf_scenario_run(wf_scenario* s, const float* actions, int K, int H, int M, const wf_wind_process* process, double ws_lo,
                    double ws_hi, unsigned long long seed, double gamma, int tail, double risk_weight, const double* anchor,
                    int n_farms, const int* farms, double* expected_returns, double* cvar, double* score, double* member_returns,
                    double* rewards, double* wind_paths, float* final_yaw, int* best, int on_device);

/* detail != 0: the following wf_scenario_run calls record four HIP events per chunk, so that wf_scenario_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_scenario_set_timing(wf_scenario* s, int detail);

/* HIP-event milliseconds of the last wf_scenario_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels (both 0 unless wf_scenario_set_timing asked for the
 * split).  Pointers may be NULL. */
int wf_scenario_last_timing(wf_scenario* s, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/scenario_timing.py).  Owned by the object. */
wf_handle* wf_scenario_evaluator(wf_scenario* s);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_SCENARIO_KERNELS][3] ints: rows wf_scenario_layout_kernel, wf_scenario_reduce_kernel
 * (their LDS is dynamic). */
int wf_scenario_kernel_info(wf_scenario* s, int* info);

const char* wf_scenario_last_error(wf_scenario* s);

#ifdef __cplusplus
}
#endif
#endif /* WFSCENARIO_H */
