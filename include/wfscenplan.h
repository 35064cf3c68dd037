/* wfscenplan.h — a scenario planner on the device: the cross-entropy method (CEM) over action sequences, every candidate
 * scored over an ENSEMBLE of M wind futures drawn from the wind process — the scenplan extension of libwfstep.so
 * (include/wfstep.h).
 *
 * The plan extension (include/wfplan.h) searches action sequences under ONE wind path: the current wind held, or rows the
 * caller brings.  The scenario extension (include/wfscenario.h) scores sequences the caller brings over an ensemble of
 * futures.  A receding-horizon controller that knows the wind PROCESS but not its realisation needs both at once: the search
 * of the first, scored by the statistics of the second, under the env's own actuator.  Here ONE glue kernel stands between
 * two evaluator steps and does both jobs — it reduces K M H rows to K scores, refits, and lays the next K M H rows out — and
 * nothing is read back in between.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle:
 * tests/scenplan_ref.py restates it in NumPy over the float64 oracle, composed from tests/plan_ref.py and
 * tests/scenario_ref.py.
 *
 * INPUTS per listed farm b — b is the farm's index in the parent's batch, never its position in a list or a chunk — under the
 * parent's wf_env_config (continuous encoding only) and env state, which are READ ONLY here:
 *   H, K, E, I, sigma [I], seed, gamma, mean0          as wf_plan_run's (include/wfplan.h): K >= 3, E in 1 .. K, sigma a HOST array
 *   M, process, ws_lo, ws_hi, scenario_seed, tail (q in 1 .. M), risk_weight (lam), anchor
 *                                                      as wf_scenario_run's (include/wfscenario.h)
 *   limits   1 <= H <= WF_LOOKAHEAD_MAX_H, 1 <= M <= WF_SCENARIO_MAX_MEMBERS, K M H <= WF_SCENARIO_MAX_ROWS,
 *            1 <= I <= WF_SCENPLAN_MAX_ITERATIONS (16)
 *   WHY I <= 16: the planner's Philox stream is its iteration number i = 0 .. I - 1, and the member paths own streams 16, 17
 *   and 18.  With I <= 16 the two never meet, even when seed and scenario_seed are equal.
 *
 * MEMBER PATHS: exactly wfscenario.h's — the same streams, counters and arithmetic, keyed by scenario_seed, from the farm's
 *   current wind, reverting to the anchor.  They are drawn ONCE per farm and are the same in every iteration: common random
 *   numbers across candidates and across iterations.  Candidate 0 carries the best sequence forward, so it scores the same
 *   bits each time it is evaluated again, and the plan's score never decreases.
 * CANDIDATES of iteration i: exactly wfplan.h's, from the mean mu (mean0, or zeros, before iteration 0): k = 0 the best
 *   sequence so far (the hold in iteration 0); k = 1 mu; k >= 2 element e = h N + t:
 *   (float) clip((double)mu[e] + sigma[i] z, -yaw_step, +yaw_step), z wfplan.h's deviate of philox4x32_10(seed, ctr, stream = i),
 *   ctr = ((uint64)b << 32) | (uint32)(k H N + e).
 * ROWS  R = K M H per farm: row ((k M + m) H + h) holds the yaw AFTER step h of candidate k (wfplan.h's trajectory: it does not
 *   depend on m) and is solved under member m's wind of tick h + 1.  ROW REWARD and normalisers: wfscenario.h's — step 0 is
 *   normalised by the farm's CURRENT speed (a speed wf_env_set_prev_wind left pending is neither used nor consumed), step
 *   h >= 1 by member m's speed of step h - 1.
 * SCORE per candidate: wfscenario.h's member returns (ascending h), mean in ascending m, ranks of the members by counting
 *   (return, m), tail mean over ranks 0 .. q - 1 in ascending rank, score = ((1 - lam) mean) + (lam cvar).
 * UPDATE after iteration i: wfplan.h's with "return" read as "score" — rank_k by (score, k), the elites are rank < E,
 *   mu[e] = (float)((float64 sum over the elites in ASCENDING k) / E), the winner is the largest score, the lowest index among
 *   equals; a winner other than 0 becomes the best sequence so far.
 * OUTPUTS (any may be NULL)
 *   plan                 [n][H][N] float32, the best sequence seen
 *   plan_score, plan_expected, plan_cvar   [n] double, the winner's in the last iteration
 *   plan_member_returns  [n][M] double, the winner's member returns in the last iteration
 *   hold_score           [n] double, candidate 0 of iteration 0
 *   first_action         [n][N] float32, plan's row 0
 *   final_yaw            [n][N] float32, the yaw after walking plan
 *   mean                 [n][H][N] float32, the last mu: shifted by one step it is the next call's mean0
 *   wind_paths           [n][M][H][2] double (speed, direction) of tick h + 1
 * DETERMINISM.  No floating-point atomics and no order that depends on scheduling: two runs, any chunking and any farm list
 * give identical bits from identical step outputs.
 *
 * ACCURACY.  A candidate's score carries the bound wfscenario.h's rule gives it: (1 - lam) times the mean of its member
 * bounds plus lam times the largest member bound.  A farm's plan has the reference's bits when, in every iteration, the
 * last elite and the first non-elite, and the winner and every other candidate of a different trajectory, are further apart
 * than the sum of their score bounds.  A rank flip among the members inside one candidate only moves cvar within that bound:
 * it needs no condition of its own.  strict != 0 solves every row in float64.
 *
 * An object belongs to a parent handle, reads it and stores nothing in it; it must be destroyed BEFORE it.  It owns an
 * EVALUATOR as a plan object does: evaluator farm e = slot R + row, chunks of max_eval_farms / R farms.  Per chunk
 * wf_scenplan_paths_kernel draws the member paths and writes every row's wind and wind_paths, once; then ONE kernel,
 * wf_scenplan_advance_kernel, is launched I + 1 times, one workgroup per slot, with one wf_step of the evaluator between two
 * launches: launch v reduces iteration v - 1 (row rewards, member returns, statistics, ranks, elite mean, winner) and lays
 * out iteration v (draws, trajectories, the M member rows of every step); the last one writes the outputs instead.
 * wf_set_wind_counts is called once per chunk.  The candidates of an iteration are kept between two launches in a grow-only
 * [C][K][H][N] float32 buffer, as wfplan.h's.
 *
 * VERSION-1 LIMITS.  Those of wfplan.h and wfscenario.h: the ON-THE-FLY path, ONE layout, one turbine definition, a parent
 * configured `discrete` is refused.  wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFSCENPLAN_H
#define WFSCENPLAN_H

#include "wfplan.h"
#include "wfscenario.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_SCENPLAN_KERNELS 2
#define WF_SCENPLAN_MIN_K 3
#define WF_SCENPLAN_MAX_ITERATIONS 16

typedef struct wf_scenplan wf_scenplan;

int wf_scenplan_create(wf_handle* h, wf_scenplan** out);
int wf_scenplan_destroy(wf_scenplan* p);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = K M H rows (checked when a run starts);
 *                   <= 0: the default 65 536 */
int wf_scenplan_config(wf_scenplan* p, int strict, int max_eval_farms);

/* Plans for the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   H, K, E, I, sigma, seed, gamma          as wf_plan_run; sigma is always a HOST array of I doubles
 *   M, process, ws_lo, ws_hi, scenario_seed, tail, risk_weight   as wf_scenario_run
 *   anchor      [n_farms][2] double, block i belongs to farms[i], or NULL = every farm's current wind
 *   mean0       [n_farms][H][N] float, block i belongs to farms[i], or NULL = zeros
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   the outputs as above; any may be NULL
 * on_device != 0: anchor, mean0 and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_plan_run).  A device anchor is the caller's to keep valid: only a host anchor is checked.
 * WF_E_INVALID: no wind set, no env state, H, M, K, K M H or I outside the limits, E outside 1 .. K, sigma NULL or an entry
 * negative or not finite, gamma or risk_weight outside [0, 1] or not finite, tail outside 1 .. M, process NULL or a parameter
 * outside its range, bounds that are not finite with 0 < ws_lo < ws_hi, a host anchor whose speed is not > 0 or whose
 * direction is not finite, a farm index out of range, max_eval_farms below K M H.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts or with turbine definitions; a parent configured discrete. */
int wf_scenplan_run(wf_scenplan* p, int H, int K, int E, int I, const double* sigma, unsigned long long seed, double gamma, int M,
                    const wf_wind_process* process, double ws_lo, double ws_hi, unsigned long long scenario_seed, int tail,
                    double risk_weight, const double* anchor, const float* mean0, int n_farms, const int* farms, float* plan,
                    double* plan_score, double* plan_expected, double* plan_cvar, double* plan_member_returns, double* hold_score,
                    float* first_action, float* final_yaw, float* mean, double* wind_paths, int on_device);

/* detail != 0: the following wf_scenplan_run calls record 2 I + 2 HIP events per chunk, so that wf_scenplan_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_scenplan_set_timing(wf_scenplan* p, int detail);

/* HIP-event milliseconds of the last wf_scenplan_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_set_wind_counts + wf_step calls, and the glue kernels' launches (both 0 unless wf_scenplan_set_timing asked
 * for the split).  Pointers may be NULL. */
int wf_scenplan_last_timing(wf_scenplan* p, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/scenplan_timing.py).  Owned by the object. */
wf_handle* wf_scenplan_evaluator(wf_scenplan* p);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_SCENPLAN_KERNELS][3] ints: rows wf_scenplan_paths_kernel, wf_scenplan_advance_kernel
 * (their LDS is dynamic). */
int wf_scenplan_kernel_info(wf_scenplan* p, int* info);

const char* wf_scenplan_last_error(wf_scenplan* p);

#ifdef __cplusplus
}
#endif
#endif /* WFSCENPLAN_H */
