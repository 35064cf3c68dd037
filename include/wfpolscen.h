/* wfpolscen.h — policy rollouts over a wind ensemble: what each of K parameter vectors of one small MLP policy earns in closed
 * loop under each of M wind futures drawn from the wind process, with the mean, the tail mean and a choice per farm, on the
 * device — the policy-scenario extension of libwfstep.so (include/wfstep.h).
 *
 * The project scores control laws along two axes: what acts (action sequences, yaw-table controllers, MLP policies) and the
 * wind it acts under (one path, or an ensemble drawn from the process).  This extension is the cell {MLP policies, ensemble}.
 * A network is a feedback law — it observes the local wind, which comes out of the wake solve —, so it moves the yaw
 * differently under every future and its K M closed loops per farm are K M rows of ONE batched step per env step.  It serves
 * checkpoint selection and the fitness of ES / CEM / PBT under a process, and the policy's "expected" and "worst quarter"
 * columns beside wf_rollscen_run's and wf_scenplan_run's.  This is THE PROJECT'S OWN definition, COMPOSED of two existing ones
 * and restating neither's arithmetic.  PARITY UNPINNED beyond the oracle: tests/polscen_ref.py composes tests/scenario_ref.py
 * (paths, statistics) and tests/policy_ref.py (the closed loop).
 *
 * NETWORK, OBSERVATION, ACTION, TRANSITION: include/wfpolicy.h's (POLICY CLASS, PARAMETERS, ARITHMETIC, CLOSED LOOP).
 *   wf_polscen_set_network takes wf_policy_set_network's arguments.  params [K][P] float32: the same K policies for every
 *   farm and every member.
 * MEMBER PATHS: include/wfscenario.h's (MEMBER PATHS), bit for bit — Philox streams 16 to 18 keyed by (seed, b, m, u), rate_m,
 *   the latent recursion towards the anchor (default: the farm's current wind), the stored speed clipped to (ws_lo, ws_hi), the
 *   stored direction wrapped.  wf_scenario_run with the same (seed, M, H, process, bounds, anchor) returns the same
 *   wind_paths.  The deviate's counter is m * 64 + u - 1: H <= WF_LOOKAHEAD_MAX_H = 64 is part of the keying.
 * CLOSED LOOP of policy k under member m on farm b, from the env state (y, acc, moves) of the farm, which is READ ONLY:
 *   round 0 solves the current yaw under the current wind: observation 0, the same for every (k, m) of the farm;
 *   step h takes the action from observation h, applies the fused step's transition with move counter moves + 1 + h and
 *   solves the new yaw under member m's tick h + 1; observation h + 1 is that yaw, that solve's local wind and that tick as
 *   the free wind.  It is wf_policy_run's loop with wind = wind_paths[b][m].
 * ROW REWARD: wf_lookahead_run's formula with include/wfscenario.h's convention: step 0 is normalised by the farm's CURRENT
 *   speed — a speed wf_env_set_prev_wind left pending is neither used nor consumed —, step h >= 1 by member m's speed of
 *   step h - 1.
 * MEMBER RETURN, MEAN, RANKS BY COUNT, TAIL MEAN, score = ((1 - lam) mean) + (lam cvar), best (the lowest index among equal
 *   maxima): include/wfscenario.h's (MEMBER RETURN, STATISTICS), in its summation orders.
 * With no speed pending, member m's outputs have the bits of wf_policy_run(wind = wind_paths[:, m]) on the same handle in the
 * same mode, and M = 1 under a still process (every sigma, revert and the ramp 0) those of wf_policy_run(wind = NULL) — from
 * identical step outputs: always with strict != 0; in the parent's float32 mode where the two evaluators, of K M and of K rows
 * per farm, are served by the same step kernel, which the library picks by batch size (at 16 384 against 2 048 rows of 80
 * turbines the two ways' member returns did not have the same bits, and named the same best policy on every farm:
 * profiles/polscen_timing.json).
 *
 * LIMITS  1 <= K <= WF_POLSCEN_MAX_K, 1 <= M <= WF_POLSCEN_MAX_MEMBERS, 1 <= H <= WF_POLSCEN_MAX_H; max_eval_farms >= K M.
 *   What wf_policy_run refuses is refused here: several layouts, several turbine definitions, wake-model parameter sets.
 * OUTPUTS (any may be NULL)
 *   expected_returns, cvar, score [n][K] double         member_returns [n][K][M] double
 *   rewards, farm_power [n][K][M][H] double (farm_power in W)
 *   wind_paths   [n][M][H][2] double (speed, direction) of tick h + 1
 *   actions      [n][K][M][H][N] float32, RAW: what wf_env_step takes
 *   observations [n][K][M][H][3 N + 2] float32, un-normalised, the CENTRAL lay-out for both kinds
 *   final_yaw    [n][K][M][N] float32        gated [n][K][M] int, (step, turbine) pairs with a closed budget gate
 *   first_action [n][K][N] float32: step 0's action; it does not depend on m, because observation 0 does not
 *   best         [n] int
 * No floating-point atomics and no order that depends on scheduling: two runs, any chunking, any farm list and host or device
 * arrays give identical bits from identical step outputs.
 *
 * An object belongs to a parent handle, reads it and stores nothing in it; it must be destroyed BEFORE it.  It owns an
 * EVALUATOR: a further wf_handle on the parent's device and stream, K M rows per farm: evaluator farm e = (k M + m) C + slot
 * in a chunk of C farm slots (chunk = the largest farm count with chunk K M <= max_eval_farms), so that a policy's M C rows are
 * contiguous.  Per chunk: ONE paths kernel draws the C M paths into a device buffer and writes wind_paths; the policy
 * extension's begin kernel writes the round-0 rows; then H + 1 steps of the evaluator (power, load, local wind) with the policy
 * extension's advance kernel between two of them — the SAME kernel wf_policy_run launches, told the member count and the path
 * buffer — and wf_set_wind_counts on the evaluator after it; ONE returns kernel forms the last reward and the member returns,
 * ONE statistics kernel the per-policy statistics and the choice.  A whole run is enqueued without a host round trip between
 * its launches.
 *
 * VERSION-1 LIMITS.  The evaluator always runs on the ON-THE-FLY path (a wind per row).  No caller-made paths: that is
 * wf_policy_run with a wind per call.  wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFPOLSCEN_H
#define WFPOLSCEN_H

#include "wfpolicy.h"
#include "wfstep.h"
#include "wfwindgen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_POLSCEN_KERNELS 6
#define WF_POLSCEN_MAX_K 64
#define WF_POLSCEN_MAX_MEMBERS 64
#define WF_POLSCEN_MAX_H 64

typedef struct wf_polscen wf_polscen;

int wf_polscen_create(wf_handle* h, wf_polscen** out);
int wf_polscen_destroy(wf_polscen* p);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's K M rows (checked when a run starts);
 *                   <= 0: the default 65 536 */
int wf_polscen_config(wf_polscen* p, int strict, int max_eval_farms);

/* The network the following runs evaluate (copied; a new object holds none): wf_policy_set_network's arguments, checks and
 * refusals (include/wfpolicy.h). */
int wf_polscen_set_network(wf_polscen* p, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind,
                           double out_scale, const double* shift, const double* scale);

/* The K policies over M members on the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   params      [K][P] float, P the network's parameter count
 *   process, ws_lo, ws_hi, seed, tail, risk_weight, anchor ([n_farms][2] or NULL)   as wf_scenario_run takes them
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   the outputs as above; any may be NULL
 * on_device != 0: params, anchor and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_lookahead_run).  A device anchor is the caller's to keep valid: only a host anchor is checked.
 * WF_E_INVALID: no wind set, no env state, no network set, params or process NULL, a parameter vector of the wrong length (P),
 * K, M or H outside the limits, tail outside 1 .. M, risk_weight or gamma outside [0, 1] or not finite, a process parameter
 * outside its range, bounds that are not finite with 0 < ws_lo < ws_hi, a host anchor whose speed is not > 0 or whose
 * direction is not finite, a network that does not fit the parent (wf_policy_run's checks), a farm index out of range,
 * max_eval_farms below K M.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts, with turbine definitions or with wake-model parameter sets. */
int wf_polscen_run(wf_polscen* p, const float* params, int K, int P, int H, int M, const wf_wind_process* process, double ws_lo,
                   double ws_hi, unsigned long long seed, double gamma, int tail, double risk_weight, const double* anchor,
                   int n_farms, const int* farms, double* expected_returns, double* cvar, double* score, double* member_returns,
                   double* rewards, double* farm_power, double* wind_paths, float* actions, float* observations, float* final_yaw,
                   int* gated, float* first_action, int* best, int on_device);

/* detail != 0: the following wf_polscen_run calls record 2 (H + 1) + 2 HIP events per chunk, so that wf_polscen_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_polscen_set_timing(wf_polscen* p, int detail);

/* HIP-event milliseconds of the last wf_polscen_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_step calls, and the glue — the kernels between them and the evaluator's wf_set_wind_counts after every
 * advance (both 0 unless wf_polscen_set_timing asked for the split).  Pointers may be NULL. */
int wf_polscen_last_timing(wf_polscen* p, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/polscen_timing.py).  Owned by the object. */
wf_handle* wf_polscen_evaluator(wf_polscen* p);

/* Register / LDS footprint of the kernels a run launches, as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS
 * bytes, private-segment bytes.  info [WF_POLSCEN_KERNELS][3] ints: rows wf_polscen_paths_kernel, wf_polscen_returns_kernel,
 * wf_polscen_stats_kernel (the LDS of the last two is dynamic), then the policy extension's wf_policy_transpose_kernel,
 * wf_policy_begin_kernel and wf_policy_advance_kernel. */
int wf_polscen_kernel_info(wf_polscen* p, int* info);

const char* wf_polscen_last_error(wf_polscen* p);

#ifdef __cplusplus
}
#endif
#endif /* WFPOLSCEN_H */
