/* wfrollscen.h — scenario rollouts: K yaw-table controllers (filter, deadband, preview) run in closed loop under each of M wind
 * futures drawn from a wind process, scored by the mean and the tail mean of their returns, with a choice, on the device — the
 * scenario-rollout extension of libwfstep.so (include/wfstep.h).
 *
 * The extensions cover action sequences under one wind path (include/wflookahead.h) and over an ensemble (include/wfscenario.h),
 * and controllers under one wind path (include/wfrollout.h).  This is the fourth cell: controllers over an ensemble.  An
 * open-loop sequence is the same under every future; a look-up-table controller is a FEEDBACK policy — it filters each
 * future's wind, looks the table up and moves the yaw differently under every member —, so only an ensemble says what its
 * gain, deadband and preview are worth under a wind PROCESS rather than on one realisation, and per farm from the farm's own
 * state: controller selection in a receding horizon.  The controller sees only the free wind and the yaw state, so every yaw
 * of every (controller, member, step) is known before any farm is solved: the K M H solves of a farm are independent rows of
 * ONE batched step.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle.  It is composed word for word
 * from include/wfrollout.h (the controller) and include/wfscenario.h (paths, rows, rewards, statistics), and
 * tests/rollscen_ref.py composes their NumPy restatements over the float64 oracle.
 *
 * INPUTS per listed farm b — b is the farm's index in the parent's batch, never its position in a list or a chunk — under the
 * parent's wf_env_config and env state, which is READ ONLY here:
 *   K controllers (slot, alpha, deadband, lead): include/wfrollout.h's, on the table slots of the rose object the object was
 *     created on, 1 <= K <= WF_ROLLSCEN_MAX_K, lead <= WF_ROLLOUT_MAX_LEAD, the same for every farm
 *   H, M, process, ws_lo, ws_hi, seed, gamma, tail, risk_weight, anchor: include/wfscenario.h's
 *   filter0  [n][K][2] double (speed, direction), the filter states to start from, the same under every member; NULL = the
 *            farm's current wind
 *   limits   1 <= H <= WF_LOOKAHEAD_MAX_H, 1 <= M <= WF_SCENARIO_MAX_MEMBERS, K M H <= WF_ROLLSCEN_MAX_ROWS
 * Both action encodings are served, as by wf_rollout_run.
 *
 * MEMBER PATHS: include/wfscenario.h's, bit for bit — Philox streams 16 to 18 keyed by (seed, b, m, u), paths that start at the
 *   farm's current wind, stored speeds clipped and stored directions wrapped, the latent neither.  A farm's paths depend on
 *   (seed, b, m, process, anchor, bounds) and its current wind alone: wf_scenario_run with the same arguments returns the same
 *   wind_paths.
 * OBSERVATIONS of member m: obs[0] is the wind the parent holds; obs[j], j = 1 .. H, is member m's tick j: the wind of step
 *   j - 1.
 * CONTROLLER k under member m, for h = 0 .. H - 1: include/wfrollout.h's steps 1 to 5 on these observations — the observation
 *   obs[min(h + lead, H)], the float64 filter (every product and sum rounded on its own, alpha == 1 copies), the table look-up
 *   clipped to the env's bounds, the RAW action from the deadband, the fused step's transition with the move counter
 *   moves + 1 + h.  With lead 0 step 0 sees obs[0] only: its action is the same under every member.  With lead >= 1 the
 *   controller previews ITS OWN MEMBER's future: a perfect forecast inside each scenario — what a preview is worth at best,
 *   not what a forecast of the process is worth.
 * EVALUATOR ROWS  R = K M H per farm: row ((k M + m) H + h) holds the yaw AFTER step h of controller k under member m and is
 *   solved under member m's tick h + 1: include/wfscenario.h's row order, and with it its ROW REWARD (step 0 normalised by the
 *   farm's CURRENT speed — a pending prev-wind speed is neither used nor consumed —, step h >= 1 by member m's speed of step
 *   h - 1), MEMBER RETURN (ascending h) and STATISTICS (mean in ascending m, ranks as counts by (return, m), cvar over the tail
 *   lowest in ascending rank, score = ((1 - lam) mean) + (lam cvar), best the lowest index among equal maxima), word for word.
 * OUTPUTS (any may be NULL)
 *   expected_returns [n][K] double        cvar [n][K] double        score [n][K] double
 *   member_returns   [n][K][M] double     rewards [n][K][M][H] double
 *   wind_paths       [n][M][H][2] double (speed, direction) of tick h + 1
 *   actions          [n][K][M][H][N] float32, the RAW actions, as wf_rollout_run reports them
 *   final_yaw        [n][K][M][N] float32, the yaw after step H - 1
 *   gated            [n][K][M] int, the (step, turbine) pairs at which the budget gate was closed
 *   first_action     [n][K][N] float32, member 0's action of step 0: equal across the members iff lead == 0
 *   best             [n] int
 * No floating-point atomics and no order that depends on scheduling: two runs, any chunking and any farm list give identical
 * bits from identical step outputs; actions, final_yaw, gated, first_action and wind_paths do not depend on the solver at all.
 *
 * ACCURACY: include/wfscenario.h's — a row's reward carries the step's per-turbine tolerance, the tail mean is within the
 * largest member bound; strict != 0 solves every row in float64.
 *
 * An object is created on a rose object (and through it on that object's parent handle), as a rollout object is: it reads the
 * rose object's device tables and the parent and stores nothing in either; it must be destroyed BEFORE the rose object.  It
 * owns an EVALUATOR: evaluator farm e = slot R + row, chunks of the largest farm count with chunk R <= max_eval_farms.  Per
 * chunk ONE lay-out kernel draws the paths, walks every (controller, member)'s filter and table brackets once — not per
 * turbine —, then the trajectories, and writes the [chunk][R][N] yaw block, every row's wind, wind_paths, actions, final_yaw,
 * gated and first_action; wf_set_wind_counts and one wf_step on the evaluator write power and load; ONE reduce kernel — the
 * body of the scenario extension's — forms the outputs.  A whole run is enqueued without a host round trip between its
 * launches.  The brackets of a slot stay in LDS up to WF_ROLLSCEN_LDS_RECORDS rows and go through a scratch block in global
 * memory above: two instances of the lay-out kernel, picked at launch.
 *
 * VERSION-1 LIMITS.  The evaluator always runs on the ON-THE-FLY path.  A parent with several layouts or several turbine
 * definitions is refused.  The controllers are the same for every farm.  No per-turbine power of the rows, no farm power, no
 * caller-made paths (that is wf_rollout_run with a wind per call).  wfstep.h and WF_ABI_VERSION are not touched by this
 * extension.
 */
#ifndef WFROLLSCEN_H
#define WFROLLSCEN_H

#include "wflookahead.h"
#include "wfrollout.h"
#include "wfrose.h"
#include "wfscenario.h"
#include "wfstep.h"
#include "wfwindgen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_ROLLSCEN_KERNELS 3
#define WF_ROLLSCEN_MAX_K 64
#define WF_ROLLSCEN_MAX_ROWS 4096
#define WF_ROLLSCEN_LDS_RECORDS 1024

typedef struct wf_rollscen wf_rollscen;

/* `tables` is a rose object of `h` (wf_rose_create(h, ..)): the controllers' slots are its table slots */
int wf_rollscen_create(wf_handle* h, wf_rose* tables, wf_rollscen** out);
int wf_rollscen_destroy(wf_rollscen* r);

/* The evaluator, as wf_scenario_config: strict != 0 solves every row in float64; max_eval_farms must hold one farm's
 * R = K M H rows (checked when a run starts); <= 0: the default 65 536 */
int wf_rollscen_config(wf_rollscen* r, int strict, int max_eval_farms);

/* Scenario rollouts of the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   slot, alpha, deadband, lead   [K] the controllers: always HOST arrays, validated
 *   anchor      [n_farms][2] double, block i belongs to farms[i], or NULL = the farm's current wind
 *   filter0     [n_farms][K][2] double, or NULL = the farm's current wind
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   the outputs as above; any may be NULL
 * on_device != 0: anchor, filter0 and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt, when the controllers
 * differ from the previous call's and when a `farms` list is given.  A device anchor is the caller's to keep valid: only a
 * host anchor is checked.
 * WF_E_INVALID: no wind set, no env state, a NULL controller array, process NULL, K outside 1 .. WF_ROLLSCEN_MAX_K, H outside
 * 1 .. WF_LOOKAHEAD_MAX_H, M outside 1 .. WF_SCENARIO_MAX_MEMBERS, K M H > WF_ROLLSCEN_MAX_ROWS, a slot out of range, empty or
 * set for another turbine count, alpha outside (0, 1] or not finite, a deadband negative or not finite, a lead outside
 * 0 .. WF_ROLLOUT_MAX_LEAD, tail outside 1 .. M, risk_weight or gamma outside [0, 1] or not finite, a process parameter outside
 * its range, bounds that are not finite with 0 < ws_lo < ws_hi, a host anchor whose speed is not > 0 or whose direction is not
 * finite, a farm index out of range, max_eval_farms below K M H.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types). */
int wf_rollscen_run(wf_rollscen* r, int K, const int* slot, const double* alpha, const float* deadband, const int* lead, int H,
                    int M, const wf_wind_process* process, double ws_lo, double ws_hi, unsigned long long seed, double gamma,
                    int tail, double risk_weight, const double* anchor, const double* filter0, int n_farms, const int* farms,
                    double* expected_returns, double* cvar, double* score, double* member_returns, double* rewards,
                    double* wind_paths, float* actions, float* final_yaw, int* gated, float* first_action, int* best,
                    int on_device);

/* detail != 0: the following wf_rollscen_run calls record four HIP events per chunk, so that wf_rollscen_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_rollscen_set_timing(wf_rollscen* r, int detail);

/* HIP-event milliseconds of the last wf_rollscen_run (synchronises), as wf_scenario_last_timing.  Pointers may be NULL. */
int wf_rollscen_last_timing(wf_rollscen* r, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/rollscen_timing.py).  Owned by the object. */
wf_handle* wf_rollscen_evaluator(wf_rollscen* r);

/* Register / LDS footprint of the kernels as the runtime reports it: info [WF_ROLLSCEN_KERNELS][3] ints (vgprs, static LDS
 * bytes, private-segment bytes): rows wf_rollscen_layout_kernel with its brackets in LDS, the same with its brackets in
 * global memory, wf_rollscen_reduce_kernel (their LDS is dynamic).  The lay-out keeps a thread per (controller, member,
 * turbine): no private segment at any N. */
int wf_rollscen_kernel_info(wf_rollscen* r, int* info);

const char* wf_rollscen_last_error(wf_rollscen* r);

#ifdef __cplusplus
}
#endif
#endif /* WFROLLSCEN_H */
