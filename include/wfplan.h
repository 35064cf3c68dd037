/* wfplan.h — a receding-horizon planner on the device: the cross-entropy method (CEM) over action sequences, scored by the
 * discounted return the env would pay over the next H steps — the plan extension of libwfstep.so (include/wfstep.h).
 *
 * The lookahead extension (include/wflookahead.h) scores K given action sequences in one batched step.  A planner repeats
 * draw, score and refit several times per env step; written over that call it pays a host round trip and a handful of small
 * kernels between any two evaluator steps.  Here ONE glue kernel stands between two steps and no host read: the pattern of
 * the yaw search (include/wfyawopt.h), for the sequential problem.  What it gives is the model-predictive baseline under the
 * env's OWN transition — the yaw moves at most yaw_step per step and the actuation budget then silences a turbine —, run
 * beside the batched env at the env's rate.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle:
 * tests/plan_ref.py restates it in NumPy over the float64 oracle.
 *
 * INPUTS per farm b, under the parent's wf_env_config (continuous encoding only) and env state, which is READ ONLY here:
 *   H       horizon, 1 <= H <= WF_LOOKAHEAD_MAX_H
 *   K       candidates per iteration, K >= 3, K H <= WF_LOOKAHEAD_MAX_ROWS
 *   E       elites, 1 <= E <= K
 *   I       iterations, I >= 1, with sigma [I] (a HOST array): finite non-negative doubles, degrees — the caller supplies the
 *           refining widths, as the yaw search's passes do.  There is no fitted standard deviation: the kernel takes no square
 *           root and every candidate has bits NumPy can reproduce
 *   seed    64 bits
 *   gamma   double, finite, in [0, 1]
 *   wind    [n_farms][H][2] double (speed, direction), or NULL = the parent's current wind held: as in wf_lookahead_run
 *   mean0   [n_farms][H][N] float32, or NULL = zeros: the warm start of a receding horizon
 *
 * CANDIDATES of iteration i, raw actions [K][H][N] float32, mu the current mean (mean0 before iteration 0):
 *   k = 0   the best sequence so far; in iteration 0 all zeros, the hold: the plan is never worse than doing nothing
 *   k = 1   mu, unperturbed
 *   k >= 2  element e = h N + t:  a = (float) clip((double)mu[e] + sigma[i] z, -yaw_step, +yaw_step), product and sum rounded
 *           separately (the library is built with -ffp-contract=off), yaw_step the env's float32 widened
 * THE DEVIATE  z = ((double)S 2^-32 - 2.0) 1.7320508075688772, S the exact 64-bit sum of the four 32-bit words of
 *   philox4x32_10(seed, ctr, stream = i), ctr = ((uint64)b << 32) | (uint32)(k H N + e), b the farm's index IN THE PARENT: a
 *   farm's draws do not depend on chunking, on its place in `farms` or on the batch.  z has mean 0 and unit variance, lies
 *   in [-3.4642, 3.4642], and takes no transcendental: the same in NumPy and on the device.
 * SCORING as the lookahead extension scores: the trajectory of candidate k by the fused env step's transition from the
 *   parent's env state; evaluator row k H + h holds the yaw AFTER step h under wind h; the row reward and its normaliser as
 *   wflookahead.h states them; ret_k = sum_h g_h r_h in ascending h.
 * UPDATE after iteration i:
 *   rank_k = #{j : ret_j > ret_k or (ret_j == ret_k and j < k)}; the elites are rank < E
 *   mu[e]  = (float)((sum over the elites in ASCENDING k of (double)a_k[e]) / E): the sum first, the one division last
 *   winner = the largest return, the lowest index among equals; a winner other than 0 becomes the best sequence so far
 * OUTPUTS (any may be NULL)
 *   plan         [n][H][N] float32, the best sequence seen
 *   plan_return  [n] double, the winner's return in the last iteration
 *   hold_return  [n] double, candidate 0 of iteration 0
 *   first_action [n][N] float32, plan's row 0
 *   final_yaw    [n][N] float32, the yaw after walking plan
 *   mean         [n][H][N] float32, the last mu: shifted by one step it is the next call's mean0
 * No floating-point atomics and no order that depends on scheduling: two runs, and any chunking, give identical bits from
 * identical step outputs.
 *
 * ACCURACY, the rule wflookahead.h states: returns of two candidates closer than the sum of their bounds are not ordered
 * reliably.  Here an order decides who is elite and who wins, so a farm's plan has the reference's bits when, in every
 * iteration, the last elite and the first non-elite, and the winner and the runner-up, are further apart than that (rows of
 * identical yaw tie exactly on both sides).  strict != 0 solves every row in float64.
 *
 * An object belongs to a parent handle, reads it and stores nothing in it; it must be destroyed BEFORE it.  It owns an
 * EVALUATOR as a lookahead object does: evaluator farm e = slot R + row, R = K H, chunks of max_eval_farms / R farms.  Per
 * chunk ONE kernel, wf_plan_advance_kernel, is launched I + 1 times, one workgroup per slot, with one wf_step of the
 * evaluator between two launches; launch v reduces iteration v - 1 (row rewards, returns, ranks, elite mean, winner) and
 * lays out iteration v (draws, trajectories, yaw rows), the last one writes the outputs instead.  wf_set_wind_counts is
 * called once per chunk: the rows' wind is the same in every iteration.  The candidates of an iteration are KEPT between
 * the two launches in a grow-only [C][K][H][N] float32 buffer — 4 C K H N bytes, as much as the evaluator's yaw block (8 MiB
 * for 65 536 rows of 32 turbines) — and not drawn again: the reduce reads E + 1 of the K sequences, the elites and the
 * winner, and a redraw would spend ten Philox rounds on each of their elements to save that one write.
 *
 * VERSION-1 LIMITS.  Those of wflookahead.h (the ON-THE-FLY path, ONE layout, one turbine definition), and: a parent
 * configured `discrete` is refused.  wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFPLAN_H
#define WFPLAN_H

#include "wflookahead.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_PLAN_KERNELS 1
#define WF_PLAN_MIN_K 3

typedef struct wf_plan wf_plan;

int wf_plan_create(wf_handle* h, wf_plan** out);
int wf_plan_destroy(wf_plan* p);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's R = K H rows (checked when a run starts,
 *                   where K and H are known); <= 0: the default 65 536 */
int wf_plan_config(wf_plan* p, int strict, int max_eval_farms);

/* Plans for the listed farms, from the wind and the env state the parent holds at the time of the call.
 *   H, K, E, I, sigma, seed, gamma   as above; sigma is always a HOST array of I doubles
 *   wind        [n_farms][H][2] double, or NULL = the parent's current wind held
 *   mean0       [n_farms][H][N] float, block i belongs to farms[i], or NULL = zeros
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   plan, plan_return, hold_return, first_action, final_yaw, mean   as above; any may be NULL
 * on_device != 0: wind, mean0 and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_lookahead_run).
 * WF_E_INVALID: no wind set, no env state (wf_env_config and wf_env_reset come first), H outside 1 .. WF_LOOKAHEAD_MAX_H,
 * K < 3, K H > WF_LOOKAHEAD_MAX_ROWS, E outside 1 .. K, I < 1, sigma NULL or an entry negative or not finite, gamma outside
 * [0, 1] or not finite, a farm index out of range, max_eval_farms below K H.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts (wf_set_layouts*) or with turbine definitions
 * (wf_set_turbine_types); a parent configured discrete. */
int wf_plan_run(wf_plan* p, int H, int K, int E, int I, const double* sigma, unsigned long long seed, double gamma,
                const double* wind, const float* mean0, int n_farms, const int* farms, float* plan, double* plan_return,
                double* hold_return, float* first_action, float* final_yaw, float* mean, int on_device);

/* detail != 0: the following wf_plan_run calls record 2 I + 2 HIP events per chunk, so that wf_plan_last_timing can split
 * the total into step and glue time.  Default 0: two events per run. */
int wf_plan_set_timing(wf_plan* p, int detail);

/* HIP-event milliseconds of the last wf_plan_run (synchronises): from its first to its last launch; of these the evaluator's
 * wf_set_wind_counts + wf_step calls, and the glue kernel's launches (both 0 unless wf_plan_set_timing asked for the split).
 * Pointers may be NULL. */
int wf_plan_last_timing(wf_plan* p, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/plan_timing.py).  Owned by the object. */
wf_handle* wf_plan_evaluator(wf_plan* p);

/* Register / LDS footprint of the kernel as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_PLAN_KERNELS][3] ints: row wf_plan_advance_kernel (its LDS is dynamic). */
int wf_plan_kernel_info(wf_plan* p, int* info);

const char* wf_plan_last_error(wf_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* WFPLAN_H */
