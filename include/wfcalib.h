/* wfcalib.h — wake-model calibration on the device: candidate parameter sets (include/wfmodelset.h: wf_model_set) scored
 * against measured turbine powers, and a cross-entropy fit of the eighteen fields to them — the calib extension of
 * libwfstep.so (include/wfstep.h).
 *
 * wf_set_model_sets gives every farm of a batch its own wake-model fields.  A calibration written over it builds a handle of
 * S C farms, sets a batch of candidates, steps, sums squares and draws again on the host: every batch of candidates then goes
 * through the host-side construction of its constants, an allocation, an upload and two stream drains.  Here the candidates'
 * constants are WRITTEN ON THE DEVICE into the evaluator's table, and ONE glue kernel stands between two evaluator steps: the
 * pattern of the planner (include/wfplan.h), over model fields instead of action sequences.  wf_calib_score is to wf_calib_fit
 * what wf_lookahead_run is to wf_plan_run.  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle:
 * tests/calib_ref.py restates it in NumPy over the float64 oracle.
 *
 * THE PARENT supplies the model (every field outside a set), ONE layout and ONE turbine definition.  It needs no wind, no env
 * state and no batch larger than 1; it is read and never changed.
 *
 * OBSERVATIONS.  G independent problems (a site, a direction sector, a time window) of C conditions each; host or device
 * pointers (on_device):
 *   ws, wd   [G][C]    double   the wind of each condition
 *   yaw      [G][C][N] float32  the yaw of each condition
 *   power    [G][C][N] double   measured power, watts
 *   weight   [G][C][N] double   >= 0 and finite, or NULL = ones; 0 masks a turbine that was off-line and pads a problem with
 *                               fewer conditions
 *   scale    double, > 0, watts (the Python layer: the rated power of the handle's table)
 * A host caller's ws, wd, yaw, power and weight are validated (finite, weight >= 0; a power under a weight of 0 may be
 * anything, NaN included: an off-line turbine as a logger records it); a device caller's are not read on the host.
 * WHAT A NaN DOES.  An entry of weight 0 adds +0 to its row whatever stands there.  Under a positive weight a NaN power (or a
 * NaN weight, or a solve that produced one) makes the loss not finite, and a loss that is not finite COUNTS AS +inf, as an
 * invalid candidate's does: it ranks last, never first.  Where every loss of a problem is +inf the winner is candidate 0, the
 * lowest index among equals: `best` is 0, a fit keeps its starting set and reports best_loss = +inf.
 *
 * LOSS of candidate set s on problem g, float64, every operation rounded once (the library is built with -ffp-contract=off):
 *   L[g][s] = sum_c ( sum_t w[g][c][t] * (((double)P_dev[g][s][c][t] - P[g][c][t]) / scale)^2 )
 * a term of weight 0 being +0; the inner sum in ascending t from 0.0, the outer one in ascending c from 0.0; P_dev the float32
 * power the float64 kernels (csrc/wf_resolve_ms.hip, csrc/wf_resolve4_ms.hip) write for evaluator row (g, s, c).  No
 * floating-point atomics: two runs, any chunking and any max_eval_farms give the same bits.
 *
 * THE FIT: the cross-entropy method of include/wfplan.h over the eighteen fields, in wf_model_set's order.
 *   lo, hi [18]  bounds; lo == hi fixes a field
 *   init         [G] or [1] starting sets (NULL: wf_model_set_from_model), each valid and inside [lo, hi]
 *   S >= 3 candidates, E elites in 1 .. S, I iterations in 1 .. WF_CALIB_MAX_ITER
 *   sigma [I]    a HOST array: finite non-negative fractions of hi - lo — the caller supplies the refining widths; nothing is
 *                fitted, the kernel takes no square root
 *   seed         64 bits
 * CANDIDATES of iteration i, mu the current mean (init before iteration 0):
 *   s = 0   the best set so far; in iteration 0 init: the fit is never worse than its start
 *   s = 1   mu
 *   s >= 2  field f:  clip(mu_f + (sigma[i] * (hi_f - lo_f)) * z, lo_f, hi_f) in float64, the two products and the sum rounded
 *           separately; z = wf_deviate(seed, ((uint64)g << 32) | (uint32)(s * 18 + f), stream = i) (csrc/ext/wf_deviate.h), g the
 *           problem's index in the call: a problem's draws do not depend on chunking.  A field with lo == hi stays at lo exactly
 * AN INVALID CANDIDATE fails what wf_set_model_sets asks of a set (ambient_ti, alpha, defl_alpha, ka TI + kb, defl_ka TI +
 *   defl_kb, ch_constant all > 0).  Its loss is +inf; its rows are solved under the problem's init constants, so that the kernels
 *   stay inside the model's domain; it is counted in n_invalid.
 * UPDATE after iteration i:
 *   rank_s = #{j : L_j < L_s or (L_j == L_s and j < s)}; the elites are rank < E
 *   mu_f   = (sum over the elites in ASCENDING s of field f) / E: the sum first, the one division last
 *   winner = the lowest loss, the lowest index among equals; a winner other than 0 becomes the best set so far
 *
 * ACCURACY.  A device power is inside parity.TOL_F64 of the oracle's (delta per turbine); a loss is then inside
 * sum w (2 |e| delta + delta^2) / scale^2 of the reference's, e the reference's residual.  Two losses closer than the sum of
 * their bounds are not ordered reliably: best_set and mean have the reference's bits where, in every iteration, every elite and
 * every non-elite, and the winner and the runner-up, are further apart than that.
 *
 * THE EVALUATOR.  An object owns one, as a plan object does: row (slot, s, c) = (slot S + s) C + c, chunks of
 * max_eval_farms / (S C) problems through the extensions' row driver with I rounds.  It holds C_slots S parameter sets, every
 * one the parent's model, with set_of[row] = slot S + s, set through wf_set_model_sets when it is (re)built: the host code
 * fills every member of its table a set does not own.  The glue kernel then overwrites IN PLACE the set-owned members of the
 * table's WfResolveConsts (csrc/modelset/wf_resolve_set.h: a device restatement of those lines of fill_resolve_consts, with
 * csrc/wf_f64_math.h's pow_any and sincos_any in place of the host's libm: the constants differ from wf_set_model_sets' by a
 * few ulp and are NOT bit-identical to them.  The contract is the oracle tolerance, not bits against the host-built table).
 * Per chunk ONE kernel, wf_calib_advance_kernel, one workgroup per slot, is launched I + 1 times with one wf_step between two
 * launches: launch v reduces iteration v - 1 (row sums, candidate sums, ranks, elite mean, winner, the winner's rows) and lays
 * out iteration v (draws, validity, constants; launch 0 also writes the rows' wind and yaw, ONCE per chunk), the last one
 * writes the outputs instead.  wf_calib_score is the same kernel with the candidates given instead of drawn, and I = 1.
 *
 * LIMITS, each refused by name: C >= 1; S <= WF_CALIB_MAX_S; S C <= max_eval_farms; N as the handle allows.
 * WF_E_UNSUPPORTED: a parent with several layouts, with turbine definitions, or one that itself holds parameter sets.
 * wfstep.h, wfmodelset.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFCALIB_H
#define WFCALIB_H

#include "wfmodelset.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_CALIB_KERNELS 1
#define WF_CALIB_FIELDS 18  /* doubles in a wf_model_set */
#define WF_CALIB_MIN_S 3    /* of a fit: the best so far, the mean, a draw */
#define WF_CALIB_MAX_S 1024
#define WF_CALIB_MAX_ITER 16

typedef struct wf_calib wf_calib;

int wf_calib_create(wf_handle* h, wf_calib** out);
int wf_calib_destroy(wf_calib* p);

/* max_eval_farms: upper bound of the evaluator's batch; it must hold one problem's S C rows (checked when a run starts);
 * <= 0: the default 65 536.  Every row is solved in float64: an evaluator that holds parameter sets knows no other mode. */
int wf_calib_config(wf_calib* p, int max_eval_farms);

/* The losses of given candidate sets.
 *   G, C, S       problems, conditions per problem, candidates per problem (1 <= S <= WF_CALIB_MAX_S)
 *   sets          a HOST array, validated as wf_set_model_sets validates: [G][S] (per_problem != 0) or [S] shared by all problems
 *   ws .. scale   the observations, as above
 *   loss          [G][S] double
 *   best          [G] int: the lowest loss, the lowest index among equals
 *   row_power     [G][S][C][N] float32, the evaluator's rows; any output may be NULL
 * on_device != 0: the observations and the outputs are device pointers and the call only enqueues work on the parent's stream
 * — except that it drains the stream first when a buffer has to grow or the evaluator has to be rebuilt. */
int wf_calib_score(wf_calib* p, int G, int C, int S, const wf_model_set* sets, int per_problem, const double* ws, const double* wd,
                   const float* yaw, const double* power, const double* weight, double scale, double* loss, int* best,
                   float* row_power, int on_device);

/* The fit.
 *   lo, hi, sigma, init   HOST arrays; init [G] (init_per_problem != 0) or [1], or NULL = the parent's model as a set
 *   best_set   [G] wf_model_set         best_loss, init_loss [G] double (init_loss: candidate 0 of iteration 0)
 *   history    [G][I] double, the winner's loss per iteration, non-increasing
 *   mean       [G] wf_model_set, the last mu
 *   fit_power  [G][C][N] float32, the best set's rows of the iteration that found it
 *   n_invalid  [G] int, invalid candidates over all iterations; any output may be NULL
 * WF_E_INVALID, by name: G < 1, C < 1, S outside 3 .. WF_CALIB_MAX_S, S C > max_eval_farms, E outside 1 .. S, I outside
 * 1 .. WF_CALIB_MAX_ITER, sigma NULL or an entry negative or not finite, a bound not finite or lo > hi, an init set invalid or
 * outside [lo, hi], scale not > 0, and of a host caller's observations: a value not finite, a negative weight. */
int wf_calib_fit(wf_calib* p, int G, int C, int S, int E, int I, const double* sigma, unsigned long long seed, const double* lo,
                 const double* hi, const wf_model_set* init, int init_per_problem, const double* ws, const double* wd,
                 const float* yaw, const double* power, const double* weight, double scale, wf_model_set* best_set,
                 double* best_loss, double* init_loss, double* history, wf_model_set* mean, float* fit_power, int* n_invalid,
                 int on_device);

/* detail != 0: the following runs record 2 I + 2 HIP events per chunk, so that wf_calib_last_timing can split the total into
 * step and glue time.  Default 0: two events per run. */
int wf_calib_set_timing(wf_calib* p, int detail);

/* HIP-event milliseconds of the last run (synchronises): from its first to its last launch; of these the evaluator's
 * wf_set_wind_counts + wf_step calls, and the glue kernel's launches (both 0 unless wf_calib_set_timing asked for the split).
 * Pointers may be NULL. */
int wf_calib_last_timing(wf_calib* p, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch a
 * run uses (tools/calib_timing.py).  Owned by the object.  Its HOST sets (wf_get_model_sets) are C_slots S copies of the
 * parent's model and NO LONGER DESCRIBE ITS DEVICE TABLE, whose set-owned members the last run's candidates have overwritten:
 * a wf_step on it solves under those candidates. */
wf_handle* wf_calib_evaluator(wf_calib* p);

/* Register / LDS footprint of the kernel as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_CALIB_KERNELS][3] ints: row wf_calib_advance_kernel. */
int wf_calib_kernel_info(wf_calib* p, int* info);

const char* wf_calib_last_error(wf_calib* p);

#ifdef __cplusplus
}
#endif
#endif /* WFCALIB_H */
