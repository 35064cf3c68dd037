/* wfpolsearch.h — policy search on the device: a cross-entropy method over the weights of one small MLP policy, scored by the
 * closed-loop rollouts of include/wfpolicy.h or, over a wind ensemble, of include/wfpolscen.h, the whole search enqueued in one
 * call — the policy-search extension of libwfstep.so (include/wfstep.h).
 *
 * Every family the project scores on the device has a search over it: action sequences (wf_plan_run, wf_scenplan_run), yaw-table
 * controllers (the grid of wf_rollout_run), wake-model sets (wf_calib_fit).  This is the one over MLP policies: the loop an
 * evolution strategy runs around wf_policy_run — draw a population, aggregate its fitness over the farms, refit mean and width
 * per weight — with the population, the fitness and the refit on the device and nothing read back between two iterations.
 * This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the oracle: tests/search_ref.py restates it in NumPy over
 * tests/policy_ref.py and tests/polscen_ref.py.
 *
 * INPUTS  the network of wf_policy_set_network (P parameters); a start vector mean0 [P] float32, finite; widths sigma0 [P]
 *   float32, each >= 0 and finite; K candidates, WF_POLSEARCH_MIN_K <= K <= WF_POLSEARCH_MAX_K; E elites, 1 <= E <= K;
 *   I iterations, 1 <= I <= WF_POLSEARCH_MAX_ITER — the iteration number is the Philox stream, and stays below the member
 *   paths' streams 16 to 18 (include/wfscenario.h), as in wf_plan_run and wf_calib_fit; sigma_min >= 0, double; seed; and the
 *   arguments of the scorer.
 * SCORER  A farm's score of candidate k is
 *   held wind or a wind per step    wf_policy_run's returns[b][k], with H, gamma, wind;
 *   M members given (M > 0)         wf_polscen_run's score[b][k], with H, M, process, bounds, scenario_seed, gamma, tail,
 *                                   risk_weight, anchor; every iteration uses the same scenario_seed, as wf_scenplan_run does.
 *   The env state and the wind are read and never changed.
 * ITERATION i = 0 .. I - 1
 *   1. CANDIDATES C_i [K][P] float32.  Row 0 is the incumbent — at i = 0 mean0 —, row 1 the mean; row k >= 2, element p, is
 *      (float)((double)mean_p + (double)sigma_p z), product and sum rounded separately, z = the deviate of ext/wf_deviate.h for
 *      (seed, counter ((u64)k << 32) | p, stream i): tests/plan_ref.py's deviate(seed, k, p, i).  A draw depends on
 *      (seed, k, p, i) only: not on the farms, a farm list, chunking or K.  There is no clip.
 *   2. FITNESS F_i[k]: the farm scores of the n listed farms, in list order, added in float64 — inside each tile of
 *      WF_POLSEARCH_TILE = 256 list positions in ascending position from 0.0, the tile sums then in ascending tile from 0.0 —
 *      and the total divided once by (double)n.
 *   3. RANKS  rank_k = #{j: g_j > g_k or (g_j == g_k and j < k)}, g = F_i with every value that is not finite replaced by -inf
 *      (the stored F_i keeps the raw value).  The winner is the rank-0 candidate: ties go to the lowest index, so the incumbent
 *      is replaced only when strictly beaten, and where no fitness is finite the winner is candidate 0.
 *      incumbent <- C_i[winner], a copy of its bits; best_fitness <- F_i[winner].
 *   4. REFIT  The elites are the candidates of rank < E.  With sums over the elites in ascending k, all float64:
 *      m_p = (sum (double)C_i[k][p]) / (double)E;  v_p = (sum d d) / (double)E, d = (double)C_i[k][p] - m_p;
 *      mean_p <- (float)m_p;  sigma_p <- (float)(sqrt(v_p) + sigma_min), sqrt correctly rounded.
 *      A weight with sigma0_p = 0 under sigma_min = 0 therefore stays at mean0_p in every candidate, bit for bit.
 *   The rollouts are deterministic and nothing they read changes between two iterations: F_i[0] has the bits of best_fitness
 *   after iteration i - 1, and best_fitness never decreases.
 * OUTPUTS (any may be NULL; host or device pointers as on_device says)
 *   best_params   [P] float32      the incumbent after the last iteration
 *   best_fitness, init_fitness  [1] double; init_fitness = F_0[0], the start vector's fitness
 *   mean, sigma   [P] float32      after the last refit: the next call's warm start
 *   fitness       [I][K] double    winner [I] int
 *   candidates    [I][K][P] float32
 *   sigma_history [I][P] float32   the widths iteration i drew with; row 0 is sigma0
 *   farm_scores   [I][n][K] double what the scorer returned
 * No floating-point atomics and no order that depends on scheduling: two runs, any chunking of the scorer and host or device
 * arrays give identical bits from identical step outputs.
 *
 * An object is created ON the handle's policy object and, optionally, its polscen object (as a rollout object on the rose
 * object): it OWNS NO EVALUATOR.  It enqueues wf_policy_run / wf_polscen_run with on_device = 1 on its own candidate and score
 * buffers; network, strict and max_eval_farms are those objects' settings.  A later wf_policy_run(candidates[i]) on the same
 * handle therefore runs on the very evaluator the search used, and its returns carry the same bits in both modes.  It must be
 * destroyed BEFORE the two objects it borrows.  Between two scorer runs stand TWO launches of this extension: the tile sums
 * (wf_polsearch_tiles_kernel: a workgroup per tile of 256 positions) and the advance (wf_polsearch_advance_kernel: the tile
 * sums added and divided, ranks and winner in LDS, then refit and next candidates, a workgroup per slice of eight candidate
 * rows); the advance is launched I + 1 times, the first seeds from mean0 and sigma0, the last writes the outputs.  A whole
 * search is enqueued on the parent's stream with no host read between its launches, with the exceptions wf_policy_run names.
 *
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFPOLSEARCH_H
#define WFPOLSEARCH_H

#include "wfpolicy.h"
#include "wfpolscen.h"
#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_POLSEARCH_KERNELS 2
#define WF_POLSEARCH_MIN_K 3
#define WF_POLSEARCH_MAX_K 64
#define WF_POLSEARCH_MAX_ITER 16
#define WF_POLSEARCH_TILE 256

typedef struct wf_polsearch wf_polsearch;

/* policy: the handle's policy object (the held-wind scorer); scen: its polscen object (the ensemble scorer), or NULL — a
 * search with members is then refused.  WF_E_INVALID: a NULL handle or policy object. */
int wf_polsearch_create(wf_handle* h, wf_policy* policy, wf_polscen* scen, wf_polsearch** out);
int wf_polsearch_destroy(wf_polsearch* s);

/* The search, from the wind and the env state the parent holds at the time of the call.
 *   mean0, sigma0   [P] float
 *   K, E, I, sigma_min, seed   as above
 *   H, gamma        the scorer's horizon and discount
 *   wind            M == 0: [n_farms][H][2] double, or NULL = the parent's current wind held (wf_policy_run); M > 0: NULL
 *   M               0: wf_policy_run scores; > 0: wf_polscen_run scores over M members, with
 *   process, ws_lo, ws_hi, scenario_seed, tail, risk_weight, anchor ([n_farms][2] or NULL)   as wf_polscen_run takes them
 *   farms           [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   the outputs as above; any may be NULL
 * on_device != 0: mean0, sigma0, wind, anchor and the outputs are device pointers and the call only enqueues work on the
 * parent's stream — with wf_policy_run's exceptions: a growing buffer, an evaluator rebuild, a `farms` list.  A host caller's
 * mean0, sigma0 and anchor are checked; a device caller's are not.  The VALUES of `wind` are checked for neither caller, as
 * wf_policy_run checks none: only its shape follows from n_farms and H.
 * WF_E_INVALID, by name: K, E or I outside their ranges; a non-finite mean0; a negative or non-finite sigma0 or sigma_min;
 * mean0 or sigma0 NULL; members on an object created without a polscen object; a wind given with members; and everything the
 * scorer refuses, with its own message — among it no network set and a P that is not the network's parameter count. */
int wf_polsearch_run(wf_polsearch* s, const float* mean0, const float* sigma0, int P, int K, int E, int I, double sigma_min,
                     unsigned long long seed, int H, double gamma, const double* wind, int M, const wf_wind_process* process,
                     double ws_lo, double ws_hi, unsigned long long scenario_seed, int tail, double risk_weight, const double* anchor,
                     int n_farms, const int* farms, float* best_params, double* best_fitness, double* init_fitness, float* mean,
                     float* sigma, double* fitness, int* winner, float* candidates, float* sigma_history, double* farm_scores,
                     int on_device);

/* detail != 0: the following wf_polsearch_run calls record 2 I + 2 HIP events, so that wf_polsearch_last_timing can split the
 * total.  Default 0: two events per run. */
int wf_polsearch_set_timing(wf_polsearch* s, int detail);

/* HIP-event milliseconds of the last wf_polsearch_run (synchronises): from its first to its last launch; of these the scorer's
 * runs, and this extension's own kernels (both 0 unless wf_polsearch_set_timing asked for the split).  Pointers may be NULL. */
int wf_polsearch_last_timing(wf_polsearch* s, float* total_ms, float* scorer_ms, float* own_ms);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_POLSEARCH_KERNELS][3] ints: rows wf_polsearch_tiles_kernel, wf_polsearch_advance_kernel (the
 * LDS of both is dynamic). */
int wf_polsearch_kernel_info(wf_polsearch* s, int* info);

const char* wf_polsearch_last_error(wf_polsearch* s);

#ifdef __cplusplus
}
#endif
#endif /* WFPOLSEARCH_H */
