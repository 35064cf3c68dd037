/* wfpolicy.h — closed-loop rollouts of MLP policies on the device: what each of K parameter vectors of one small network
 * earns over the next H steps of the fused env, the network observing what the env would show it after every step — the
 * policy extension of libwfstep.so (include/wfstep.h).
 *
 * Action sequences (include/wflookahead.h) and yaw-table controllers (include/wfrollout.h) are scored in one call because
 * their yaw does not depend on the wake solve: all K H rows of a farm are rows of ONE batched step.  A network policy observes
 * the per-turbine local wind speed and direction, which come OUT of the solve, so its steps are sequential: this extension
 * runs ONE batched step per env step, K rows per farm, with one glue kernel between two steps and no host read.  It serves
 * the evaluation of a checkpoint over many farms (K = 1) and of a population of parameter vectors (evolution strategies,
 * CEM policy search, PBT, checkpoint selection: K > 1).  This is THE PROJECT'S OWN definition.  PARITY UNPINNED beyond the
 * oracle: tests/policy_ref.py restates it in NumPy over the float64 oracle.
 *
 * POLICY CLASS.  A deterministic MLP of L linear layers, 1 <= L <= WF_POLICY_MAX_LAYERS, hidden widths <=
 * WF_POLICY_MAX_WIDTH, of one of two kinds:
 *   WF_POLICY_CENTRAL  input: the env's flattened observation, D = 3 N + 2 — yaw [N], local wind speed [N], local wind
 *                      direction [N], free wind (speed, direction), caller's turbine order; output N (continuous encoding) or
 *                      3 N (discrete encoding, turbine-major: outputs 3 t .. 3 t + 2 belong to turbine t)
 *   WF_POLICY_SHARED   input: one turbine's (yaw_t, ws_t, wd_t), with use_freewind also the free wind: D = 3 or 5; output 1
 *                      or 3.  The same weights serve every turbine: the parameter-shared decentralised agent
 * PARAMETERS  params [K][P] float32, 1 <= K <= WF_POLICY_MAX_K, the same K policies for every farm.  A vector is laid out
 *   as torch.nn.utils.parameters_to_vector lays out an nn.Sequential of nn.Linear: per layer the weight [out][in] row-major,
 *   then the bias [out]; P = sum_l (in_l + 1) out_l.  shift [D], scale [D] double: the input normalisation (NULL: 0 and 1).
 * ARITHMETIC, all float64, every product and sum rounded separately (no fused multiply-add):
 *   input       x_i = ((double)obs_i - shift_i) scale_i
 *   layer       z_o = (double)b_o, then for i ascending z_o = z_o + (double)W[o][i] x_i
 *   hidden      one activation per network: WF_POLICY_RELU (z > 0 ? z : 0), WF_POLICY_SOFTSIGN (z / (1 + |z|), one correctly
 *               rounded division) or WF_POLICY_TANH (1 - 2 / (exp(2 c) + 1), c = z clamped to +-20, exp the library's
 *               exp_lean: a few ulp)
 *   last layer  linear, then `final` (WF_POLICY_NONE, WF_POLICY_SOFTSIGN or WF_POLICY_TANH) f and out_scale
 *   continuous  a_t = (float)(out_scale f(z_t)), rounded once; the env's transition then clips it to +-yaw_step
 *   discrete    the action of turbine t is the index of the largest of its three outputs f(z), the lowest index among equals
 *   With relu and softsign a NumPy loop reproduces the device's bits; with tanh the float64 value is a few ulp off and the
 *   float32 action differs by at most one float32 ulp.  The fixed order rules out the matrix pipe: intended.
 *
 * CLOSED LOOP of policy k on farm b, from the env state (y, acc, moves) of the farm, which is READ ONLY here:
 *   round 0     solves the CURRENT yaw under the farm's current wind: its wind_speed / wind_dir outputs, y and the current
 *               wind are observation 0.  The extension computes this itself: no observation is taken from the caller.
 *   for h = 0 .. H - 1
 *     the action comes from observation h;
 *     the fused env step's transition (budget gate, increment, clip: include/wflookahead.h, move counter moves + 1 + h) gives
 *     the yaw after step h; acc += |increment|;
 *     that row is solved under wind h: the current wind held, or wind [n_farms][H][2] as wf_lookahead_run takes it;
 *     its reward is wf_lookahead_run's ROW REWARD, load term included: step 0 normalised by the pending prev-wind speed
 *     (wf_env_set_prev_wind), else the current speed — NOT consumed —, step h >= 1 by the speed of wind h - 1;
 *     observation h + 1 is the new yaw, that solve's local wind and wind h.
 *   ret = sum_h g_h r_h, g_0 = 1, g_h = g_{h-1} gamma, added in ascending h, product and sum rounded separately.
 *   best = the policy of the largest return, the lowest index among equal maxima.
 * OUTPUTS (any may be NULL)
 *   returns      [n_farms][K] double
 *   rewards      [n_farms][K][H] double
 *   farm_power   [n_farms][K][H] double (W)
 *   actions      [n_farms][K][H][N] float32, RAW: what wf_env_step / wf_lookahead_run take
 *   observations [n_farms][K][H][3 N + 2] float32, un-normalised, the CENTRAL lay-out for both kinds
 *   final_yaw    [n_farms][K][N] float32
 *   gated        [n_farms][K] int, (step, turbine) pairs with a closed budget gate
 *   best         [n_farms] int
 * No floating-point atomics and no order that depends on scheduling: two runs, any chunking and any farm list give identical
 * bits from identical step outputs.  Feeding `actions` of policy k to wf_lookahead_run (same mode, same wind) returns this
 * run's rewards, farm_power, returns and final_yaw.
 *
 * An object belongs to a parent handle, reads it (layout, model, wind, env parameters and env state, kernel choice, resolve
 * mode) and stores nothing in it; it must be destroyed BEFORE it.  It owns an EVALUATOR: a further wf_handle on the parent's
 * device and stream, K rows per farm: evaluator farm e = k C + slot in a chunk of C farm slots (chunk = the largest farm count
 * with chunk K <= max_eval_farms).  Per chunk: ONE begin kernel writes the round-0 rows; then H + 1 steps of the evaluator
 * (power, load, local wind) with ONE advance kernel between two of them — reward of the step before, observation, network,
 * transition, next yaw row — and, under a wind per step, wf_set_wind_counts on the evaluator after it; ONE reduce kernel forms
 * the last reward and the outputs.  The parameters are uploaded once per call and transposed on the device to [in][out].  A
 * whole run is enqueued without a host round trip between its launches.
 *
 * VERSION-1 LIMITS.  The evaluator is given device arrays, a wind per row, so it always runs on the ON-THE-FLY path.  A parent
 * with several layouts, several turbine definitions or wake-model parameter sets per farm is refused.  No series source on
 * the C side: a caller on a time-series episode passes the series' coming rows as `wind`.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFPOLICY_H
#define WFPOLICY_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_POLICY_KERNELS 4
#define WF_POLICY_MAX_H 256
#define WF_POLICY_MAX_K 64
#define WF_POLICY_MAX_LAYERS 4
#define WF_POLICY_MAX_WIDTH 256

#define WF_POLICY_CENTRAL 0
#define WF_POLICY_SHARED 1

#define WF_POLICY_NONE 0
#define WF_POLICY_RELU 1
#define WF_POLICY_SOFTSIGN 2
#define WF_POLICY_TANH 3

typedef struct wf_policy wf_policy;

int wf_policy_create(wf_handle* h, wf_policy** out);
int wf_policy_destroy(wf_policy* p);

/* The evaluator: a new object holds strict 0, 65 536 evaluator farms.
 *   strict != 0     the evaluator solves every row in float64 (wf_set_risk_resolve mode 2); otherwise the parent's mode
 *   max_eval_farms  upper bound of the evaluator's batch; it must hold one farm's K rows (checked when a run starts, where K is
 *                   known); <= 0: the default 65 536 */
int wf_policy_config(wf_policy* p, int strict, int max_eval_farms);

/* The network the following runs evaluate (copied; a new object holds none).
 *   kind          WF_POLICY_CENTRAL or WF_POLICY_SHARED
 *   n_layers      L; widths [L + 1]: widths[0] = D, widths[l + 1] = the outputs of layer l
 *   activation    of the hidden layers: WF_POLICY_RELU, WF_POLICY_SOFTSIGN or WF_POLICY_TANH
 *   final         after the last layer: WF_POLICY_NONE, WF_POLICY_SOFTSIGN or WF_POLICY_TANH
 *   use_freewind  WF_POLICY_SHARED: the input also holds the free wind (D = 5, else 3); ignored for WF_POLICY_CENTRAL
 *   out_scale     finite
 *   shift, scale  [D] HOST arrays, or NULL = 0 / 1; finite
 * WF_E_INVALID: an unknown kind, L outside 1 .. WF_POLICY_MAX_LAYERS, a hidden width outside 1 .. WF_POLICY_MAX_WIDTH, an
 * unknown activation, a non-finite shift, scale or out_scale.  What depends on the parent — D and the output width against
 * its N and action encoding — is checked when a run starts. */
int wf_policy_set_network(wf_policy* p, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind,
                          double out_scale, const double* shift, const double* scale);

/* Closed-loop returns of the K policies on the listed farms, from the wind and the env state the parent holds at the time of
 * the call.
 *   params      [K][P] float, P the network's parameter count
 *   wind        [n_farms][H][2] double, or NULL = the parent's current wind held
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   returns .. best   as above; any may be NULL
 * on_device != 0: params, wind and the outputs are device pointers and the call only enqueues work on the parent's stream —
 * except that it drains the stream first when a buffer has to grow, when the evaluator has to be rebuilt and when a `farms`
 * list is given (as wf_lookahead_run).
 * WF_E_INVALID: no wind set, no env state, no network set, params == NULL, a parameter vector of the wrong length (P),
 * H outside 1 .. WF_POLICY_MAX_H, K outside 1 .. WF_POLICY_MAX_K, gamma outside [0, 1] or not finite, an input width that is
 * not the kind's D, an output width that does not match the env's action encoding, a farm index out of range, max_eval_farms
 * below K.
 * WF_E_UNSUPPORTED (version 1): a parent with several layouts, with turbine definitions or with wake-model parameter sets. */
int wf_policy_run(wf_policy* p, const float* params, int K, int P, int H, const double* wind, double gamma, int n_farms,
                  const int* farms, double* returns, double* rewards, double* farm_power, float* actions, float* observations,
                  float* final_yaw, int* gated, int* best, int on_device);

/* detail != 0: the following wf_policy_run calls record 2 (H + 1) + 2 HIP events per chunk, so that wf_policy_last_timing can
 * split the total into step and glue time.  Default 0: two events per run. */
int wf_policy_set_timing(wf_policy* p, int detail);

/* HIP-event milliseconds of the last wf_policy_run (synchronises): from its first to its last launch; of these the
 * evaluator's wf_step calls, and the glue — the kernels of this extension and, under a wind per step, the evaluator's
 * wf_set_wind_counts between two steps (both 0 unless wf_policy_set_timing asked for the split).  Pointers may be NULL. */
int wf_policy_last_timing(wf_policy* p, float* total_ms, float* step_ms, float* glue_ms);

/* The evaluator handle (NULL before the first run): for introspection and for timing a plain wf_step loop on the very batch
 * a run uses (tools/policy_timing.py).  Owned by the object. */
wf_handle* wf_policy_evaluator(wf_policy* p);

/* Register / LDS footprint of the kernels as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_POLICY_KERNELS][3] ints: rows wf_policy_transpose_kernel, wf_policy_begin_kernel,
 * wf_policy_advance_kernel, wf_policy_reduce_kernel (the LDS of the last two is dynamic). */
int wf_policy_kernel_info(wf_policy* p, int* info);

const char* wf_policy_last_error(wf_policy* p);

#ifdef __cplusplus
}
#endif
#endif /* WFPOLICY_H */
