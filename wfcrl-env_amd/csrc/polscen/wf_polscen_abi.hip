// wf_polscen_abi.hip — the C boundary of the policy-scenario extension (include/wfpolscen.h): an object that belongs to a parent
// handle, owns an evaluator handle and its device buffers, and enqueues a whole run on the parent's stream.  The run is the
// extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K M rows per farm, the evaluator and its steps for
// power, load and local wind, events) with H + 1 rounds per chunk, exactly as policy/ drives it: this file supplies its own
// checks — the union of the policy extension's (policy/wf_policy_host.h) and the scenario extension's —, the paths kernel and
// the policy extension's begin kernel as the driver's lay-out, the H launches of the policy extension's advance kernel, each
// followed by wf_set_wind_counts on the evaluator, and the returns and statistics kernels as the reduce, and names the
// caller's arrays to stage.  What the launches of a run share goes to the device once, before the first of them (WfPolicyRun).
// Reads the parent (layout, model, wind, env parameters and env state, kernel choice, resolve mode); stores nothing in it — in
// particular the speed a wf_env_set_prev_wind left for the next env step stays for that step, and is not read here.
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/wfpolscen.h"
#include "../../../include/wflookahead.h"
#include "../../../include/wfscenario.h"
#include "../ensemble/wf_ensemble_host.h"
#include "../ext/wf_ext.h"
#include "../policy/wf_policy_host.h"
#include "wf_polscen.h"

using namespace wfi;

static_assert(WF_POLSCEN_MAX_H == WF_LOOKAHEAD_MAX_H, "the deviate's counter m * 64 + u - 1 is the scenario extension's keying");
static_assert(WF_POLSCEN_MAX_MEMBERS == WF_SCENARIO_MAX_MEMBERS && WF_POLSCEN_MAX_K == WF_POLICY_MAX_K, "the limits of both parents");
static_assert(WF_POLSCEN_KERNELS == 3 + WF_POLICY_KERNELS - 1, "three kernels of its own and the policy extension's transpose, begin and advance");
static_assert(staging::kMaxSegs >= 15, "a run names two inputs and thirteen outputs");

struct wf_polscen : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  bool has_net = false;
  WfPolicyNet net{};
  std::vector<double> norm;   // [2][D] shift, scale as set
  // device buffers (grow-only)
  row_batch rows;             // E = C K M farms, with loads and local wind
  dev_buf<float> d_wt;        // [K][P] the transposed parameters
  dev_buf<float> d_acc;       // [E][N] the rows' accumulators
  dev_buf<double> d_ret, d_disc;  // [E] the rows' return so far and next discount
  dev_buf<int> d_gated;       // [E] the rows' closed gates
  dev_buf<double> d_mret;     // [E] the rows' member returns
  dev_buf<double> d_paths;    // [C][M][H][2] the chunk's member paths
  dev_buf<double> d_norm;     // [2][D] shift, scale ...
  std::vector<double> norm_up;    // ... the host copy the upload reads
  dev_buf<WfPolicyRun> d_run;     // what the launches of a run share ...
  WfPolicyRun run{};              // ... its host copy: the upload reads it ...
  hipEvent_t run_read = nullptr;  // ... and both uploads have read theirs when this event is reached
  dev_buf<char> d_stage;      // staging for host callers: params, anchor; the thirteen outputs
  evaluator eval;
  ~wf_polscen() { if (run_read) hipEventDestroy(run_read); }
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K M";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the rollouts start at the fused env's state)";

}  // namespace

extern "C" {

int wf_polscen_create(wf_handle* h, wf_polscen** out) { return ext_create(h, out); }

int wf_polscen_destroy(wf_polscen* p) { return ext_destroy(p); }

int wf_polscen_config(wf_polscen* p, int strict, int max_eval_farms) {
  if (!p) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  p->strict = strict != 0; p->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_polscen_set_timing(wf_polscen* p, int detail) {
  if (!p) return WF_E_INVALID;
  p->detail = detail != 0;
  return WF_OK;
}

int wf_polscen_set_network(wf_polscen* p, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind,
                           double out_scale, const double* shift, const double* scale) {
  if (!p) return WF_E_INVALID;
  const int rc = policy_network(p, kind, n_layers, widths, activation, final, use_freewind, out_scale, shift, scale, &p->net, &p->norm);
  if (rc == WF_OK) p->has_net = true;
  return rc;
}

int wf_polscen_run(wf_polscen* p, const float* params, int K, int P, int H, int M, const wf_wind_process* process, double ws_lo,
                   double ws_hi, unsigned long long seed, double gamma, int tail, double risk_weight, const double* anchor,
                   int n_farms, const int* farms, double* expected_returns, double* cvar, double* score, double* member_returns,
                   double* rewards, double* farm_power, double* wind_paths, float* actions, float* observations, float* final_yaw,
                   int* gated, float* first_action, int* best, int on_device) {
  if (!p) return WF_E_INVALID;
  wf_handle* h = p->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  row_batch& b = p->rows;
  const float* d_par = nullptr;
  const double* d_anchor = nullptr;
  double *d_exp = nullptr, *d_cvar = nullptr, *d_score = nullptr, *d_mr = nullptr, *d_rew = nullptr, *d_fp = nullptr, *d_wp = nullptr;
  float *d_act = nullptr, *d_obs = nullptr, *d_fy = nullptr, *d_first = nullptr;
  int *d_gat = nullptr, *d_best = nullptr;
  staging st(p, p->d_stage, on_device);
  WfPolicyNet net = p->net;
  WfPolicyPlan plan{};
  bool uploaded = false;
  row_policy k;
  k.what = "policy scenarios serve"; k.name = "wf_polscen_run";
  k.rows_msg = kRowsMsg; k.loads = true; k.local_wind = true;
  k.strict = p->strict; k.max_eval = p->max_eval;
  k.check = [&]() -> int {
    if (!p->has_net) return ext_fail(p, WF_E_INVALID, "no network: wf_polscen_set_network comes first");
    if (H < 1 || H > WF_POLSCEN_MAX_H) return ext_fail(p, WF_E_INVALID, "the horizon H must be in 1..64");
    if (K < 1 || K > WF_POLSCEN_MAX_K) return ext_fail(p, WF_E_INVALID, "the number of policies K must be in 1..64");
    if (M < 1 || M > WF_POLSCEN_MAX_MEMBERS) return ext_fail(p, WF_E_INVALID, "the number of members M must be in 1..64");
    int rc = check_ensemble_statistics(p, M, tail, risk_weight, gamma);
    if (rc != WF_OK) return rc;
    if (!params) return ext_fail(p, WF_E_INVALID, "wf_polscen_run: params is NULL");
    rc = check_ensemble_process(p, "wf_polscen_run", process, ws_lo, ws_hi);
    if (rc != WF_OK) return rc;
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(p, WF_E_INVALID, kNoEnv);
    rc = check_ensemble_anchor(p, anchor, n_farms, on_device);
    if (rc == WF_OK) rc = policy_network_fits(p, h, net, P);
    if (rc != WF_OK) return rc;
    k.rows = K * M; k.rounds = H + 1;
    return WF_OK;
  };
  k.reserve = [&](int C, int E) -> int {
    const int D = net.width[0];
    int rc = reserve(p, p->d_wt, (size_t)K * P);
    if (rc == WF_OK) rc = reserve(p, p->d_acc, (size_t)E * N);
    if (rc == WF_OK) rc = reserve(p, p->d_ret, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_disc, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_gated, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_mret, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_paths, (size_t)C * M * H * 2);
    if (rc == WF_OK) rc = reserve(p, p->d_norm, 2 * (size_t)D);
    if (rc == WF_OK) rc = reserve(p, p->d_run, 1);
    if (rc != WF_OK) return rc;
    plan = wf_policy_plan(net, N, M * C);  // (a tile is T consecutive rows of a policy's M C)
    if (plan.lds_bytes > 64 * 1024) return ext_fail(p, WF_E_UNSUPPORTED, "policy scenarios serve farms whose one row fits the advance kernel's LDS: this layout is too large");
    const size_t fk = (size_t)n_farms * K, fkm = fk * M, fr = fkm * H;
    st.in(params, (size_t)K * P, &d_par); st.in(anchor, (size_t)n_farms * 2, &d_anchor);
    st.out(expected_returns, fk, &d_exp); st.out(cvar, fk, &d_cvar); st.out(score, fk, &d_score);
    st.out(member_returns, fkm, &d_mr); st.out(rewards, fr, &d_rew); st.out(farm_power, fr, &d_fp);
    st.out(wind_paths, (size_t)n_farms * M * H * 2, &d_wp);
    st.out(actions, fr * N, &d_act); st.out(observations, fr * (3 * (size_t)N + 2), &d_obs);
    st.out(final_yaw, fkm * N, &d_fy); st.out(gated, fkm, &d_gat); st.out(first_action, fk * N, &d_first);
    st.out(best, (size_t)n_farms, &d_best);
    return WF_OK;
  };
  // once per call, after the staging has given the caller's arrays their device pointers and before the first launch: the
  // normalisation, the run's block and the transpose
  auto upload = [&](int E) -> int {
    if (!p->run_read) WFX_HIP(p, hipEventCreateWithFlags(&p->run_read, hipEventDisableTiming));
    else WFX_HIP(p, hipEventSynchronize(p->run_read));  // (the previous run's uploads have read the host copies)
    p->norm_up = p->norm;
    WFX_HIP(p, hipMemcpyAsync(p->d_norm, p->norm_up.data(), sizeof(double) * p->norm_up.size(), hipMemcpyHostToDevice, h->stream));
    WfPolicyRun& r = p->run;
    r = WfPolicyRun{};
    r.net = net; r.pl = plan;
    r.N = N; r.K = K; r.H = H; r.M = M;
    r.env = env_view(h);
    r.ws = h->d_ws; r.wd = h->d_wd; r.wind_stride = wind_stride;
    r.ws_prev = nullptr;  // step 0 is normalised by the current speed: a pending speed is neither used nor consumed
    r.load_coef = h->env.load_coef; r.gamma = gamma;
    r.params = d_par; r.wt = p->d_wt; r.shift = p->d_norm; r.scale = p->d_norm + net.width[0];
    r.yaw = b.d_yaw; r.power_ev = b.d_pow; r.load_ev = b.d_load; r.lws = b.d_lws; r.lwd = b.d_lwd;
    r.ews = b.d_wind; r.ewd = b.d_wind + E;
    r.st = WfPolicyState{p->d_acc, p->d_ret, p->d_disc, p->d_gated};
    r.wind = nullptr; r.paths = p->d_paths;
    r.returns = nullptr; r.rewards = d_rew; r.farm_power = d_fp; r.actions = d_act; r.observations = d_obs;
    r.final_yaw = d_fy; r.gated = d_gat; r.best = nullptr; r.first_action = d_first;
    WFX_HIP(p, hipMemcpyAsync(p->d_run, &r, sizeof(WfPolicyRun), hipMemcpyHostToDevice, h->stream));
    WFX_HIP(p, hipEventRecord(p->run_read, h->stream));
    WFX_HIP(p, wfk_launch_policy_transpose(&p->run, p->d_run, h->stream));
    uploaded = true;
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    if (!uploaded) {
      const int rc = upload(E);
      if (rc != WF_OK) return rc;
    }
    const size_t first = (size_t)sl.base;
    WfPolscenPathsArgs pa{};
    pa.sl = sl;
    pa.ens = ensemble_args(h, M, H, *process, ws_lo, ws_hi, seed, d_anchor, first);
    pa.paths = p->d_paths;
    pa.wind_paths = d_wp ? d_wp + first * M * H * 2 : nullptr;
    WFX_HIP(p, wfk_launch_polscen_paths(&pa, h->stream));
    WFX_HIP(p, wfk_launch_policy_begin(&p->run, p->d_run, &sl, h->stream));
    return WF_OK;
  };
  k.advance = [&](const WfSlots& sl, int E, int r) -> int {
    WFX_HIP(p, wfk_launch_policy_advance(&p->run, p->d_run, &sl, r, h->stream));
    // the kernel wrote member m's tick r into the rows' wind block; the evaluator takes it before its next step
    WFX_EV(p, p->eval.ev, wf_set_wind_counts(p->eval.ev, b.d_wind, E, b.d_wind + E, E, 1));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    WfPolscenReduceArgs ra{};
    ra.mret = p->d_mret; ra.member_returns = d_mr;
    ra.expected = d_exp; ra.cvar = d_cvar; ra.score = d_score; ra.best = d_best;
    ra.lam = risk_weight; ra.q = tail;
    WFX_HIP(p, wfk_launch_polscen_returns(&p->run, p->d_run, &sl, &ra, h->stream));
    WFX_HIP(p, wfk_launch_polscen_stats(&p->run, p->d_run, &sl, &ra, h->stream));
    return WF_OK;
  };
  return run_rows(p, b, p->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | paths + begin e1 | wind + step e2 | advance 1 + wind e3 | step e4 | ... | returns + statistics e
int wf_polscen_last_timing(wf_polscen* p, float* total_ms, float* step_ms, float* glue_ms) {
  if (!p) return WF_E_INVALID;
  return last_timing(p, "wf_polscen_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_polscen_evaluator(wf_polscen* p) { return p ? p->eval.ev : nullptr; }

int wf_polscen_kernel_info(wf_polscen* p, int* info) {
  if (!p || !info) return ext_fail(p, WF_E_INVALID, "wf_polscen_kernel_info: NULL argument");
  return kernel_info(p, WF_POLSCEN_KERNELS, wfk_polscen_func_attributes, info);
}

const char* wf_polscen_last_error(wf_polscen* p) { return p ? p->err.c_str() : "wf_polscen: NULL object"; }

}  // extern "C"
