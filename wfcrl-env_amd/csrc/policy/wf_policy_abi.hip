// wf_policy_abi.hip — the C boundary of the policy extension (include/wfpolicy.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole closed-loop run on the parent's stream.  The run is the
// extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K rows per farm, the evaluator and its steps for
// power, load and local wind, events) with H + 1 rounds per chunk: this file supplies its own checks, the begin kernel as the
// driver's lay-out, the H launches of the advance kernel — each followed, under a wind per step, by wf_set_wind_counts on the
// evaluator — and the reduce (wf_policy_kernels.hip), and names the caller's arrays to stage.  What the launches of a run share
// goes to the device once, before the first of them (WfPolicyRun: policy/wf_policy.h says why); the parameters are transposed
// there before the first chunk.  Reads the parent (layout, model, wind, env parameters and env
// state, kernel choice, resolve mode); stores nothing in it — in particular the speed a wf_env_set_prev_wind left for the next
// env step stays for that step.
#include <cmath>
#include <string>
#include <vector>

#include "../../../include/wfpolicy.h"
#include "../ext/wf_ext.h"
#include "wf_policy.h"
#include "wf_policy_host.h"

using namespace wfi;

struct wf_policy : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  bool has_net = false;
  WfPolicyNet net{};
  std::vector<double> norm;   // [2][D] shift, scale as set
  // device buffers (grow-only)
  row_batch rows;             // E = C K farms, with loads and local wind
  dev_buf<float> d_wt;        // [K][P] the transposed parameters
  dev_buf<float> d_acc;       // [E][N] the rows' accumulators
  dev_buf<double> d_ret, d_disc;  // [E] the rows' return so far and next discount
  dev_buf<int> d_gated;       // [E] the rows' closed gates
  dev_buf<double> d_norm;     // [2][D] shift, scale ...
  std::vector<double> norm_up;    // ... the host copy the upload reads
  dev_buf<WfPolicyRun> d_run;     // what the launches of a run share ...
  WfPolicyRun run{};              // ... its host copy: the upload reads it ...
  hipEvent_t run_read = nullptr;  // ... and both uploads have read theirs when this event is reached
  dev_buf<char> d_stage;      // staging for host callers: params, wind; the eight outputs
  evaluator eval;
  ~wf_policy() { if (run_read) hipEventDestroy(run_read); }
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the rollouts start at the fused env's state)";

}  // namespace

// ---- what polscen/ shares (policy/wf_policy_host.h) ----
namespace wfi {

int policy_network(ext_base* p, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind, double out_scale,
                   const double* shift, const double* scale, WfPolicyNet* net, std::vector<double>* norm) {
  if (kind != WF_POLICY_CENTRAL && kind != WF_POLICY_SHARED)
    return ext_fail(p, WF_E_INVALID, "unknown policy kind: WF_POLICY_CENTRAL or WF_POLICY_SHARED");
  if (n_layers < 1 || n_layers > WF_POLICY_MAX_LAYERS) return ext_fail(p, WF_E_INVALID, "the number of layers L must be in 1..4");
  if (!widths) return ext_fail(p, WF_E_INVALID, "wf_policy_set_network: widths is NULL");
  for (int l = 0; l <= n_layers; ++l)
    if (widths[l] < 1) return ext_fail(p, WF_E_INVALID, "every width must be >= 1");
  for (int l = 1; l < n_layers; ++l)
    if (widths[l] > WF_POLICY_MAX_WIDTH) return ext_fail(p, WF_E_INVALID, "a hidden width must be in 1..256");
  if (activation != WF_POLICY_RELU && activation != WF_POLICY_SOFTSIGN && activation != WF_POLICY_TANH)
    return ext_fail(p, WF_E_INVALID, "unknown activation: WF_POLICY_RELU, WF_POLICY_SOFTSIGN or WF_POLICY_TANH");
  if (final != WF_POLICY_NONE && final != WF_POLICY_SOFTSIGN && final != WF_POLICY_TANH)
    return ext_fail(p, WF_E_INVALID, "unknown final activation: WF_POLICY_NONE, WF_POLICY_SOFTSIGN or WF_POLICY_TANH");
  if (!std::isfinite(out_scale)) return ext_fail(p, WF_E_INVALID, "out_scale must be finite");
  const int D = widths[0];
  for (int i = 0; i < D; ++i) {
    if (shift && !std::isfinite(shift[i])) return ext_fail(p, WF_E_INVALID, "every shift must be finite");
    if (scale && !std::isfinite(scale[i])) return ext_fail(p, WF_E_INVALID, "every scale must be finite");
  }
  WfPolicyNet n{};
  n.kind = kind; n.L = n_layers; n.act = activation; n.fin = final; n.use_freewind = use_freewind != 0;
  n.out_scale = out_scale;
  int off = 0;
  for (int l = 0; l <= n_layers; ++l) n.width[l] = widths[l];
  for (int l = 0; l < n_layers; ++l) {
    n.woff[l] = off; off += widths[l] * widths[l + 1];
    n.boff[l] = off; off += widths[l + 1];
  }
  n.P = off;
  *net = n;
  norm->assign(2 * (size_t)D, 0.0);
  for (int i = 0; i < D; ++i) {
    (*norm)[i] = shift ? shift[i] : 0.0;
    (*norm)[D + i] = scale ? scale[i] : 1.0;
  }
  return WF_OK;
}

int policy_network_fits(ext_base* p, const wf_handle* h, WfPolicyNet& net, int P) {
  const int N = h->N;
  const int D = net.kind == WF_POLICY_CENTRAL ? 3 * N + 2 : (net.use_freewind ? 5 : 3);
  if (net.width[0] != D)
    return ext_fail(p, WF_E_INVALID, "the network's input width does not match its kind: 3 N + 2 (central), 3 or 5 (shared)");
  const int per = h->env.discrete ? 3 : 1, want = net.kind == WF_POLICY_CENTRAL ? per * N : per;
  if (net.width[net.L] != want)
    return ext_fail(p, WF_E_INVALID, "the network's output width does not match the env's action encoding: N or 3 N (central), 1 or 3 (shared)");
  if (P != net.P)
    return ext_fail(p, WF_E_INVALID, "a parameter vector of the wrong length: P must be sum_l (in_l + 1) out_l, " + std::to_string(net.P) + " for this network");
  net.discrete = h->env.discrete;
  return WF_OK;
}

}  // namespace wfi

extern "C" {

int wf_policy_create(wf_handle* h, wf_policy** out) { return ext_create(h, out); }

int wf_policy_destroy(wf_policy* p) { return ext_destroy(p); }

int wf_policy_config(wf_policy* p, int strict, int max_eval_farms) {
  if (!p) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  p->strict = strict != 0; p->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_policy_set_timing(wf_policy* p, int detail) {
  if (!p) return WF_E_INVALID;
  p->detail = detail != 0;
  return WF_OK;
}

int wf_policy_set_network(wf_policy* p, int kind, int n_layers, const int* widths, int activation, int final, int use_freewind,
                          double out_scale, const double* shift, const double* scale) {
  if (!p) return WF_E_INVALID;
  const int rc = policy_network(p, kind, n_layers, widths, activation, final, use_freewind, out_scale, shift, scale, &p->net, &p->norm);
  if (rc == WF_OK) p->has_net = true;
  return rc;
}

int wf_policy_run(wf_policy* p, const float* params, int K, int P, int H, const double* wind, double gamma, int n_farms,
                  const int* farms, double* returns, double* rewards, double* farm_power, float* actions, float* observations,
                  float* final_yaw, int* gated, int* best, int on_device) {
  if (!p) return WF_E_INVALID;
  wf_handle* h = p->h;
  const int N = h->N;
  row_batch& b = p->rows;
  const float* d_par = nullptr;
  const double* d_wind = nullptr;
  double *d_ret = nullptr, *d_rew = nullptr, *d_fp = nullptr;
  float *d_act = nullptr, *d_obs = nullptr, *d_fy = nullptr;
  int *d_gat = nullptr, *d_best = nullptr;
  staging st(p, p->d_stage, on_device);
  WfPolicyNet net = p->net;
  WfPolicyPlan plan{};
  bool uploaded = false;
  row_policy k;
  k.what = "policy rollouts serve"; k.name = "wf_policy_run";
  k.rows_msg = kRowsMsg; k.loads = true; k.local_wind = true;
  k.strict = p->strict; k.max_eval = p->max_eval;
  k.check = [&]() -> int {
    if (!p->has_net) return ext_fail(p, WF_E_INVALID, "no network: wf_policy_set_network comes first");
    if (H < 1 || H > WF_POLICY_MAX_H) return ext_fail(p, WF_E_INVALID, "the horizon H must be in 1..256");
    if (K < 1 || K > WF_POLICY_MAX_K) return ext_fail(p, WF_E_INVALID, "the number of policies K must be in 1..64");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return ext_fail(p, WF_E_INVALID, "gamma must be finite and in [0, 1]");
    if (!params) return ext_fail(p, WF_E_INVALID, "wf_policy_run: params is NULL");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(p, WF_E_INVALID, kNoEnv);
    const int rc = policy_network_fits(p, h, net, P);
    if (rc != WF_OK) return rc;
    k.rows = K; k.rounds = H + 1;
    return WF_OK;
  };
  k.reserve = [&](int C, int E) -> int {
    const int D = net.width[0];
    int rc = reserve(p, p->d_wt, (size_t)K * P);
    if (rc == WF_OK) rc = reserve(p, p->d_acc, (size_t)E * N);
    if (rc == WF_OK) rc = reserve(p, p->d_ret, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_disc, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_gated, (size_t)E);
    if (rc == WF_OK) rc = reserve(p, p->d_norm, 2 * (size_t)D);
    if (rc == WF_OK) rc = reserve(p, p->d_run, 1);
    if (rc != WF_OK) return rc;
    plan = wf_policy_plan(net, N, C);
    if (plan.lds_bytes > 64 * 1024) return ext_fail(p, WF_E_UNSUPPORTED, "policy rollouts serve farms whose one row fits the advance kernel's LDS: this layout is too large");
    const size_t fk = (size_t)n_farms * K, fr = fk * H;
    st.in(params, (size_t)K * P, &d_par); st.in(wind, (size_t)n_farms * H * 2, &d_wind);
    st.out(returns, fk, &d_ret); st.out(rewards, fr, &d_rew); st.out(farm_power, fr, &d_fp);
    st.out(actions, fr * N, &d_act); st.out(observations, fr * (3 * (size_t)N + 2), &d_obs);
    st.out(final_yaw, fk * N, &d_fy); st.out(gated, fk, &d_gat); st.out(best, (size_t)n_farms, &d_best);
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
    r.N = N; r.K = K; r.H = H; r.M = 1;  // (no ensemble: paths and first_action stay null)
    r.env = env_view(h);
    r.ws = h->d_ws; r.wd = h->d_wd; r.wind_stride = h->wind_count == 1 ? 0 : 1;
    r.ws_prev = (h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed
    r.load_coef = h->env.load_coef; r.gamma = gamma;
    r.params = d_par; r.wt = p->d_wt; r.shift = p->d_norm; r.scale = p->d_norm + net.width[0];
    r.yaw = b.d_yaw; r.power_ev = b.d_pow; r.load_ev = b.d_load; r.lws = b.d_lws; r.lwd = b.d_lwd;
    r.ews = b.d_wind; r.ewd = b.d_wind + E;
    r.st = WfPolicyState{p->d_acc, p->d_ret, p->d_disc, p->d_gated};
    r.wind = d_wind;
    r.returns = d_ret; r.rewards = d_rew; r.farm_power = d_fp; r.actions = d_act; r.observations = d_obs;
    r.final_yaw = d_fy; r.gated = d_gat; r.best = d_best;
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
    WFX_HIP(p, wfk_launch_policy_begin(&p->run, p->d_run, &sl, h->stream));
    return WF_OK;
  };
  k.advance = [&](const WfSlots& sl, int E, int r) -> int {
    WFX_HIP(p, wfk_launch_policy_advance(&p->run, p->d_run, &sl, r, h->stream));
    // a wind per step: the kernel wrote the wind of step r - 1 into the rows' block; the evaluator takes it before its next step
    if (d_wind) WFX_EV(p, p->eval.ev, wf_set_wind_counts(p->eval.ev, b.d_wind, E, b.d_wind + E, E, 1));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    WFX_HIP(p, wfk_launch_policy_reduce(&p->run, p->d_run, &sl, h->stream));
    return WF_OK;
  };
  return run_rows(p, b, p->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | begin e1 | wind + step e2 | advance 1 (+ wind) e3 | step e4 | ... | reduce e
int wf_policy_last_timing(wf_policy* p, float* total_ms, float* step_ms, float* glue_ms) {
  if (!p) return WF_E_INVALID;
  return last_timing(p, "wf_policy_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_policy_evaluator(wf_policy* p) { return p ? p->eval.ev : nullptr; }

int wf_policy_kernel_info(wf_policy* p, int* info) {
  if (!p || !info) return ext_fail(p, WF_E_INVALID, "wf_policy_kernel_info: NULL argument");
  return kernel_info(p, WF_POLICY_KERNELS, wfk_policy_func_attributes, info);
}

const char* wf_policy_last_error(wf_policy* p) { return p ? p->err.c_str() : "wf_policy: NULL object"; }

}  // extern "C"
