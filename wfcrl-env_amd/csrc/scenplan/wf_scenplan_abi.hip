// wf_scenplan_abi.hip — the C boundary of the scenplan extension (include/wfscenplan.h): an object that belongs to a parent
// handle, owns an evaluator handle and its device buffers, and enqueues a whole scenario-planning run on the parent's stream.
// The run is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K M H rows per farm, the evaluator
// and its steps for power and load, events), with I rounds per chunk: this file supplies its own checks — those of its two
// parents, plan/ and scenario/ —, the paths kernel and the I + 1 launches of the advance kernel (wf_scenplan_kernels.hip) as the
// driver's lay-out, advance and reduce, and names the caller's arrays to stage.  What the advance launches of a run share goes
// to the device once, before the first of them (WfScenPlanRun).  Reads the parent (layout, model, wind, env parameters and env
// state, kernel choice, resolve mode); stores nothing in it — in particular the speed a wf_env_set_prev_wind left for the next
// env step stays for that step, and is not read here.
#include <cmath>
#include <vector>

#include "../../../include/wfscenplan.h"
#include "../ensemble/wf_ensemble_host.h"
#include "../ext/wf_ext.h"
#include "wf_scenplan.h"

using namespace wfi;

static_assert(WF_SCENARIO_MAX_ROWS == WF_LOOKAHEAD_MAX_ROWS, "the advance kernel's LDS is sized for the look-ahead's row limit");
static_assert(WF_SCENPLAN_MIN_K * 2048 > WF_SCENARIO_MAX_ROWS, "the paths kernel draws a farm's M H ticks in one tile");
static_assert(WF_SCENPLAN_MAX_ITERATIONS <= 16, "the planner's streams 0 .. I - 1 stay below the paths' streams 16 .. 18");

struct wf_scenplan : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  row_batch rows;          // E = C K M H farms, with loads
  dev_buf<float> d_cand;   // [C][K][H][N] the candidates of an iteration, kept from its lay-out to its reduce
  dev_buf<float> d_best;   // [C][H][N] best sequence so far
  dev_buf<float> d_mu;     // [C][H][N] the mean
  dev_buf<double> d_mret;  // [C][K][M] the last iteration's member returns
  dev_buf<double> d_stat;  // [C][K][2] ... and (mean, tail mean)
  dev_buf<char> d_stage;   // staging for host callers: anchor, mean0; the ten outputs
  dev_buf<WfScenPlanRun> d_run;  // what the advance launches of a run share ...
  WfScenPlanRun run{};           // ... its host copy: the upload reads it ...
  hipEvent_t run_read = nullptr;  // ... and has done so when this event is reached
  evaluator eval;
  ~wf_scenplan() { if (run_read) hipEventDestroy(run_read); }
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K M H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the plans start at the fused env's state)";

}  // namespace

extern "C" {

int wf_scenplan_create(wf_handle* h, wf_scenplan** out) { return ext_create(h, out); }

int wf_scenplan_destroy(wf_scenplan* p) { return ext_destroy(p); }

int wf_scenplan_config(wf_scenplan* p, int strict, int max_eval_farms) {
  if (!p) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  p->strict = strict != 0; p->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_scenplan_set_timing(wf_scenplan* p, int detail) {
  if (!p) return WF_E_INVALID;
  p->detail = detail != 0;
  return WF_OK;
}

int wf_scenplan_run(wf_scenplan* p, int H, int K, int E, int I, const double* sigma, unsigned long long seed, double gamma, int M,
                    const wf_wind_process* process, double ws_lo, double ws_hi, unsigned long long scenario_seed, int tail,
                    double risk_weight, const double* anchor, const float* mean0, int n_farms, const int* farms, float* plan,
                    double* plan_score, double* plan_expected, double* plan_cvar, double* plan_member_returns, double* hold_score,
                    float* first_action, float* final_yaw, float* mean, double* wind_paths, int on_device) {
  if (!p) return WF_E_INVALID;
  wf_handle* h = p->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  row_batch& b = p->rows;
  const double* d_anchor = nullptr;
  const float* d_mean0 = nullptr;
  float *d_plan = nullptr, *d_fa = nullptr, *d_fy = nullptr, *d_mean = nullptr;
  double *d_ps = nullptr, *d_pe = nullptr, *d_pc = nullptr, *d_pm = nullptr, *d_hs = nullptr, *d_paths = nullptr;
  std::vector<double> sg;  // the caller's sigma, copied: a launch takes its entry by value
  staging st(p, p->d_stage, on_device);
  bool uploaded = false;
  row_policy k;
  k.what = "scenario planning serves"; k.name = "wf_scenplan_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = p->strict; k.max_eval = p->max_eval;
  k.check = [&]() -> int {
    if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(p, WF_E_INVALID, "the horizon H must be in 1..64");
    if (M < 1 || M > WF_SCENARIO_MAX_MEMBERS) return ext_fail(p, WF_E_INVALID, "the number of members M must be in 1..64");
    if (K < WF_SCENPLAN_MIN_K || K > WF_SCENARIO_MAX_ROWS / (M * H))
      return ext_fail(p, WF_E_INVALID, "the number of candidates K must be >= 3 (the best so far, the mean, a draw) with K M H <= 4096");
    if (E < 1 || E > K) return ext_fail(p, WF_E_INVALID, "the number of elites E must be in 1..K");
    if (I < 1 || I > WF_SCENPLAN_MAX_ITERATIONS)
      return ext_fail(p, WF_E_INVALID, "the number of iterations I must be in 1..16 (the planner's streams stay below the paths' 16 to 18)");
    if (!sigma) return ext_fail(p, WF_E_INVALID, "wf_scenplan_run: sigma is NULL");
    for (int i = 0; i < I; ++i)
      if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return ext_fail(p, WF_E_INVALID, "every sigma must be finite and non-negative");
    int rc = check_ensemble(p, "wf_scenplan_run", M, tail, risk_weight, gamma, process, ws_lo, ws_hi);
    if (rc != WF_OK) return rc;
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(p, WF_E_INVALID, kNoEnv);
    if (h->env.discrete)
      return ext_fail(p, WF_E_UNSUPPORTED,
                      "scenario planning serves the continuous action encoding: this handle is configured discrete (wf_env_config)");
    rc = check_ensemble_anchor(p, anchor, n_farms, on_device);
    if (rc != WF_OK) return rc;
    sg.assign(sigma, sigma + I);
    k.rows = K * M * H; k.rounds = I;
    return WF_OK;
  };
  k.reserve = [&](int C, int) -> int {
    int rc = reserve(p, p->d_cand, (size_t)C * K * H * N);
    if (rc == WF_OK) rc = reserve(p, p->d_best, (size_t)C * H * N);
    if (rc == WF_OK) rc = reserve(p, p->d_mu, (size_t)C * H * N);
    if (rc == WF_OK) rc = reserve(p, p->d_mret, (size_t)C * K * M);
    if (rc == WF_OK) rc = reserve(p, p->d_stat, (size_t)C * K * 2);
    if (rc == WF_OK) rc = reserve(p, p->d_run, 1);
    if (rc != WF_OK) return rc;
    const size_t fh = (size_t)n_farms * H, f = (size_t)n_farms;
    st.in(anchor, f * 2, &d_anchor); st.in(mean0, fh * N, &d_mean0);
    st.out(plan, fh * N, &d_plan); st.out(plan_score, f, &d_ps); st.out(plan_expected, f, &d_pe); st.out(plan_cvar, f, &d_pc);
    st.out(plan_member_returns, f * M, &d_pm); st.out(hold_score, f, &d_hs);
    st.out(first_action, f * N, &d_fa); st.out(final_yaw, f * N, &d_fy); st.out(mean, fh * N, &d_mean);
    st.out(wind_paths, fh * M * 2, &d_paths);
    return WF_OK;
  };
  // the run's block, once the staging has given the caller's arrays their device pointers: before the first launch
  auto upload = [&](int Ev) -> int {
    if (!p->run_read) WFX_HIP(p, hipEventCreateWithFlags(&p->run_read, hipEventDisableTiming));
    else WFX_HIP(p, hipEventSynchronize(p->run_read));  // (the previous run's upload has read the host copy)
    WfScenPlanRun& r = p->run;
    r = WfScenPlanRun{};
    r.N = N; r.K = K; r.M = M; r.H = H; r.E = E; r.I = I; r.q = tail;
    r.wind_stride = wind_stride;
    r.load_coef = h->env.load_coef; r.gamma = gamma; r.lam = risk_weight; r.seed = seed;
    r.ws = h->d_ws;
    r.env = env_view(h); r.env.discrete = 0;
    r.yaw = b.d_yaw; r.ews = b.d_wind;
    r.power_ev = b.d_pow; r.load_ev = b.d_load;
    r.cand = p->d_cand; r.best = p->d_best; r.mu = p->d_mu; r.mret = p->d_mret; r.stat = p->d_stat;
    r.mean0 = d_mean0;
    r.plan = d_plan; r.plan_score = d_ps; r.plan_expected = d_pe; r.plan_cvar = d_pc; r.hold_score = d_hs;
    r.plan_member_returns = d_pm; r.first_action = d_fa; r.final_yaw = d_fy; r.mean = d_mean;
    WFX_HIP(p, hipMemcpyAsync(p->d_run, &r, sizeof(WfScenPlanRun), hipMemcpyHostToDevice, h->stream));
    WFX_HIP(p, hipEventRecord(p->run_read, h->stream));
    uploaded = true;
    return WF_OK;
  };
  // launch v of a chunk: the driver's lay-out is v = 0, its advance of round r is v = r, its reduce is v = I
  auto launch = [&](const WfSlots& sl, int Ev, int v) -> int {
    if (!uploaded) {
      const int rc = upload(Ev);
      if (rc != WF_OK) return rc;
    }
    WFX_HIP(p, wfk_launch_scenplan_advance(&p->run, p->d_run, &sl, v, v < I ? sg[v] : 0.0, h->stream));
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int Ev) -> int {
    const size_t first = (size_t)sl.base;
    WfScenPlanPathsArgs pa{};
    pa.sl = sl;
    pa.ens = ensemble_args(h, M, H, *process, ws_lo, ws_hi, scenario_seed, d_anchor, first);
    pa.K = K;
    pa.ews = b.d_wind; pa.ewd = b.d_wind + Ev;
    pa.wind_paths = d_paths ? d_paths + first * M * H * 2 : nullptr;
    WFX_HIP(p, wfk_launch_scenplan_paths(&pa, h->stream));
    return launch(sl, Ev, 0);
  };
  k.advance = [&](const WfSlots& sl, int Ev, int r) -> int { return launch(sl, Ev, r); };
  k.reduce = [&](const WfSlots& sl, int Ev) -> int { return launch(sl, Ev, I); };
  return run_rows(p, b, p->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | paths + launch 0 e1 | wind + step e2 | launch 1 e3 | step e4 | ... | launch I e
int wf_scenplan_last_timing(wf_scenplan* p, float* total_ms, float* step_ms, float* glue_ms) {
  if (!p) return WF_E_INVALID;
  return last_timing(p, "wf_scenplan_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_scenplan_evaluator(wf_scenplan* p) { return p ? p->eval.ev : nullptr; }

int wf_scenplan_kernel_info(wf_scenplan* p, int* info) {
  if (!p || !info) return ext_fail(p, WF_E_INVALID, "wf_scenplan_kernel_info: NULL argument");
  return kernel_info(p, WF_SCENPLAN_KERNELS, wfk_scenplan_func_attributes, info);
}

const char* wf_scenplan_last_error(wf_scenplan* p) { return p ? p->err.c_str() : "wf_scenplan: NULL object"; }

}  // extern "C"
