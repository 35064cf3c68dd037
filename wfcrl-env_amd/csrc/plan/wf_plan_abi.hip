// wf_plan_abi.hip — the C boundary of the plan extension (include/wfplan.h): an object that belongs to a parent handle, owns
// an evaluator handle and its device buffers, and enqueues a whole planning run on the parent's stream.  The run is the
// extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K H rows per farm, the evaluator and its steps
// for power and load, events), with I rounds per chunk: this file supplies its own checks, the I + 1 launches of the one
// kernel (wf_plan_kernels.hip) as the driver's lay-out, advance and reduce, and names the caller's arrays to stage.  What the
// launches of a run share goes to the device once, before the first of them (WfPlanRun: plan/wf_plan.h says why).  Reads
// the parent (layout, model, wind, env parameters and env state, kernel choice, resolve mode); stores nothing in it.
#include <cmath>
#include <vector>

#include "../../../include/wfplan.h"
#include "../ext/wf_ext.h"
#include "../../../include/wfwindgen.h"
#include "../series/wf_series.h"
#include "wf_plan.h"

using namespace wfi;

struct wf_plan : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  int series_ahead = 0;    // wf_plan_set_series (include/wfseries.h): the rows' wind is the window of the series' coming rows
  const wf_windgen* wind_source = nullptr;  // wf_plan_set_wind_source (include/wfwindgen.h): that series is a generator's, not the parent's
  // device buffers (grow-only)
  row_batch rows;          // E = C K H farms, with loads
  dev_buf<double> d_window;  // [n_farms][H][2] that window, laid out like a caller's wind
  dev_buf<float> d_cand;   // [E][N] the candidates of an iteration, kept from its lay-out to its reduce
  dev_buf<float> d_best;   // [C][H][N] best sequence so far
  dev_buf<float> d_mu;     // [C][H][N] the mean
  dev_buf<char> d_stage;   // staging for host callers: wind, mean0; plan, plan_return, hold_return, first_action, final_yaw, mean
  dev_buf<WfPlanRun> d_run;  // what the launches of a run share ...
  WfPlanRun run{};           // ... its host copy: the upload reads it ...
  hipEvent_t run_read = nullptr;  // ... and has done so when this event is reached
  evaluator eval;
  ~wf_plan() { if (run_read) hipEventDestroy(run_read); }
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the plans start at the fused env's state)";

}  // namespace

extern "C" {

int wf_plan_create(wf_handle* h, wf_plan** out) { return ext_create(h, out); }

int wf_plan_destroy(wf_plan* p) { return ext_destroy(p); }

int wf_plan_config(wf_plan* p, int strict, int max_eval_farms) {
  if (!p) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  p->strict = strict != 0; p->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_plan_set_timing(wf_plan* p, int detail) {
  if (!p) return WF_E_INVALID;
  p->detail = detail != 0;
  return WF_OK;
}

int wf_plan_set_series(wf_plan* p, int ahead) {
  if (!p) return WF_E_INVALID;
  p->series_ahead = ahead != 0;
  return WF_OK;
}

int wf_plan_set_wind_source(wf_plan* p, wf_windgen* g) {
  if (!p) return WF_E_INVALID;
  p->wind_source = g;
  return WF_OK;
}

int wf_plan_run(wf_plan* p, int H, int K, int E, int I, const double* sigma, unsigned long long seed, double gamma,
                const double* wind, const float* mean0, int n_farms, const int* farms, float* plan, double* plan_return,
                double* hold_return, float* first_action, float* final_yaw, float* mean, int on_device) {
  if (!p) return WF_E_INVALID;
  wf_handle* h = p->h;
  const int N = h->N;
  const bool ahead = p->series_ahead != 0;
  row_batch& b = p->rows;
  const double* d_wind = nullptr;
  const float* d_mean0 = nullptr;
  float *d_plan = nullptr, *d_fa = nullptr, *d_fy = nullptr, *d_mean = nullptr;
  double *d_pr = nullptr, *d_hr = nullptr;
  std::vector<double> sg;  // the caller's sigma, copied: a launch takes its entry by value
  staging st(p, p->d_stage, on_device);
  bool uploaded = false;
  row_policy k;
  k.what = "planning serves"; k.name = "wf_plan_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = p->strict; k.max_eval = p->max_eval;
  k.check = [&]() -> int {
    if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(p, WF_E_INVALID, "the horizon H must be in 1..64");
    if (K < WF_PLAN_MIN_K || K > WF_LOOKAHEAD_MAX_ROWS / H)
      return ext_fail(p, WF_E_INVALID, "the number of candidates K must be >= 3 (the best so far, the mean, a draw) with K H <= 4096");
    if (E < 1 || E > K) return ext_fail(p, WF_E_INVALID, "the number of elites E must be in 1..K");
    if (I < 1) return ext_fail(p, WF_E_INVALID, "the number of iterations I must be >= 1");
    if (!sigma) return ext_fail(p, WF_E_INVALID, "wf_plan_run: sigma is NULL");
    for (int i = 0; i < I; ++i)
      if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return ext_fail(p, WF_E_INVALID, "every sigma must be finite and non-negative");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return ext_fail(p, WF_E_INVALID, "gamma must be finite and in [0, 1]");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(p, WF_E_INVALID, kNoEnv);
    if (h->env.discrete)
      return ext_fail(p, WF_E_UNSUPPORTED, "planning serves the continuous action encoding: this handle is configured discrete (wf_env_config)");
    if (ahead) {
      const int rc = series_ahead_check(p, p->wind_source, wind != nullptr, H);
      if (rc != WF_OK) return rc;
    }
    sg.assign(sigma, sigma + I);
    k.rows = K * H; k.rounds = I;
    return WF_OK;
  };
  k.reserve = [&](int C, int Ev) -> int {
    int rc = reserve(p, p->d_cand, (size_t)Ev * N);
    if (rc == WF_OK) rc = reserve(p, p->d_best, (size_t)C * H * N);
    if (rc == WF_OK) rc = reserve(p, p->d_mu, (size_t)C * H * N);
    if (rc == WF_OK) rc = reserve(p, p->d_run, 1);
    if (rc != WF_OK) return rc;
    const size_t fh = (size_t)n_farms * H;
    st.in(wind, fh * 2, &d_wind); st.in(mean0, fh * N, &d_mean0);
    if (ahead) {  // (the farm list is on the device by now: run_rows uploads it before this hook)
      rc = series_ahead_window(p, p->wind_source, p->d_window, H, n_farms, farms ? b.farms.d.p : nullptr);
      if (rc != WF_OK) return rc;
      d_wind = p->d_window;
    }
    st.out(plan, fh * N, &d_plan); st.out(plan_return, (size_t)n_farms, &d_pr); st.out(hold_return, (size_t)n_farms, &d_hr);
    st.out(first_action, (size_t)n_farms * N, &d_fa); st.out(final_yaw, (size_t)n_farms * N, &d_fy); st.out(mean, fh * N, &d_mean);
    return WF_OK;
  };
  // the run's block, once the staging has given the caller's arrays their device pointers: before the first launch
  auto upload = [&](int Ev) -> int {
    if (!p->run_read) WFX_HIP(p, hipEventCreateWithFlags(&p->run_read, hipEventDisableTiming));
    else WFX_HIP(p, hipEventSynchronize(p->run_read));  // (the previous run's upload has read the host copy)
    WfPlanRun& r = p->run;
    r = WfPlanRun{};
    r.N = N; r.K = K; r.H = H; r.E = E; r.I = I;
    r.wind_stride = h->wind_count == 1 ? 0 : 1;
    r.load_coef = h->env.load_coef; r.gamma = gamma; r.seed = seed;
    r.ws = h->d_ws; r.wd = h->d_wd;
    r.ws_prev = (!ahead && h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed; series-ahead: the current speed
    r.env = env_view(h); r.env.discrete = 0;
    r.yaw = b.d_yaw; r.ews = b.d_wind; r.ewd = b.d_wind + Ev;
    r.power_ev = b.d_pow; r.load_ev = b.d_load;
    r.cand = p->d_cand; r.best = p->d_best; r.mu = p->d_mu;
    r.wind = d_wind; r.mean0 = d_mean0;
    r.plan = d_plan; r.plan_return = d_pr; r.hold_return = d_hr; r.first_action = d_fa; r.final_yaw = d_fy; r.mean = d_mean;
    WFX_HIP(p, hipMemcpyAsync(p->d_run, &r, sizeof(WfPlanRun), hipMemcpyHostToDevice, h->stream));
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
    WFX_HIP(p, wfk_launch_plan_advance(&p->run, p->d_run, &sl, v, v < I ? sg[v] : 0.0, h->stream));
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int Ev) -> int { return launch(sl, Ev, 0); };
  k.advance = [&](const WfSlots& sl, int Ev, int r) -> int { return launch(sl, Ev, r); };
  k.reduce = [&](const WfSlots& sl, int Ev) -> int { return launch(sl, Ev, I); };
  return run_rows(p, b, p->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | launch 0 e1 | wind + step e2 | launch 1 e3 | step e4 | ... | launch I e
int wf_plan_last_timing(wf_plan* p, float* total_ms, float* step_ms, float* glue_ms) {
  if (!p) return WF_E_INVALID;
  return last_timing(p, "wf_plan_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_plan_evaluator(wf_plan* p) { return p ? p->eval.ev : nullptr; }

int wf_plan_kernel_info(wf_plan* p, int* info) {
  if (!p || !info) return ext_fail(p, WF_E_INVALID, "wf_plan_kernel_info: NULL argument");
  return kernel_info(p, WF_PLAN_KERNELS, wfk_plan_func_attributes, info);
}

const char* wf_plan_last_error(wf_plan* p) { return p ? p->err.c_str() : "wf_plan: NULL object"; }

}  // extern "C"
