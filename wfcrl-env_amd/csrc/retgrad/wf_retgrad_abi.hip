// wf_retgrad_abi.hip — the C boundary of the retgrad extension (include/wfretgrad.h): an object that belongs to a parent
// handle, owns an evaluator handle and its device buffers, and enqueues a whole return-gradient run on the parent's stream.
// The run is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K H (2 N + 1) rows per farm, the
// evaluator and its step for power and load, events); this file supplies its own checks, a chunk's lay-out, reduce and best
// launches (wf_retgrad_kernels.hip) and names the caller's arrays to stage.  Reads the parent (layout, model, wind, env
// parameters and env state, kernel choice, resolve mode); stores nothing in it — in particular the speed a
// wf_env_set_prev_wind left for the next env step stays for that step.
#include <cmath>

#include "../../../include/wfretgrad.h"
#include "../ext/wf_ext.h"
#include "../../../include/wfwindgen.h"
#include "../series/wf_series.h"
#include "wf_retgrad.h"

using namespace wfi;

struct wf_retgrad : ext_base {
  // configuration
  int strict = 0, max_eval = WF_RETGRAD_DEFAULT_EVAL_FARMS;
  int series_ahead = 0;   // wf_retgrad_set_series: the rows' wind is the window of the series' coming rows
  const wf_windgen* wind_source = nullptr;  // wf_retgrad_set_wind_source (include/wfwindgen.h): that series is a generator's, not the parent's
  // device buffers (grow-only)
  row_batch rows;                   // E = C K H (2 N + 1) farms, with loads
  dev_buf<double> d_div;            // [C][K][H][N] the divisors
  dev_buf<unsigned char> d_flags;   // [C][K][H][N] the pass flags
  dev_buf<double> d_ret;            // [C][K] the chunk's returns: what the best kernel reads
  dev_buf<double> d_window;         // [n_farms][H][2] the series window, laid out like a caller's wind
  dev_buf<char> d_stage;            // staging for host callers: actions, wind, terminal; the ten outputs
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K H (2 N + 1)";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the sequences start at the fused env's state)";

}  // namespace

extern "C" {

int wf_retgrad_create(wf_handle* h, wf_retgrad** out) { return ext_create(h, out); }

int wf_retgrad_destroy(wf_retgrad* r) { return ext_destroy(r); }

int wf_retgrad_config(wf_retgrad* r, int strict, int max_eval_farms) {
  if (!r) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = WF_RETGRAD_DEFAULT_EVAL_FARMS;
  r->strict = strict != 0; r->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_retgrad_set_timing(wf_retgrad* r, int detail) {
  if (!r) return WF_E_INVALID;
  r->detail = detail != 0;
  return WF_OK;
}

int wf_retgrad_set_series(wf_retgrad* r, int ahead) {
  if (!r) return WF_E_INVALID;
  r->series_ahead = ahead != 0;
  return WF_OK;
}

int wf_retgrad_set_wind_source(wf_retgrad* r, wf_windgen* g) {
  if (!r) return WF_E_INVALID;
  r->wind_source = g;
  return WF_OK;
}

int wf_retgrad_run(wf_retgrad* r, const float* actions, int K, int H, const double* wind, double gamma, double delta,
                   const double* terminal, int n_farms, const int* farms, double* returns, double* rewards, double* farm_power,
                   float* final_yaw, int* best, double* action_gradient, double* reward_gradient, double* state_gradient,
                   float* yaw, unsigned char* pass_mask, int on_device) {
  if (!r) return WF_E_INVALID;
  wf_handle* h = r->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool ahead = r->series_ahead != 0;
  row_batch& b = r->rows;
  const float* d_act = nullptr;
  const double *d_wind = nullptr, *d_term = nullptr;
  double *d_ret = nullptr, *d_rew = nullptr, *d_fp = nullptr, *d_ag = nullptr, *d_rg = nullptr, *d_sg = nullptr;
  float *d_fy = nullptr, *d_traj = nullptr;
  int* d_best = nullptr;
  unsigned char* d_mask = nullptr;
  staging st(r, r->d_stage, on_device);
  const WfEnvView env = env_view(h);
  row_policy k;
  k.what = "return gradients serve"; k.name = "wf_retgrad_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = r->strict; k.max_eval = r->max_eval;
  k.check = [&]() -> int {
    if (H < 1 || H > WF_RETGRAD_MAX_H) return ext_fail(r, WF_E_INVALID, "the horizon H must be in 1..64");
    if (K < 1) return ext_fail(r, WF_E_INVALID, "the number of sequences K must be >= 1");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return ext_fail(r, WF_E_INVALID, "gamma must be finite and in [0, 1]");
    if (!std::isfinite(delta) || !(delta > 0.0)) return ext_fail(r, WF_E_INVALID, "delta, the perturbation in degrees, must be finite and > 0");
    if (!actions) return ext_fail(r, WF_E_INVALID, "wf_retgrad_run: actions is NULL");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(r, WF_E_INVALID, kNoEnv);
    if (h->env.discrete) return ext_fail(r, WF_E_UNSUPPORTED, "return gradients serve the continuous action encoding only: the env is configured for the discrete encoding");
    if (N > WF_RETGRAD_MAX_N) return ext_fail(r, WF_E_UNSUPPORTED, "return gradients serve at most 1024 turbines");
    if (ahead) {
      const int rc = series_ahead_check(r, r->wind_source, wind != nullptr, H);
      if (rc != WF_OK) return rc;
    }
    const long long rows = (long long)K * H * (2 * N + 1);
    if (rows > (long long)k.max_eval) return ext_fail(r, WF_E_INVALID, kRowsMsg);
    k.rows = (int)rows;
    return WF_OK;
  };
  k.reserve = [&](int C, int) -> int {
    const size_t fk = (size_t)n_farms * K, fr = fk * H;
    const size_t ck = (size_t)C * K;
    int rc = reserve(r, r->d_div, ck * H * N);
    if (rc == WF_OK) rc = reserve(r, r->d_flags, ck * H * N);
    if (rc == WF_OK) rc = reserve(r, r->d_ret, ck);
    if (rc != WF_OK) return rc;
    st.in(actions, fr * N, &d_act); st.in(wind, (size_t)n_farms * H * 2, &d_wind); st.in(terminal, fk * N, &d_term);
    if (ahead) {  // (the farm list is on the device by now: run_rows uploads it before this hook)
      rc = series_ahead_window(r, r->wind_source, r->d_window, H, n_farms, farms ? b.farms.d.p : nullptr);
      if (rc != WF_OK) return rc;
      d_wind = r->d_window;
    }
    st.out(returns, fk, &d_ret); st.out(rewards, fr, &d_rew); st.out(farm_power, fr, &d_fp);
    st.out(final_yaw, fk * N, &d_fy); st.out(best, (size_t)n_farms, &d_best);
    st.out(action_gradient, fr * N, &d_ag); st.out(reward_gradient, fr * N, &d_rg); st.out(state_gradient, fk * N, &d_sg);
    st.out(yaw, fr * N, &d_traj); st.out(pass_mask, fr * N, &d_mask);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t first = (size_t)sl.base, seq = (size_t)K * H * N;
    WfRetgradLayoutArgs la{};
    la.sl = sl;
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N; la.K = K; la.H = H;
    la.env = env; la.delta = delta;
    la.actions = d_act + first * seq;
    la.wind = d_wind ? d_wind + first * H * 2 : nullptr;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    la.div = r->d_div; la.flags = r->d_flags;
    la.traj = d_traj ? d_traj + first * seq : nullptr;
    la.pass_mask = d_mask ? d_mask + first * seq : nullptr;
    la.final_yaw = d_fy ? d_fy + first * K * N : nullptr;
    WFX_HIP(r, wfk_launch_retgrad_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base, fk = first * K, seq = (size_t)K * H * N;
    WfRetgradReduceArgs ra{};
    ra.sl = sl; ra.N = N; ra.K = K; ra.H = H;
    ra.ws = h->d_ws; ra.wind_stride = wind_stride;
    ra.ws_prev = (!ahead && h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed; series-ahead: the current speed
    ra.ews = b.d_wind;
    ra.load_coef = h->env.load_coef; ra.gamma = gamma;
    ra.power_ev = b.d_pow; ra.load_ev = b.d_load;
    ra.div = r->d_div; ra.flags = r->d_flags;
    ra.terminal = d_term ? d_term + fk * N : nullptr;
    ra.returns_ev = r->d_ret;
    ra.returns = d_ret ? d_ret + fk : nullptr;
    ra.rewards = d_rew ? d_rew + fk * H : nullptr;
    ra.farm_power = d_fp ? d_fp + fk * H : nullptr;
    ra.action_gradient = d_ag ? d_ag + first * seq : nullptr;
    ra.reward_gradient = d_rg ? d_rg + first * seq : nullptr;
    ra.state_gradient = d_sg ? d_sg + fk * N : nullptr;
    WFX_HIP(r, wfk_launch_retgrad_reduce(&ra, h->stream));
    if (d_best) {
      WfRetgradBestArgs ba{};
      ba.n_slots = sl.n_slots; ba.K = K; ba.returns_ev = r->d_ret; ba.best = d_best + first;
      WFX_HIP(r, wfk_launch_retgrad_best(&ba, h->stream));
    }
    return WF_OK;
  };
  return run_rows(r, b, r->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce (+ best) e3, then the next chunk's e0
int wf_retgrad_last_timing(wf_retgrad* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  return last_timing(r, "wf_retgrad_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_retgrad_evaluator(wf_retgrad* r) { return r ? r->eval.ev : nullptr; }

int wf_retgrad_kernel_info(wf_retgrad* r, int* info) {
  if (!r || !info) return ext_fail(r, WF_E_INVALID, "wf_retgrad_kernel_info: NULL argument");
  return kernel_info(r, WF_RETGRAD_KERNELS, wfk_retgrad_func_attributes, info);
}

const char* wf_retgrad_last_error(wf_retgrad* r) { return r ? r->err.c_str() : "wf_retgrad: NULL object"; }

}  // extern "C"
