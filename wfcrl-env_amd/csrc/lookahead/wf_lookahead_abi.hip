// wf_lookahead_abi.hip — the C boundary of the lookahead extension (include/wflookahead.h): an object that belongs to a
// parent handle, owns an evaluator handle and its device buffers, and enqueues a whole look-ahead run on the parent's stream.
// The run is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K H rows per farm, the evaluator
// and its step for power and load, events); this file supplies its own checks, a chunk's lay-out and reduce launches
// (wf_lookahead_kernels.hip) and names the caller's arrays to stage.  Reads the parent (layout, model, wind, env parameters
// and env state, kernel choice, resolve mode); stores nothing in it — in particular the speed a wf_env_set_prev_wind left
// for the next env step stays for that step.
#include <cmath>

#include "../../../include/wflookahead.h"
#include "../ext/wf_ext.h"
#include "../../../include/wfwindgen.h"
#include "../series/wf_series.h"
#include "wf_lookahead.h"

using namespace wfi;

struct wf_lookahead : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  int series_ahead = 0;   // wf_lookahead_set_series (include/wfseries.h): the rows' wind is the window of the series' coming rows
  const wf_windgen* wind_source = nullptr;  // wf_lookahead_set_wind_source (include/wfwindgen.h): that series is a generator's, not the parent's
  // device buffers (grow-only)
  row_batch rows;         // E = C K H farms, with loads
  dev_buf<double> d_window;  // [n_farms][H][2] that window, laid out like a caller's wind
  dev_buf<char> d_stage;  // staging for host callers: actions, wind; returns, rewards, farm_power, final_yaw, best
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the sequences start at the fused env's state)";

}  // namespace

extern "C" {

int wf_lookahead_create(wf_handle* h, wf_lookahead** out) { return ext_create(h, out); }

int wf_lookahead_destroy(wf_lookahead* l) { return ext_destroy(l); }

int wf_lookahead_config(wf_lookahead* l, int strict, int max_eval_farms) {
  if (!l) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  l->strict = strict != 0; l->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_lookahead_set_timing(wf_lookahead* l, int detail) {
  if (!l) return WF_E_INVALID;
  l->detail = detail != 0;
  return WF_OK;
}

int wf_lookahead_set_series(wf_lookahead* l, int ahead) {
  if (!l) return WF_E_INVALID;
  l->series_ahead = ahead != 0;
  return WF_OK;
}

int wf_lookahead_set_wind_source(wf_lookahead* l, wf_windgen* g) {
  if (!l) return WF_E_INVALID;
  l->wind_source = g;
  return WF_OK;
}

int wf_lookahead_run(wf_lookahead* l, const float* actions, int K, int H, const double* wind, double gamma, int n_farms,
                     const int* farms, double* returns, double* rewards, double* farm_power, float* final_yaw, int* best,
                     int on_device) {
  if (!l) return WF_E_INVALID;
  wf_handle* h = l->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool ahead = l->series_ahead != 0;
  row_batch& b = l->rows;
  const float* d_act = nullptr;
  const double* d_wind = nullptr;
  double *d_ret = nullptr, *d_rew = nullptr, *d_fp = nullptr;
  float* d_fy = nullptr;
  int* d_best = nullptr;
  staging st(l, l->d_stage, on_device);
  const WfEnvView env = env_view(h);
  row_policy k;
  k.what = "look-ahead returns serve"; k.name = "wf_lookahead_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = l->strict; k.max_eval = l->max_eval;
  k.check = [&]() -> int {
    if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(l, WF_E_INVALID, "the horizon H must be in 1..64");
    if (K < 1 || K > WF_LOOKAHEAD_MAX_ROWS / H) return ext_fail(l, WF_E_INVALID, "the number of sequences K must be >= 1 with K H <= 4096");
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return ext_fail(l, WF_E_INVALID, "gamma must be finite and in [0, 1]");
    if (!actions) return ext_fail(l, WF_E_INVALID, "wf_lookahead_run: actions is NULL");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(l, WF_E_INVALID, kNoEnv);
    if (ahead) {
      const int rc = series_ahead_check(l, l->wind_source, wind != nullptr, H);
      if (rc != WF_OK) return rc;
    }
    k.rows = K * H;
    return WF_OK;
  };
  k.reserve = [&](int, int) -> int {
    const size_t fk = (size_t)n_farms * K, fr = fk * H;
    st.in(actions, fr * N, &d_act); st.in(wind, (size_t)n_farms * H * 2, &d_wind);
    if (ahead) {  // (the farm list is on the device by now: run_rows uploads it before this hook)
      const int rc = series_ahead_window(l, l->wind_source, l->d_window, H, n_farms, farms ? b.farms.d.p : nullptr);
      if (rc != WF_OK) return rc;
      d_wind = l->d_window;
    }
    st.out(returns, fk, &d_ret); st.out(rewards, fr, &d_rew); st.out(farm_power, fr, &d_fp);
    st.out(final_yaw, fk * N, &d_fy); st.out(best, (size_t)n_farms, &d_best);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t first = (size_t)sl.base;
    WfLookaheadLayoutArgs la{};
    la.sl = sl;
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N; la.K = K; la.H = H;
    la.env = env;
    la.actions = d_act + first * k.rows * N;
    la.wind = d_wind ? d_wind + first * H * 2 : nullptr;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    la.final_yaw = d_fy ? d_fy + first * K * N : nullptr;
    WFX_HIP(l, wfk_launch_lookahead_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base;
    WfLookaheadReduceArgs ra{};
    ra.sl = sl; ra.N = N; ra.K = K; ra.H = H;
    ra.ws = h->d_ws; ra.wind_stride = wind_stride;
    ra.ws_prev = (!ahead && h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed; series-ahead: the current speed
    ra.ews = b.d_wind;
    ra.load_coef = h->env.load_coef; ra.gamma = gamma;
    ra.power_ev = b.d_pow; ra.load_ev = b.d_load;
    ra.returns = d_ret ? d_ret + first * K : nullptr;
    ra.rewards = d_rew ? d_rew + first * k.rows : nullptr;
    ra.farm_power = d_fp ? d_fp + first * k.rows : nullptr;
    ra.best = d_best ? d_best + first : nullptr;
    WFX_HIP(l, wfk_launch_lookahead_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(l, b, l->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_lookahead_last_timing(wf_lookahead* l, float* total_ms, float* step_ms, float* glue_ms) {
  if (!l) return WF_E_INVALID;
  return last_timing(l, "wf_lookahead_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_lookahead_evaluator(wf_lookahead* l) { return l ? l->eval.ev : nullptr; }

int wf_lookahead_kernel_info(wf_lookahead* l, int* info) {
  if (!l || !info) return ext_fail(l, WF_E_INVALID, "wf_lookahead_kernel_info: NULL argument");
  return kernel_info(l, WF_LOOKAHEAD_KERNELS, wfk_lookahead_func_attributes, info);
}

const char* wf_lookahead_last_error(wf_lookahead* l) { return l ? l->err.c_str() : "wf_lookahead: NULL object"; }

}  // extern "C"
