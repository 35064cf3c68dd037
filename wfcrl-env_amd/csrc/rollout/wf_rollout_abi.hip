// wf_rollout_abi.hip — the C boundary of the rollout extension (include/wfrollout.h): an object that is created on a rose
// object (whose device tables it reads) and on that object's parent handle, owns an evaluator handle and its device buffers,
// and enqueues a whole rollout run on the parent's stream.  The run is the extensions' shared row driver's (ext/wf_ext.h:
// run_rows — checks, chunks of K H rows per farm, the evaluator and its step for power and load, events); this file supplies
// its own checks, the upload of the controllers, a chunk's lay-out and reduce launches (wf_rollout_kernels.hip) and names the
// caller's arrays to stage.  Reads the parent (layout, model, wind, env parameters and env state, kernel choice, resolve
// mode) and the rose object's tables; stores nothing in either — in particular the speed a wf_env_set_prev_wind left for the
// next env step stays for that step.
#include <cmath>

#include "../../../include/wfrollout.h"
#include "../ext/wf_ext.h"
#include "../../../include/wfwindgen.h"
#include "../series/wf_series.h"
#include "wf_rollout.h"

using namespace wfi;

struct wf_rollout : ext_base {
  const wf_rose* tables = nullptr;  // the rose object: read, never written; it outlives this object
  // configuration
  int strict = 0, max_eval = 65536;
  int series_ahead = 0;  // wf_rollout_set_series: the rows' wind is the window of the series' coming rows
  const wf_windgen* wind_source = nullptr;  // wf_rollout_set_wind_source (include/wfwindgen.h): that series is a generator's, not the parent's
  // the controllers the device holds: [K] slot, lead (ints), alpha (doubles), deadband (floats), and the host copy the upload reads
  std::vector<int> c_int;
  std::vector<double> c_alpha;
  std::vector<float> c_band;
  dev_buf<int> d_cint;      // [2][K] slot, lead
  dev_buf<double> d_calpha; // [K]
  dev_buf<float> d_cband;   // [K]
  // device buffers (grow-only)
  row_batch rows;                // E = C K H farms, with loads
  dev_buf<WfRolloutBracket> d_brk;  // [E] the lay-out kernel's brackets
  dev_buf<double> d_window;      // [n_farms][H][2] the series window, laid out like a caller's wind
  dev_buf<char> d_stage;         // staging for host callers: wind, filter0; the eight outputs
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the controllers start at the fused env's state)";

}  // namespace

extern "C" {

int wf_rollout_create(wf_handle* h, wf_rose* tables, wf_rollout** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  if (!tables) return fail(h, WF_E_INVALID, "wf_rollout_create: the rose object (the controllers' tables) is NULL");
  if (rose_parent(tables) != h) return fail(h, WF_E_INVALID, "wf_rollout_create: the rose object belongs to another handle");
  const int rc = ext_create(h, out);
  if (rc == WF_OK) (*out)->tables = tables;
  return rc;
}

int wf_rollout_destroy(wf_rollout* r) { return ext_destroy(r); }

int wf_rollout_config(wf_rollout* r, int strict, int max_eval_farms) {
  if (!r) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  r->strict = strict != 0; r->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_rollout_set_timing(wf_rollout* r, int detail) {
  if (!r) return WF_E_INVALID;
  r->detail = detail != 0;
  return WF_OK;
}

int wf_rollout_set_series(wf_rollout* r, int ahead) {
  if (!r) return WF_E_INVALID;
  r->series_ahead = ahead != 0;
  return WF_OK;
}

int wf_rollout_set_wind_source(wf_rollout* r, wf_windgen* g) {
  if (!r) return WF_E_INVALID;
  r->wind_source = g;
  return WF_OK;
}

int wf_rollout_run(wf_rollout* r, int K, const int* slot, const double* alpha, const float* deadband, const int* lead, int H,
                   const double* wind, const double* filter0, double gamma, int n_farms, const int* farms, double* returns,
                   double* rewards, double* farm_power, float* actions, float* final_yaw, int* gated, double* filter_final,
                   int* best, int on_device) {
  if (!r) return WF_E_INVALID;
  wf_handle* h = r->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool ahead = r->series_ahead != 0;
  row_batch& b = r->rows;
  const double *d_wind = nullptr, *d_f0 = nullptr;
  double *d_ret = nullptr, *d_rew = nullptr, *d_fp = nullptr, *d_ff = nullptr;
  float *d_act = nullptr, *d_fy = nullptr;
  int *d_gated = nullptr, *d_best = nullptr;
  staging st(r, r->d_stage, on_device);
  const WfEnvView env = env_view(h);
  row_policy k;
  k.what = "controller rollouts serve"; k.name = "wf_rollout_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = r->strict; k.max_eval = r->max_eval;
  k.check = [&]() -> int {
    if (K < 1 || K > WF_ROLLOUT_MAX_K) return ext_fail(r, WF_E_INVALID, "the number of controllers K must be in 1..64");
    if (H < 1 || H > WF_ROLLOUT_MAX_H) return ext_fail(r, WF_E_INVALID, "the horizon H must be in 1..1024");
    if (K > WF_ROLLOUT_MAX_ROWS / H) return ext_fail(r, WF_E_INVALID, "the rows of a farm are limited: K H <= 4096");
    if (!slot || !alpha || !deadband || !lead) return ext_fail(r, WF_E_INVALID, "wf_rollout_run: a controller array is NULL");
    for (int c = 0; c < K; ++c) {
      if (slot[c] < 0 || slot[c] >= WF_ROSE_SLOTS) return ext_fail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
      int tn = 0;
      if (!rose_device_table(r->tables, slot[c], &tn).T) return ext_fail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
      if (tn != N) return ext_fail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
      if (!(alpha[c] > 0.0) || !(alpha[c] <= 1.0)) return ext_fail(r, WF_E_INVALID, "a controller's alpha must be in (0, 1]");
      if (!std::isfinite(deadband[c]) || deadband[c] < 0.0f) return ext_fail(r, WF_E_INVALID, "a controller's deadband must be finite and >= 0");
      if (lead[c] < 0 || lead[c] > WF_ROLLOUT_MAX_LEAD) return ext_fail(r, WF_E_INVALID, "a controller's lead must be in 0..16");
    }
    if (!std::isfinite(gamma) || gamma < 0.0 || gamma > 1.0) return ext_fail(r, WF_E_INVALID, "gamma must be finite and in [0, 1]");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(r, WF_E_INVALID, kNoEnv);
    if (ahead) {
      const int rc = series_ahead_check(r, r->wind_source, wind != nullptr, H);
      if (rc != WF_OK) return rc;
    }
    k.rows = K * H;
    return WF_OK;
  };
  k.reserve = [&](int, int E) -> int {
    const size_t fk = (size_t)n_farms * K, fr = fk * H;
    int rc = reserve(r, r->d_brk, (size_t)E);
    if (rc == WF_OK) rc = reserve(r, r->d_cint, 2 * (size_t)WF_ROLLOUT_MAX_K);
    if (rc == WF_OK) rc = reserve(r, r->d_calpha, (size_t)WF_ROLLOUT_MAX_K);
    if (rc == WF_OK) rc = reserve(r, r->d_cband, (size_t)WF_ROLLOUT_MAX_K);
    if (rc != WF_OK) return rc;
    // the controllers: uploaded when they differ from what the device holds
    std::vector<int> ci(2 * (size_t)K);
    for (int c = 0; c < K; ++c) { ci[c] = slot[c]; ci[K + c] = lead[c]; }
    const std::vector<double> ca(alpha, alpha + K);
    const std::vector<float> cb(deadband, deadband + K);
    if (ci != r->c_int || ca != r->c_alpha || cb != r->c_band) {
      WFX_HIP(r, hipStreamSynchronize(h->stream));  // (a previous upload may still read the host copies)
      r->c_int = ci; r->c_alpha = ca; r->c_band = cb;
      WFX_HIP(r, hipMemcpyAsync(r->d_cint, r->c_int.data(), sizeof(int) * 2 * K, hipMemcpyHostToDevice, h->stream));
      WFX_HIP(r, hipMemcpyAsync(r->d_calpha, r->c_alpha.data(), sizeof(double) * K, hipMemcpyHostToDevice, h->stream));
      WFX_HIP(r, hipMemcpyAsync(r->d_cband, r->c_band.data(), sizeof(float) * K, hipMemcpyHostToDevice, h->stream));
    }
    st.in(wind, (size_t)n_farms * H * 2, &d_wind); st.in(filter0, fk * 2, &d_f0);
    if (ahead) {  // (the farm list is on the device by now: run_rows uploads it before this hook)
      rc = series_ahead_window(r, r->wind_source, r->d_window, H, n_farms, farms ? b.farms.d.p : nullptr);
      if (rc != WF_OK) return rc;
      d_wind = r->d_window;
    }
    st.out(returns, fk, &d_ret); st.out(rewards, fr, &d_rew); st.out(farm_power, fr, &d_fp);
    st.out(actions, fr * N, &d_act); st.out(final_yaw, fk * N, &d_fy); st.out(gated, fk, &d_gated);
    st.out(filter_final, fk * 2, &d_ff); st.out(best, (size_t)n_farms, &d_best);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t first = (size_t)sl.base;
    WfRolloutLayoutArgs la{};
    la.sl = sl;
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N; la.K = K; la.H = H;
    la.env = env;
    for (int i = 0; i < WF_ROSE_SLOTS; ++i) la.tab[i] = rose_device_table(r->tables, i, nullptr);
    la.c_slot = r->d_cint; la.c_lead = r->d_cint + K; la.c_alpha = r->d_calpha; la.c_deadband = r->d_cband;
    la.wind = d_wind ? d_wind + first * H * 2 : nullptr;
    la.filter0 = d_f0 ? d_f0 + first * K * 2 : nullptr;
    la.brk = r->d_brk;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    la.actions = d_act ? d_act + first * k.rows * N : nullptr;
    la.final_yaw = d_fy ? d_fy + first * K * N : nullptr;
    la.gated = d_gated ? d_gated + first * K : nullptr;
    la.filter_final = d_ff ? d_ff + first * K * 2 : nullptr;
    WFX_HIP(r, wfk_launch_rollout_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base;
    WfRolloutReduceArgs ra{};
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
    WFX_HIP(r, wfk_launch_rollout_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(r, b, r->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_rollout_last_timing(wf_rollout* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  return last_timing(r, "wf_rollout_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_rollout_evaluator(wf_rollout* r) { return r ? r->eval.ev : nullptr; }

int wf_rollout_kernel_info(wf_rollout* r, int* info) {
  if (!r || !info) return ext_fail(r, WF_E_INVALID, "wf_rollout_kernel_info: NULL argument");
  return kernel_info(r, WF_ROLLOUT_KERNELS, wfk_rollout_func_attributes, info);
}

const char* wf_rollout_last_error(wf_rollout* r) { return r ? r->err.c_str() : "wf_rollout: NULL object"; }

}  // extern "C"
