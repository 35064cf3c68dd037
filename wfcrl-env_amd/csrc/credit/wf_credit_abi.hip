// wf_credit_abi.hip — the C boundary of the credit extension (include/wfcredit.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole counterfactual run on the parent's stream.  The run
// is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of 1 + N K rows per farm, the evaluator
// and its step for power and load, events); this file supplies its own checks, a chunk's lay-out and reduce launches
// (wf_credit_kernels.hip) and names the caller's arrays to stage.  Reads the parent (layout, model, wind, env parameters and
// env state, kernel choice, resolve mode); stores nothing in it — in particular the speed a wf_env_set_prev_wind left for
// the next env step stays for that step.
#include "../../../include/wfcredit.h"
#include "../ext/wf_ext.h"
#include "../../../include/wfwindgen.h"
#include "../series/wf_series.h"
#include "wf_credit.h"

using namespace wfi;

struct wf_credit : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  int series_ahead = 0;   // wf_credit_set_series (include/wfseries.h): the rows' wind is the series' coming row
  const wf_windgen* wind_source = nullptr;  // wf_credit_set_wind_source (include/wfwindgen.h): that series is a generator's, not the parent's
  // device buffers (grow-only)
  row_batch rows;         // E = C (1 + N K) farms, with loads
  dev_buf<double> d_window;  // [n_farms][2] that row of every listed farm
  dev_buf<char> d_stage;  // staging for host callers: base and alt rows; reward, farm_power, difference
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least 1 + N K";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (an action, or base == NULL, is taken at the fused env's state)";

bool is_kind(int k) { return k == WF_CREDIT_YAW || k == WF_CREDIT_ACTION; }

}  // namespace

extern "C" {

int wf_credit_create(wf_handle* h, wf_credit** out) { return ext_create(h, out); }

int wf_credit_destroy(wf_credit* c) { return ext_destroy(c); }

int wf_credit_config(wf_credit* c, int strict, int max_eval_farms) {
  if (!c) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (c->h->N > 0 && max_eval_farms < c->h->N + 1) return ext_fail(c, WF_E_INVALID, kRowsMsg);
  c->strict = strict != 0; c->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_credit_set_timing(wf_credit* c, int detail) {
  if (!c) return WF_E_INVALID;
  c->detail = detail != 0;
  return WF_OK;
}

int wf_credit_set_series(wf_credit* c, int ahead) {
  if (!c) return WF_E_INVALID;
  c->series_ahead = ahead != 0;
  return WF_OK;
}

int wf_credit_set_wind_source(wf_credit* c, wf_windgen* g) {
  if (!c) return WF_E_INVALID;
  c->wind_source = g;
  return WF_OK;
}

int wf_credit_run(wf_credit* c, int base_kind, const float* base, int alt_kind, const float* alt, int K, int n_farms,
                  const int* farms, double* reward, double* farm_power, double* difference, int on_device) {
  if (!c) return WF_E_INVALID;
  wf_handle* h = c->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool ahead = c->series_ahead != 0;
  row_batch& b = c->rows;
  const float *d_base = nullptr, *d_alt = nullptr;
  double *d_rew = nullptr, *d_fp = nullptr, *d_dif = nullptr;
  staging st(c, c->d_stage, on_device);
  const WfCreditEnv env = env_view(h);
  row_policy k;
  k.what = "counterfactual rewards serve"; k.name = "wf_credit_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = c->strict; k.max_eval = c->max_eval;
  k.check = [&]() -> int {
    if (K < 1 || K > WF_CREDIT_MAX_ALT) return ext_fail(c, WF_E_INVALID, "the number of alternatives K must be in 1..8");
    if (!is_kind(base_kind) || !is_kind(alt_kind)) return ext_fail(c, WF_E_INVALID, "base_kind and alt_kind are WF_CREDIT_YAW (0) or WF_CREDIT_ACTION (1)");
    if (!alt && K != 1) return ext_fail(c, WF_E_INVALID, "alt == NULL (hold / zero yaw) is one alternative: K must be 1");
    const bool needs_env = !base || base_kind == WF_CREDIT_ACTION || alt_kind == WF_CREDIT_ACTION;
    if (needs_env && !h->d_env_yaw) return ext_fail(c, WF_E_INVALID, kNoEnv);
    if (ahead) {
      const int rc = series_ahead_check(c, c->wind_source, false, 1);
      if (rc != WF_OK) return rc;
    }
    k.rows = 1 + N * K;
    return WF_OK;
  };
  k.reserve = [&](int, int) -> int {
    const size_t fn = (size_t)n_farms * N, fr = (size_t)n_farms * k.rows;
    st.in(base, fn, &d_base); st.in(alt, fn * K, &d_alt);
    st.out(reward, fr, &d_rew); st.out(farm_power, fr, &d_fp); st.out(difference, fn * K, &d_dif);
    if (ahead)  // (the farm list is on the device by now: run_rows uploads it before this hook)
      return series_ahead_window(c, c->wind_source, c->d_window, 1, n_farms, farms ? b.farms.d.p : nullptr);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t off = (size_t)sl.base * N;
    WfCreditLayoutArgs la{};
    la.sl = sl;
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N; la.K = K;
    la.env = env; la.base_kind = base_kind; la.alt_kind = alt_kind;
    la.base = d_base ? d_base + off : nullptr;
    la.alt = d_alt ? d_alt + off * K : nullptr;
    la.wind = ahead ? c->d_window + (size_t)sl.base * 2 : nullptr;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    WFX_HIP(c, wfk_launch_credit_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base;
    WfCreditReduceArgs ra{};
    ra.sl = sl; ra.N = N; ra.K = K;
    ra.ws = h->d_ws; ra.wind_stride = wind_stride;
    ra.ws_prev = (!ahead && h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed; series-ahead: the current speed
    ra.load_coef = h->env.load_coef;
    ra.yaw_ev = b.d_yaw; ra.power_ev = b.d_pow; ra.load_ev = b.d_load;
    ra.reward = d_rew ? d_rew + first * k.rows : nullptr;
    ra.farm_power = d_fp ? d_fp + first * k.rows : nullptr;
    ra.difference = d_dif ? d_dif + first * N * K : nullptr;
    WFX_HIP(c, wfk_launch_credit_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(c, b, c->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_credit_last_timing(wf_credit* c, float* total_ms, float* step_ms, float* glue_ms) {
  if (!c) return WF_E_INVALID;
  return last_timing(c, "wf_credit_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_credit_evaluator(wf_credit* c) { return c ? c->eval.ev : nullptr; }

int wf_credit_kernel_info(wf_credit* c, int* info) {
  if (!c || !info) return ext_fail(c, WF_E_INVALID, "wf_credit_kernel_info: NULL argument");
  return kernel_info(c, WF_CREDIT_KERNELS, wfk_credit_func_attributes, info);
}

const char* wf_credit_last_error(wf_credit* c) { return c ? c->err.c_str() : "wf_credit: NULL object"; }

}  // extern "C"
