// wf_scenario_abi.hip — the C boundary of the scenario extension (include/wfscenario.h): an object that belongs to a parent
// handle, owns an evaluator handle and its device buffers, and enqueues a whole scenario run on the parent's stream.  The run
// is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of K M H rows per farm, the evaluator and
// its step for power and load, events); this file supplies its own checks, a chunk's lay-out and reduce launches
// (wf_scenario_kernels.hip) and names the caller's arrays to stage.  Reads the parent (layout, model, wind, env parameters
// and env state, kernel choice, resolve mode); stores nothing in it — in particular the speed a wf_env_set_prev_wind left
// for the next env step stays for that step, and is not read here.
#include <cmath>
#include <vector>

#include "../../../include/wfscenario.h"
#include "../ensemble/wf_ensemble_host.h"
#include "../ext/wf_ext.h"
#include "wf_scenario.h"

using namespace wfi;

static_assert(WF_SCENARIO_MAX_ROWS == WF_LOOKAHEAD_MAX_ROWS, "the reduce kernel's LDS is sized for the look-ahead's row limit");

struct wf_scenario : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  row_batch rows;         // E = C K M H farms, with loads
  dev_buf<char> d_stage;  // staging for host callers: actions, anchor; the eight outputs
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K M H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the sequences start at the fused env's state)";

}  // namespace

extern "C" {

int wf_scenario_create(wf_handle* h, wf_scenario** out) { return ext_create(h, out); }

int wf_scenario_destroy(wf_scenario* s) { return ext_destroy(s); }

int wf_scenario_config(wf_scenario* s, int strict, int max_eval_farms) {
  if (!s) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  s->strict = strict != 0; s->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_scenario_set_timing(wf_scenario* s, int detail) {
  if (!s) return WF_E_INVALID;
  s->detail = detail != 0;
  return WF_OK;
}

int wf_scenario_run(wf_scenario* s, const float* actions, int K, int H, int M, const wf_wind_process* process, double ws_lo,
                    double ws_hi, unsigned long long seed, double gamma, int tail, double risk_weight, const double* anchor,
                    int n_farms, const int* farms, double* expected_returns, double* cvar, double* score, double* member_returns,
                    double* rewards, double* wind_paths, float* final_yaw, int* best, int on_device) {
  if (!s) return WF_E_INVALID;
  wf_handle* h = s->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  row_batch& b = s->rows;
  const float* d_act = nullptr;
  const double* d_anchor = nullptr;
  double *d_exp = nullptr, *d_cvar = nullptr, *d_score = nullptr, *d_mret = nullptr, *d_rew = nullptr, *d_paths = nullptr;
  float* d_fy = nullptr;
  int* d_best = nullptr;
  staging st(s, s->d_stage, on_device);
  const WfEnvView env = env_view(h);
  row_policy k;
  k.what = "scenario returns serve"; k.name = "wf_scenario_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = s->strict; k.max_eval = s->max_eval;
  k.check = [&]() -> int {
    if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(s, WF_E_INVALID, "the horizon H must be in 1..64");
    if (M < 1 || M > WF_SCENARIO_MAX_MEMBERS) return ext_fail(s, WF_E_INVALID, "the number of members M must be in 1..64");
    if (K < 1 || K > WF_SCENARIO_MAX_ROWS / (M * H))
      return ext_fail(s, WF_E_INVALID, "the number of sequences K must be >= 1 with K M H <= 4096");
    int rc = check_ensemble(s, "wf_scenario_run", M, tail, risk_weight, gamma, process, ws_lo, ws_hi);
    if (rc != WF_OK) return rc;
    if (!actions) return ext_fail(s, WF_E_INVALID, "wf_scenario_run: actions is NULL");
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(s, WF_E_INVALID, kNoEnv);
    rc = check_ensemble_anchor(s, anchor, n_farms, on_device);
    if (rc != WF_OK) return rc;
    k.rows = K * M * H;
    return WF_OK;
  };
  k.reserve = [&](int, int) -> int {
    const size_t fk = (size_t)n_farms * K, fm = (size_t)n_farms * M * H;
    st.in(actions, fk * H * N, &d_act); st.in(anchor, (size_t)n_farms * 2, &d_anchor);
    st.out(expected_returns, fk, &d_exp); st.out(cvar, fk, &d_cvar); st.out(score, fk, &d_score);
    st.out(member_returns, fk * M, &d_mret); st.out(rewards, fk * M * H, &d_rew); st.out(wind_paths, fm * 2, &d_paths);
    st.out(final_yaw, fk * N, &d_fy); st.out(best, (size_t)n_farms, &d_best);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t first = (size_t)sl.base;
    WfScenarioLayoutArgs la{};
    la.sl = sl;
    la.ens = ensemble_args(h, M, H, *process, ws_lo, ws_hi, seed, d_anchor, first);
    la.N = N; la.K = K;
    la.env = env;
    la.actions = d_act + first * K * H * N;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    la.wind_paths = d_paths ? d_paths + first * M * H * 2 : nullptr;
    la.final_yaw = d_fy ? d_fy + first * K * N : nullptr;
    WFX_HIP(s, wfk_launch_scenario_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base;
    WfScenarioReduceArgs ra{};
    ra.sl = sl; ra.N = N; ra.K = K; ra.M = M; ra.H = H;
    ra.ws = h->d_ws; ra.wind_stride = wind_stride;
    ra.ews = b.d_wind;
    ra.load_coef = h->env.load_coef; ra.gamma = gamma; ra.lam = risk_weight; ra.q = tail;
    ra.power_ev = b.d_pow; ra.load_ev = b.d_load;
    ra.expected = d_exp ? d_exp + first * K : nullptr;
    ra.cvar = d_cvar ? d_cvar + first * K : nullptr;
    ra.score = d_score ? d_score + first * K : nullptr;
    ra.member_returns = d_mret ? d_mret + first * K * M : nullptr;
    ra.rewards = d_rew ? d_rew + first * k.rows : nullptr;
    ra.best = d_best ? d_best + first : nullptr;
    WFX_HIP(s, wfk_launch_scenario_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(s, b, s->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_scenario_last_timing(wf_scenario* s, float* total_ms, float* step_ms, float* glue_ms) {
  if (!s) return WF_E_INVALID;
  return last_timing(s, "wf_scenario_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_scenario_evaluator(wf_scenario* s) { return s ? s->eval.ev : nullptr; }

int wf_scenario_kernel_info(wf_scenario* s, int* info) {
  if (!s || !info) return ext_fail(s, WF_E_INVALID, "wf_scenario_kernel_info: NULL argument");
  return kernel_info(s, WF_SCENARIO_KERNELS, wfk_scenario_func_attributes, info);
}

const char* wf_scenario_last_error(wf_scenario* s) { return s ? s->err.c_str() : "wf_scenario: NULL object"; }

}  // extern "C"
