// wf_rollscen_abi.hip — the C boundary of the scenario-rollout extension (include/wfrollscen.h): an object that is created on a
// rose object (whose device tables it reads) and on that object's parent handle, owns an evaluator handle and its device
// buffers, and enqueues a whole run on the parent's stream.  The run is the extensions' shared row driver's (ext/wf_ext.h:
// run_rows — checks, chunks of K M H rows per farm, the evaluator and its step for power and load, events); this file supplies
// its own checks — the union of the rollout's and the scenario extension's —, the upload of the controllers, a chunk's lay-out
// and reduce launches (wf_rollscen_kernels.hip) and names the caller's arrays to stage.  Reads the parent (layout, model,
// wind, env parameters and env state, kernel choice, resolve mode) and the rose object's tables; stores nothing in either — in
// particular the speed a wf_env_set_prev_wind left for the next env step stays for that step, and is not read here.
#include <cmath>
#include <vector>

#include "../../../include/wfrollscen.h"
#include "../ensemble/wf_ensemble_host.h"
#include "../ext/wf_ext.h"
#include "wf_rollscen.h"

using namespace wfi;

static_assert(WF_ROLLSCEN_MAX_ROWS == WF_SCENARIO_MAX_ROWS && WF_ROLLSCEN_MAX_ROWS == WF_LOOKAHEAD_MAX_ROWS,
              "the reduce kernel's LDS is sized for the scenario extension's row limit");
static_assert(WF_ROLLSCEN_MAX_K == WF_ROLLOUT_MAX_K, "the controllers are the rollout extension's");
static_assert(staging::kMaxSegs >= 13, "a run names two inputs and eleven outputs");

struct wf_rollscen : ext_base {
  const wf_rose* tables = nullptr;  // the rose object: read, never written; it outlives this object
  // configuration
  int strict = 0, max_eval = 65536;
  // the controllers the device holds: [K] slot, lead (ints), alpha (doubles), deadband (floats), and the host copy the upload reads
  std::vector<int> c_int;
  std::vector<double> c_alpha;
  std::vector<float> c_band;
  dev_buf<int> d_cint;      // [2][K] slot, lead
  dev_buf<double> d_calpha; // [K]
  dev_buf<float> d_cband;   // [K]
  // device buffers (grow-only)
  row_batch rows;                    // E = C K M H farms, with loads
  dev_buf<WfRollscenBracket> d_brk;  // [E] the lay-out kernel's brackets, where a farm's do not stay in LDS
  dev_buf<char> d_stage;             // staging for host callers: anchor, filter0; the eleven outputs
  evaluator eval;
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least K M H";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (the controllers start at the fused env's state)";

}  // namespace

extern "C" {

int wf_rollscen_create(wf_handle* h, wf_rose* tables, wf_rollscen** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  if (!tables) return fail(h, WF_E_INVALID, "wf_rollscen_create: the rose object (the controllers' tables) is NULL");
  if (rose_parent(tables) != h) return fail(h, WF_E_INVALID, "wf_rollscen_create: the rose object belongs to another handle");
  const int rc = ext_create(h, out);
  if (rc == WF_OK) (*out)->tables = tables;
  return rc;
}

int wf_rollscen_destroy(wf_rollscen* r) { return ext_destroy(r); }

int wf_rollscen_config(wf_rollscen* r, int strict, int max_eval_farms) {
  if (!r) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  r->strict = strict != 0; r->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_rollscen_set_timing(wf_rollscen* r, int detail) {
  if (!r) return WF_E_INVALID;
  r->detail = detail != 0;
  return WF_OK;
}

int wf_rollscen_run(wf_rollscen* r, int K, const int* slot, const double* alpha, const float* deadband, const int* lead, int H,
                    int M, const wf_wind_process* process, double ws_lo, double ws_hi, unsigned long long seed, double gamma,
                    int tail, double risk_weight, const double* anchor, const double* filter0, int n_farms, const int* farms,
                    double* expected_returns, double* cvar, double* score, double* member_returns, double* rewards,
                    double* wind_paths, float* actions, float* final_yaw, int* gated, float* first_action, int* best,
                    int on_device) {
  if (!r) return WF_E_INVALID;
  wf_handle* h = r->h;
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  row_batch& b = r->rows;
  const double *d_anchor = nullptr, *d_f0 = nullptr;
  double *d_exp = nullptr, *d_cvar = nullptr, *d_score = nullptr, *d_mret = nullptr, *d_rew = nullptr, *d_paths = nullptr;
  float *d_act = nullptr, *d_fy = nullptr, *d_first = nullptr;
  int *d_gated = nullptr, *d_best = nullptr;
  bool spill = false;
  staging st(r, r->d_stage, on_device);
  const WfEnvView env = env_view(h);
  row_policy k;
  k.what = "scenario rollouts serve"; k.name = "wf_rollscen_run";
  k.rows_msg = kRowsMsg; k.loads = true;
  k.strict = r->strict; k.max_eval = r->max_eval;
  k.check = [&]() -> int {
    if (K < 1 || K > WF_ROLLSCEN_MAX_K) return ext_fail(r, WF_E_INVALID, "the number of controllers K must be in 1..64");
    if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(r, WF_E_INVALID, "the horizon H must be in 1..64");
    if (M < 1 || M > WF_SCENARIO_MAX_MEMBERS) return ext_fail(r, WF_E_INVALID, "the number of members M must be in 1..64");
    if (K > WF_ROLLSCEN_MAX_ROWS / (M * H)) return ext_fail(r, WF_E_INVALID, "the rows of a farm are limited: K M H <= 4096");
    if (!slot || !alpha || !deadband || !lead) return ext_fail(r, WF_E_INVALID, "wf_rollscen_run: a controller array is NULL");
    for (int c = 0; c < K; ++c) {
      if (slot[c] < 0 || slot[c] >= WF_ROSE_SLOTS) return ext_fail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
      int tn = 0;
      if (!rose_device_table(r->tables, slot[c], &tn).T) return ext_fail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
      if (tn != N) return ext_fail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
      if (!(alpha[c] > 0.0) || !(alpha[c] <= 1.0)) return ext_fail(r, WF_E_INVALID, "a controller's alpha must be in (0, 1]");
      if (!std::isfinite(deadband[c]) || deadband[c] < 0.0f) return ext_fail(r, WF_E_INVALID, "a controller's deadband must be finite and >= 0");
      if (lead[c] < 0 || lead[c] > WF_ROLLOUT_MAX_LEAD) return ext_fail(r, WF_E_INVALID, "a controller's lead must be in 0..16");
    }
    int rc = check_ensemble(r, "wf_rollscen_run", M, tail, risk_weight, gamma, process, ws_lo, ws_hi);
    if (rc != WF_OK) return rc;
    if (!h->d_env_yaw || !h->d_env_acc || !h->d_env_moves) return ext_fail(r, WF_E_INVALID, kNoEnv);
    rc = check_ensemble_anchor(r, anchor, n_farms, on_device);
    if (rc != WF_OK) return rc;
    k.rows = K * M * H;
    spill = k.rows > WF_ROLLSCEN_LDS_RECORDS;
    return WF_OK;
  };
  k.reserve = [&](int, int E) -> int {
    const size_t fk = (size_t)n_farms * K, fkm = fk * M, fm = (size_t)n_farms * M * H;
    int rc = spill ? reserve(r, r->d_brk, (size_t)E) : WF_OK;
    if (rc == WF_OK) rc = reserve(r, r->d_cint, 2 * (size_t)WF_ROLLSCEN_MAX_K);
    if (rc == WF_OK) rc = reserve(r, r->d_calpha, (size_t)WF_ROLLSCEN_MAX_K);
    if (rc == WF_OK) rc = reserve(r, r->d_cband, (size_t)WF_ROLLSCEN_MAX_K);
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
    st.in(anchor, (size_t)n_farms * 2, &d_anchor); st.in(filter0, fk * 2, &d_f0);
    st.out(expected_returns, fk, &d_exp); st.out(cvar, fk, &d_cvar); st.out(score, fk, &d_score);
    st.out(member_returns, fkm, &d_mret); st.out(rewards, fkm * H, &d_rew); st.out(wind_paths, fm * 2, &d_paths);
    st.out(actions, fkm * H * N, &d_act); st.out(final_yaw, fkm * N, &d_fy); st.out(gated, fkm, &d_gated);
    st.out(first_action, fk * N, &d_first); st.out(best, (size_t)n_farms, &d_best);
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    const size_t first = (size_t)sl.base;
    WfRollscenLayoutArgs la{};
    la.sl = sl;
    la.ens = ensemble_args(h, M, H, *process, ws_lo, ws_hi, seed, d_anchor, first);
    la.N = N; la.K = K;
    la.env = env;
    for (int i = 0; i < WF_ROSE_SLOTS; ++i) la.tab[i] = rose_device_table(r->tables, i, nullptr);
    la.c_slot = r->d_cint; la.c_lead = r->d_cint + K; la.c_alpha = r->d_calpha; la.c_deadband = r->d_cband;
    la.filter0 = d_f0 ? d_f0 + first * K * 2 : nullptr;
    la.spill = spill ? 1 : 0;
    la.brk = spill ? r->d_brk.p : nullptr;
    la.yaw = b.d_yaw; la.ews = b.d_wind; la.ewd = b.d_wind + E;
    la.wind_paths = d_paths ? d_paths + first * M * H * 2 : nullptr;
    la.actions = d_act ? d_act + first * k.rows * N : nullptr;
    la.final_yaw = d_fy ? d_fy + first * K * M * N : nullptr;
    la.gated = d_gated ? d_gated + first * K * M : nullptr;
    la.first_action = d_first ? d_first + first * K * N : nullptr;
    WFX_HIP(r, wfk_launch_rollscen_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t first = (size_t)sl.base;
    WfRollscenReduceArgs ra{};
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
    WFX_HIP(r, wfk_launch_rollscen_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(r, b, r->eval, k, st, &n_farms, farms);
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_rollscen_last_timing(wf_rollscen* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  return last_timing(r, "wf_rollscen_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_rollscen_evaluator(wf_rollscen* r) { return r ? r->eval.ev : nullptr; }

int wf_rollscen_kernel_info(wf_rollscen* r, int* info) {
  if (!r || !info) return ext_fail(r, WF_E_INVALID, "wf_rollscen_kernel_info: NULL argument");
  return kernel_info(r, WF_ROLLSCEN_KERNELS, wfk_rollscen_func_attributes, info);
}

const char* wf_rollscen_last_error(wf_rollscen* r) { return r ? r->err.c_str() : "wf_rollscen: NULL object"; }

}  // extern "C"
