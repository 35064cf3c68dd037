// wf_robust_abi.hip — the C boundary of the robust extension (include/wfrobust.h): an object that belongs to a parent
// handle, owns a member set, two evaluator handles and their device buffers, and enqueues a whole expected-power evaluation or
// a whole robust coordinate search on the parent's stream.  Both runs are the extensions' shared drivers' (ext/wf_ext.h):
// the evaluation is a row run of M rows per farm (run_rows), the search a run_search — checks, chunks, the evaluators and
// their steps, the visit loop, staging and copy-back, events.  This file supplies the rows' wind and the launches
// (wf_robust_kernels.hip): a lay-out kernel per chunk, a row-sum kernel and an expectation or advance kernel after a step.
// Reads the parent (layout, model, wind, kernel choice, resolve mode); stores nothing in it.
#include "../../../include/wfrobust.h"
#include "../ext/wf_ext.h"
#include "wf_robust.h"

using namespace wfi;

static_assert(WF_ROBUST_MAX_PASSES == WF_SEARCH_MAX_PASSES && WF_ROBUST_MAX_K0 == WF_SEARCH_MAX_K0 && WF_ROBUST_MAX_K == WF_SEARCH_MAX_K &&
                  WF_ROBUST_ROWS_MAX == WF_SEARCH_ROWS_MAX, "the shared search driver (ext/wf_ext.h) is built for these limits");

struct wf_robust : ext_base {
  // the members: M == 0 = none yet; device copy [2][WF_ROBUST_MAX_MEMBERS] delta, normalised weight
  int M = 0, frame = WF_ROBUST_FIXED;
  double members[2 * WF_ROBUST_MAX_MEMBERS] = {};
  dev_buf<double> d_members;
  // configuration and the buffers of every search; wf_robust_evaluate runs its rows in them and stages through them too
  yaw_search s;
  dev_buf<double> d_rowsum;  // [E]
  // the evaluators: [0] wf_robust_evaluate (R = 1), [1] wf_robust_optimize
  evaluator eval[2];
};

namespace {

std::string no_members(const char* call) {
  return std::string("no members have been set: wf_robust_set_members must be called before ") + call;
}

WfRobustMembers device_members(const wf_robust* r) {
  return WfRobustMembers{r->d_members, r->d_members + WF_ROBUST_MAX_MEMBERS, r->M, r->frame};
}

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least (K_max + 1) x members";

}  // namespace

extern "C" {

int wf_robust_create(wf_handle* h, wf_robust** out) { return ext_create(h, out); }

int wf_robust_destroy(wf_robust* r) { return ext_destroy(r); }

int wf_robust_set_members(wf_robust* r, int M, const double* delta, const double* weight, int frame) {
  if (!r || !delta || !weight) return ext_fail(r, WF_E_INVALID, "wf_robust_set_members: NULL argument");
  if (M < 1 || M > WF_ROBUST_MAX_MEMBERS) return ext_fail(r, WF_E_INVALID, "the number of members must be in 1..33");
  if (frame != WF_ROBUST_RELATIVE && frame != WF_ROBUST_FIXED)
    return ext_fail(r, WF_E_INVALID, "frame must be WF_ROBUST_RELATIVE (0) or WF_ROBUST_FIXED (1)");
  double sum = 0.0;
  for (int m = 0; m < M; ++m) {
    if (!std::isfinite(delta[m]) || (m > 0 && !(delta[m] > delta[m - 1])))
      return ext_fail(r, WF_E_INVALID, "member offsets (delta) must be finite and strictly ascending");
    if (!std::isfinite(weight[m]) || !(weight[m] >= 0.0)) return ext_fail(r, WF_E_INVALID, "member weights must be finite and >= 0 (no negative weight)");
    sum += weight[m];
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) return ext_fail(r, WF_E_INVALID, "member weights must have a positive sum (they are all zero)");
  WFX_ON_DEVICE(r);
  hipStream_t st = r->h->stream;
  WFX_HIP(r, hipStreamSynchronize(st));  // (a previous upload may still read the host copy; running kernels read the device one)
  r->M = 0;
  if (!r->d_members.p) WFX_HIP(r, hipMalloc(&r->d_members.p, sizeof(r->members)));
  for (int m = 0; m < WF_ROBUST_MAX_MEMBERS; ++m) {
    r->members[m] = m < M ? delta[m] : 0.0;
    r->members[WF_ROBUST_MAX_MEMBERS + m] = m < M ? weight[m] / sum : 0.0;
  }
  WFX_HIP(r, hipMemcpyAsync(r->d_members, r->members, sizeof(r->members), hipMemcpyHostToDevice, st));
  WFX_HIP(r, hipStreamSynchronize(st));
  r->M = M; r->frame = frame;
  return WF_OK;
}

int wf_robust_config(wf_robust* r, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms) {
  if (!r || !K) return ext_fail(r, WF_E_INVALID, "wf_robust_config: NULL argument");
  return set_search_config(r, r->s.cfg, lo, hi, n_passes, K, strict, max_eval_farms, r->M > 0 ? r->M : 1, kRowsMsg);
}

int wf_robust_set_timing(wf_robust* r, int detail) {
  if (!r) return WF_E_INVALID;
  r->detail = detail != 0;
  return WF_OK;
}

int wf_robust_evaluate(wf_robust* r, const float* yaw, int n_farms, const int* farms, double* expected_power,
                       double* expected_turbine_power, float* member_power, int on_device) {
  if (!r) return WF_E_INVALID;
  wf_handle* h = r->h;
  yaw_search& s = r->s;
  const int N = h->N, M = r->M, wind_stride = h->wind_count == 1 ? 0 : 1;
  const float* d_yaw_in = nullptr;
  float* d_mem = nullptr;
  double *d_exp = nullptr, *d_turb = nullptr;
  staging st(r, s.d_stage, on_device);
  row_policy k;
  k.what = "expected power under uncertainty serves"; k.name = "wf_robust_evaluate";
  k.rows = M; k.no_rows = no_members("wf_robust_evaluate"); k.rows_msg = kRowsMsg;
  k.strict = s.cfg.strict; k.max_eval = s.cfg.max_eval; k.split_always = true;
  k.reserve = [&](int, int E) -> int {
    const size_t fn = (size_t)n_farms * N;
    st.in(yaw, fn, &d_yaw_in); st.out(expected_power, (size_t)n_farms, &d_exp);
    st.out(expected_turbine_power, fn, &d_turb); st.out(member_power, (size_t)n_farms * M, &d_mem);
    return reserve(r, r->d_rowsum, (size_t)E);
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = device_members(r); la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = 1; la.N = N;
    la.ews = s.d_wind; la.ewd = s.d_wind + E; la.write_yaw = 1;
    la.yaw_in = d_yaw_in ? d_yaw_in + (size_t)sl.base * N : nullptr; la.yaw = s.d_yaw;
    WFX_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int E) -> int {
    const size_t base = (size_t)sl.base;
    const WfRobustRowsumArgs sa{E, N, s.d_pow, r->d_rowsum};
    WFX_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
    WfRobustExpectArgs xa{};
    xa.sl = sl; xa.mb = device_members(r); xa.N = N; xa.power = s.d_pow; xa.rowsum = r->d_rowsum;
    xa.expected = d_exp ? d_exp + base : nullptr;
    xa.turbine = d_turb ? d_turb + base * N : nullptr;
    xa.member = d_mem ? d_mem + base * M : nullptr;
    WFX_HIP(r, wfk_launch_robust_expect(&xa, h->stream));
    return WF_OK;
  };
  return run_rows(r, s, r->eval[0], k, st, &n_farms, farms);
}

int wf_robust_optimize(wf_robust* r, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                       float* power_init, int on_device) {
  if (!r || !yaw_opt || !power_opt || !power_init) return ext_fail(r, WF_E_INVALID, "wf_robust_optimize: NULL argument");
  wf_handle* h = r->h;
  evaluator& es = r->eval[1];
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  search_policy k{"robust yaw optimisation serves", "wf_robust_optimize", r->M, no_members("wf_robust_optimize"), kRowsMsg, nullptr, nullptr, nullptr};
  k.reserve = [&](int E) -> int {
    const int rc = reserve(r, r->d_rowsum, (size_t)E);
    return rc == WF_OK ? reserve(r, r->s.d_wind, 2 * (size_t)E) : rc;
  };
  // every row's wind: its farm's speed and the farm's direction plus the member's offset — a wind per row; then the visit order
  k.begin_chunk = [&](const WfSlots& sl, int R, int E) -> int {
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = device_members(r); la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = R; la.N = h->N;
    la.ews = r->s.d_wind; la.ewd = r->s.d_wind + E;
    WFX_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    WFX_EV(r, es.ev, wf_set_wind_counts(es.ev, la.ews, E, la.ewd, E, 1));
    const WfRobustOrderArgs oa{{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, wind_stride, h->N, r->s.d_order}};
    WFX_HIP(r, wfk_launch_robust_order(&oa, h->stream));
    return WF_OK;
  };
  k.visit = [&](const WfAdvanceArgs& a, int v) -> int {  // the row sums of visit v - 1, then the advance launch
    const WfRobustRowsumArgs sa{a.sl.C * a.R * r->M, a.N, r->s.d_pow, r->d_rowsum};
    if (v > 0) WFX_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
    const WfRobustAdvanceArgs aa{a, device_members(r), r->d_rowsum};
    WFX_HIP(r, wfk_launch_robust_advance(&aa, h->stream));
    return WF_OK;
  };
  return run_search(r, r->s, es, k, yaw0, n_farms, farms, yaw_opt, power_opt, power_init, on_device);
}

// an evaluation, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0.
// a search with detail, per chunk: e0 | glue e | step e | glue e | ... | glue e: V + 1 glue intervals (the first one holds the
// chunk's lay-out and order kernels and the evaluator's wind too) and V step intervals, then the next chunk's e0
int wf_robust_last_timing(wf_robust* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  return last_timing(r, "neither wf_robust_optimize nor wf_robust_evaluate has run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_robust_evaluator(wf_robust* r) { return r ? r->eval[1].ev : nullptr; }

int wf_robust_kernel_info(wf_robust* r, int* info) {
  if (!r || !info) return ext_fail(r, WF_E_INVALID, "wf_robust_kernel_info: NULL argument");
  return kernel_info(r, WF_ROBUST_KERNELS, wfk_robust_func_attributes, info);
}

const char* wf_robust_last_error(wf_robust* r) { return r ? r->err.c_str() : "wf_robust: NULL object"; }

}  // extern "C"
