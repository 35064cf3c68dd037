// wf_robust_abi.hip — the C boundary of the robust extension (include/wfrobust.h): an object that belongs to a parent
// handle, owns a member set, two evaluator handles and their device buffers, and enqueues a whole expected-power evaluation or
// a whole robust coordinate search on the parent's stream: per chunk one lay-out kernel, per visit one wf_step on the
// evaluator, one row-sum kernel and one advance kernel (wf_robust_kernels.hip).  Reads the parent (layout, model, wind,
// kernel choice, resolve mode); stores nothing in it.  The object's scaffolding — base, buffers, the evaluators that follow
// the parent, checks, events, the passes' grids — is the extensions' shared layer (ext/wf_ext.h).
#include "../../../include/wfrobust.h"
#include "../ext/wf_ext.h"
#include "wf_robust.h"

using namespace wfi;

struct wf_robust : ext_base {
  // configuration
  double lo = -25.0, hi = 25.0;
  int P = 2, K[WF_ROBUST_MAX_PASSES] = {5, 4, 0, 0};
  int strict = 0, max_eval = 65536;
  // the members: M == 0 = none yet; device copy [2][WF_ROBUST_MAX_MEMBERS] delta, normalised weight
  int M = 0, frame = WF_ROBUST_FIXED;
  double members[2 * WF_ROBUST_MAX_MEMBERS] = {};
  dev_buf<double> d_members;
  // device buffers (grow-only), shared by the two calls
  dev_buf<float> d_yaw, d_pow, d_best;  // [E][N], [E][N], [C][N]
  dev_buf<double> d_rowsum, d_wind;     // [E], [2][E]
  dev_buf<int> d_order;
  farm_list farms;
  dev_buf<float> d_in, d_outf;  // staging for host callers: the yaw rows; the float outputs
  dev_buf<double> d_outd;       // ... and the double outputs
  // the evaluators: [0] wf_robust_evaluate (R = 1), [1] wf_robust_optimize
  evaluator eval[2];
};

namespace {

// what both calls ask of the parent and of their farm list; n_farms becomes the number of farms to serve
int check_call(wf_robust* r, const char* what, const char* call, int* n_farms, const int* farms) {
  int rc = check_parent(r, what, call);
  if (rc != WF_OK) return rc;
  if (r->M <= 0) return ext_fail(r, WF_E_INVALID, std::string("no members have been set: wf_robust_set_members must be called before ") + call);
  return check_farms(r, n_farms, farms);
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
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return ext_fail(r, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (n_passes < 1 || n_passes > WF_ROBUST_MAX_PASSES) return ext_fail(r, WF_E_INVALID, "the number of passes must be in 1..4");
  if (K[0] < 2 || K[0] > WF_ROBUST_MAX_K0) return ext_fail(r, WF_E_INVALID, "the first pass needs 2..31 candidates (K_0)");
  for (int p = 1; p < n_passes; ++p)
    if (K[p] < 1 || K[p] > WF_ROBUST_MAX_K) return ext_fail(r, WF_E_INVALID, "a refining pass needs 1..15 candidates (K_p)");
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (max_eval_farms < (k_max(n_passes, K) + 1) * (r->M > 0 ? r->M : 1)) return ext_fail(r, WF_E_INVALID, kRowsMsg);
  r->lo = lo; r->hi = hi; r->P = n_passes;
  for (int p = 0; p < WF_ROBUST_MAX_PASSES; ++p) r->K[p] = p < n_passes ? K[p] : 0;
  r->strict = strict != 0; r->max_eval = max_eval_farms;
  return WF_OK;
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
  int rc = check_call(r, "expected power under uncertainty serves", "wf_robust_evaluate", &n_farms, farms);
  if (rc != WF_OK) return rc;
  const int N = h->N, M = r->M;
  if (r->max_eval < M) return ext_fail(r, WF_E_INVALID, kRowsMsg);
  WFX_ON_DEVICE(r);
  int C = r->max_eval / M;
  if (C > n_farms) C = n_farms;
  const int E = C * M;
  evaluator& es = r->eval[0];
  rc = ensure_evaluator(r, es, E, r->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N, fm = (size_t)n_farms * M;
  rc = reserve(r, r->d_yaw, en);
  if (rc == WF_OK) rc = reserve(r, r->d_pow, en);
  if (rc == WF_OK) rc = reserve(r, r->d_rowsum, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, r->d_wind, 2 * (size_t)E);
  if (rc == WF_OK && farms) rc = reserve(r, r->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw) rc = reserve(r, r->d_in, fn);
  if (rc == WF_OK && !on_device) rc = reserve(r, r->d_outd, fn + (size_t)n_farms);
  if (rc == WF_OK && !on_device) rc = reserve(r, r->d_outf, fm);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(r, r->farms, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw_in = yaw;
  if (yaw && !on_device) {
    WFX_HIP(r, hipMemcpyAsync(r->d_in, yaw, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw_in = r->d_in;
  }
  double* d_exp = expected_power ? (on_device ? expected_power : r->d_outd) : nullptr;
  double* d_turb = expected_turbine_power ? (on_device ? expected_turbine_power : r->d_outd + n_farms) : nullptr;
  float* d_mem = member_power ? (on_device ? member_power : r->d_outf) : nullptr;
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  r->n_ev = 0; r->timed = false;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfSlots sl{farms ? r->farms.d.p : nullptr, base, n_slots, C};
    if ((rc = record(r)) != WF_OK) return rc;
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = device_members(r); la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = 1; la.N = N;
    la.ews = r->d_wind; la.ewd = r->d_wind + E; la.write_yaw = 1;
    la.yaw_in = d_yaw_in ? d_yaw_in + (size_t)base * N : nullptr; la.yaw = r->d_yaw;
    WFX_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
    WFX_EV(r, es.ev, wf_set_wind_counts(es.ev, la.ews, E, la.ewd, E, 1));
    WFX_EV(r, es.ev, wf_step(es.ev, r->d_yaw, r->d_pow, nullptr, nullptr, nullptr, 1));
    if ((rc = record(r)) != WF_OK) return rc;
    const WfRobustRowsumArgs sa{E, N, r->d_pow, r->d_rowsum};
    WFX_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
    WfRobustExpectArgs xa{};
    xa.sl = sl; xa.mb = la.mb; xa.N = N; xa.power = r->d_pow; xa.rowsum = r->d_rowsum;
    xa.expected = d_exp ? d_exp + base : nullptr;
    xa.turbine = d_turb ? d_turb + (size_t)base * N : nullptr;
    xa.member = d_mem ? d_mem + (size_t)base * M : nullptr;
    WFX_HIP(r, wfk_launch_robust_expect(&xa, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
  }
  r->timed = true; r->per_chunk = 4;
  if (!on_device) {
    if (expected_power) WFX_HIP(r, hipMemcpyAsync(expected_power, r->d_outd, sizeof(double) * n_farms, hipMemcpyDeviceToHost, h->stream));
    if (expected_turbine_power)
      WFX_HIP(r, hipMemcpyAsync(expected_turbine_power, r->d_outd + n_farms, sizeof(double) * fn, hipMemcpyDeviceToHost, h->stream));
    if (member_power) WFX_HIP(r, hipMemcpyAsync(member_power, r->d_outf, sizeof(float) * fm, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_robust_optimize(wf_robust* r, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                       float* power_init, int on_device) {
  if (!r || !yaw_opt || !power_opt || !power_init) return ext_fail(r, WF_E_INVALID, "wf_robust_optimize: NULL argument");
  wf_handle* h = r->h;
  int rc = check_call(r, "robust yaw optimisation serves", "wf_robust_optimize", &n_farms, farms);
  if (rc != WF_OK) return rc;
  const int N = h->N, M = r->M, R = k_max(r->P, r->K) + 1, RM = R * M;
  if (r->max_eval < RM) return ext_fail(r, WF_E_INVALID, kRowsMsg);
  WFX_ON_DEVICE(r);
  int C = r->max_eval / RM;
  if (C > n_farms) C = n_farms;
  const int E = C * RM;
  evaluator& es = r->eval[1];
  rc = ensure_evaluator(r, es, E, r->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N;
  rc = reserve(r, r->d_yaw, en);
  if (rc == WF_OK) rc = reserve(r, r->d_pow, en);
  if (rc == WF_OK) rc = reserve(r, r->d_rowsum, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, r->d_wind, 2 * (size_t)E);
  if (rc == WF_OK) rc = reserve(r, r->d_best, (size_t)C * N);
  if (rc == WF_OK) rc = reserve(r, r->d_order, (size_t)C * N);
  if (rc == WF_OK && farms) rc = reserve(r, r->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw0) rc = reserve(r, r->d_in, fn);
  if (rc == WF_OK && !on_device) rc = reserve(r, r->d_outf, fn + 2 * (size_t)n_farms);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(r, r->farms, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw0 = yaw0;
  if (yaw0 && !on_device) {
    WFX_HIP(r, hipMemcpyAsync(r->d_in, yaw0, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw0 = r->d_in;
  }
  float* d_oyaw = on_device ? yaw_opt : r->d_outf;
  float* d_opow = on_device ? power_opt : r->d_outf + fn;
  float* d_oini = on_device ? power_init : r->d_outf + fn + n_farms;

  // the passes' grids (include/wfyawopt.h): h_0 = (hi - lo) / (K_0 - 1), h_p = 2 h_{p-1} / (K_p + 1)
  WfGrid grid[WF_ROBUST_MAX_PASSES];
  pass_grids(r->lo, r->hi, r->P, r->K, grid);
  const WfGrid none{-1, 0, 0, 0.0, 0.0};
  const int V = r->P * N;  // visits
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  const WfRobustMembers mb = device_members(r);
  r->n_ev = 0; r->timed = false;
  const bool detail = r->detail != 0;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfSlots sl{farms ? r->farms.d.p : nullptr, base, n_slots, C};
    if (base == 0 || detail) { rc = record(r); if (rc != WF_OK) return rc; }  // (detail: 2 V + 2 events per chunk)
    // every row's wind: its farm's speed and the farm's direction plus the member's offset — a wind per row
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = mb; la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = R; la.N = N;
    la.ews = r->d_wind; la.ewd = r->d_wind + E;
    WFX_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    WFX_EV(r, es.ev, wf_set_wind_counts(es.ev, la.ews, E, la.ewd, E, 1));
    const WfRobustOrderArgs oa{{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, wind_stride, N, r->d_order}};
    WFX_HIP(r, wfk_launch_robust_order(&oa, h->stream));
    const WfRobustRowsumArgs sa{E, N, r->d_pow, r->d_rowsum};
    WfRobustAdvanceArgs aa{};
    aa.sl = sl; aa.mb = mb; aa.N = N; aa.R = R; aa.lo = r->lo; aa.hi = r->hi;
    aa.order = r->d_order; aa.rowsum = r->d_rowsum; aa.yaw = r->d_yaw; aa.best = r->d_best;
    aa.yaw0 = d_yaw0 ? d_yaw0 + (size_t)base * N : nullptr;
    aa.out_yaw = d_oyaw + (size_t)base * N; aa.out_power = d_opow + base; aa.out_init = d_oini + base;
    for (int v = 0; v <= V; ++v) {  // launch v lays out visit v (v < V) from the row sums of visit v - 1 (v > 0)
      aa.prev = none; aa.next = none;
      if (v > 0) { aa.prev = grid[(v - 1) / N]; aa.prev.s = (v - 1) % N; }
      if (v < V) { aa.next = grid[v / N]; aa.next.s = v % N; }
      aa.first = v == 1;
      if (v > 0) WFX_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
      WFX_HIP(r, wfk_launch_robust_advance(&aa, h->stream));
      if (detail) { rc = record(r); if (rc != WF_OK) return rc; }
      if (v < V) {
        WFX_EV(r, es.ev, wf_step(es.ev, r->d_yaw, r->d_pow, nullptr, nullptr, nullptr, 1));
        if (detail) { rc = record(r); if (rc != WF_OK) return rc; }
      }
    }
  }
  if (!detail) { rc = record(r); if (rc != WF_OK) return rc; }
  r->timed = true; r->per_chunk = detail ? 2 * (size_t)V + 2 : 0;
  if (!on_device) {
    WFX_HIP(r, hipMemcpyAsync(yaw_opt, r->d_outf, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(r, hipMemcpyAsync(power_opt, r->d_outf + fn, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(r, hipMemcpyAsync(power_init, r->d_outf + fn + n_farms, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
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
