// wf_robust_abi.hip — the C boundary of the robust extension (include/wfrobust.h): an object that belongs to a parent
// handle, owns a member set, two evaluator handles and their device buffers, and enqueues a whole expected-power evaluation or
// a whole robust coordinate search on the parent's stream: per chunk one lay-out kernel, per visit one wf_step on the
// evaluator, one row-sum kernel and one advance kernel (wf_robust_kernels.hip).  Reads the parent (layout, model, wind,
// kernel choice, resolve mode); stores nothing in it.  The evaluators follow the idea of ensure_evaluator in
// yawopt/wf_yawopt_abi.hip — further handles configured through the public ABI of include/wfstep.h only — and share no
// state with it.
#include "../../../include/wfrobust.h"
#include "../wf_handle.h"
#include "wf_robust.h"

using namespace wfi;

// an evaluator and what it was built from
struct wf_robust_evaluator_state {
  wf_handle* ev = nullptr;
  int E = 0, mode = -1;
  wf_model_params model{};
  std::vector<double> tws, tct, tcp, lx, ly;
  wf_kernel_choice choice{};
  double guard = 0.0;
  hipStream_t stream = nullptr;
};

struct wf_robust {
  wf_handle* h = nullptr;
  std::string err;
  // configuration
  double lo = -25.0, hi = 25.0;
  int P = 2, K[WF_ROBUST_MAX_PASSES] = {5, 4, 0, 0};
  int strict = 0, max_eval = 65536;
  // the members: M == 0 = none yet; device copy [2][WF_ROBUST_MAX_MEMBERS] delta, normalised weight
  int M = 0, frame = WF_ROBUST_FIXED;
  double members[2 * WF_ROBUST_MAX_MEMBERS] = {};
  double* d_members = nullptr;
  // the evaluators: [0] wf_robust_evaluate (R = 1), [1] wf_robust_optimize
  wf_robust_evaluator_state eval[2];
  // device buffers (grow-only), shared by the two calls
  float *d_yaw = nullptr, *d_pow = nullptr, *d_best = nullptr;  // [E][N], [E][N], [C][N]
  double *d_rowsum = nullptr, *d_wind = nullptr;                // [E], [2][E]
  int *d_order = nullptr, *d_farms = nullptr;
  size_t yaw_cap = 0, pow_cap = 0, best_cap = 0, rowsum_cap = 0, wind_cap = 0, order_cap = 0, farms_cap = 0;
  std::vector<int> farms;  // host copy the upload reads from
  float *d_in = nullptr, *d_outf = nullptr;  // staging for host callers: the yaw rows; the float outputs
  double* d_outd = nullptr;                  // ... and the double outputs
  size_t in_cap = 0, outf_cap = 0, outd_cap = 0;
  // timing
  int detail = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t n_ev = 0;
  bool timed = false, timed_detail = false;
  int timed_kind = 0;  // 0 wf_robust_evaluate (four events per chunk), 1 wf_robust_optimize
  int timed_V = 0;
};

namespace {

int rfail(wf_robust* r, int code, const std::string& msg) {
  if (r) r->err = msg;
  return code;
}
#define WFB_HIP(r, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return rfail(r, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFB_EV(r, evh, call)                                                 \
  do {                                                                       \
    int rc_ = (call);                                                        \
    if (rc_ != WF_OK) return rfail(r, rc_, std::string("evaluator: ") + wf_last_error(evh)); \
  } while (0)
#define WFB_ON_DEVICE(r)                 \
  DeviceGuard guard_((r)->h->device);    \
  if (guard_.err != hipSuccess) return rfail(r, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer (the stream is drained before a buffer in use is released)
template <class T>
int reserve(wf_robust* r, T** buf, size_t* cap, size_t n) {
  if (n <= *cap) return WF_OK;
  WFB_HIP(r, hipStreamSynchronize(r->h->stream));
  hipFree(*buf);
  *buf = nullptr; *cap = 0;
  WFB_HIP(r, hipMalloc(buf, sizeof(T) * n));
  *cap = n;
  return WF_OK;
}

int k_max(const wf_robust* r) {
  int k = 0;
  for (int p = 0; p < r->P; ++p) k = r->K[p] > k ? r->K[p] : k;
  return k;
}

// what both calls ask of the parent and of their farm list; n_farms becomes the number of farms to serve
int check_call(wf_robust* r, const char* what, const char* call, int* n_farms, const int* farms) {
  wf_handle* h = r->h;
  if (h->N <= 0 || h->B <= 0) return rfail(r, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return rfail(r, WF_E_UNSUPPORTED, std::string(what) + " serves a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return rfail(r, WF_E_UNSUPPORTED, std::string(what) + " serves one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  if (h->wind_count == 0)
    return rfail(r, WF_E_INVALID, std::string("no wind has been set: wf_set_wind (or wf_wind_*) must be called before ") + call);
  if (r->M <= 0) return rfail(r, WF_E_INVALID, std::string("no members have been set: wf_robust_set_members must be called before ") + call);
  if (farms) {
    if (*n_farms < 1) return rfail(r, WF_E_INVALID, "n_farms must be >= 1");
    for (int k = 0; k < *n_farms; ++k)
      if (farms[k] < 0 || farms[k] >= h->B) return rfail(r, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  } else {
    *n_farms = h->B;
  }
  return WF_OK;
}

bool same_model(const wf_model_params& a, const wf_model_params& b) {  // (the tables are compared through the handle's vectors)
  return std::memcmp(&a, &b, offsetof(wf_model_params, n_table)) == 0 && a.n_table == b.n_table &&
         a.enable_secondary_steering == b.enable_secondary_steering && a.enable_yaw_added_recovery == b.enable_yaw_added_recovery &&
         a.enable_transverse_velocities == b.enable_transverse_velocities;
}

// An evaluator: a handle with the parent's model, layout, kernel choice and guard band on the parent's device and stream,
// E farms.  Rebuilt when any of these differs from what it was built from; the resolve mode and the stream are just set.
int ensure_evaluator(wf_robust* r, wf_robust_evaluator_state& s, int E, int mode) {
  wf_handle* h = r->h;
  const size_t n = (size_t)h->N;
  const bool same = s.ev && s.E == E && same_model(s.model, h->model) && s.tws == h->tws && s.tct == h->tct && s.tcp == h->tcp &&
                    s.lx.size() == n && std::equal(s.lx.begin(), s.lx.end(), h->lx.begin()) &&
                    std::equal(s.ly.begin(), s.ly.end(), h->ly.begin()) &&
                    std::memcmp(&s.choice, &h->choice, sizeof(wf_kernel_choice)) == 0 && s.guard == h->guard_rel;
  if (same) {
    if (s.stream != h->stream) {
      WFB_EV(r, s.ev, wf_set_stream(s.ev, (void*)h->stream, 1));
      s.stream = h->stream;
    }
    if (s.mode != mode) {
      WFB_EV(r, s.ev, wf_set_risk_resolve(s.ev, mode));
      s.mode = mode;
    }
    return WF_OK;
  }
  WFB_HIP(r, hipStreamSynchronize(h->stream));
  if (s.ev) wf_destroy(s.ev);
  s.ev = nullptr;
  wf_handle* ev = nullptr;
  if (wf_create(h->device, &ev) != WF_OK) return rfail(r, WF_E_HIP, std::string("evaluator: ") + wf_last_error(nullptr));
  s.ev = ev;
  wf_model_params m = h->model;
  m.table_ws = h->tws.data(); m.table_ct = h->tct.data(); m.table_cp = h->tcp.data();
  WFB_EV(r, ev, wf_set_stream(ev, (void*)h->stream, 1));
  WFB_EV(r, ev, wf_set_model(ev, &m));
  WFB_EV(r, ev, wf_set_kernel_choice(ev, &h->choice));
  if (h->guard_user) WFB_EV(r, ev, wf_set_risk_guard(ev, h->guard_rel));
  WFB_EV(r, ev, wf_set_layout(ev, h->N, h->lx.data(), h->ly.data()));
  WFB_EV(r, ev, wf_set_batch(ev, E));
  WFB_EV(r, ev, wf_set_risk_resolve(ev, mode));
  s.E = E; s.mode = mode; s.stream = h->stream;
  s.model = h->model; s.tws = h->tws; s.tct = h->tct; s.tcp = h->tcp;
  s.lx.assign(h->lx.begin(), h->lx.begin() + n); s.ly.assign(h->ly.begin(), h->ly.begin() + n);
  s.choice = h->choice; s.guard = h->guard_rel;
  return WF_OK;
}

int record(wf_robust* r) {
  if (r->n_ev == r->ev_pool.size()) {
    hipEvent_t e = nullptr;
    WFB_HIP(r, hipEventCreate(&e));
    r->ev_pool.push_back(e);
  }
  WFB_HIP(r, hipEventRecord(r->ev_pool[r->n_ev++], r->h->stream));
  return WF_OK;
}

// the farm list on the device (a previous upload may still read the host copy: drain first)
int upload_farms(wf_robust* r, const int* farms, int n_farms) {
  WFB_HIP(r, hipStreamSynchronize(r->h->stream));
  r->farms.assign(farms, farms + n_farms);
  WFB_HIP(r, hipMemcpyAsync(r->d_farms, r->farms.data(), sizeof(int) * n_farms, hipMemcpyHostToDevice, r->h->stream));
  return WF_OK;
}

WfRobustMembers device_members(const wf_robust* r) {
  return WfRobustMembers{r->d_members, r->d_members + WF_ROBUST_MAX_MEMBERS, r->M, r->frame};
}

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least (K_max + 1) x members";

}  // namespace

extern "C" {

int wf_robust_create(wf_handle* h, wf_robust** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  wf_robust* r = new (std::nothrow) wf_robust();
  if (!r) return fail(h, WF_E_NOMEM, "out of host memory");
  r->h = h;
  *out = r;
  return WF_OK;
}

int wf_robust_destroy(wf_robust* r) {
  if (!r) return WF_OK;
  DeviceGuard guard(r->h->device);
  hipStreamSynchronize(r->h->stream);
  for (auto& s : r->eval)
    if (s.ev) wf_destroy(s.ev);
  hipFree(r->d_members); hipFree(r->d_yaw); hipFree(r->d_pow); hipFree(r->d_best); hipFree(r->d_rowsum); hipFree(r->d_wind);
  hipFree(r->d_order); hipFree(r->d_farms); hipFree(r->d_in); hipFree(r->d_outf); hipFree(r->d_outd);
  for (hipEvent_t e : r->ev_pool) hipEventDestroy(e);
  delete r;
  return WF_OK;
}

int wf_robust_set_members(wf_robust* r, int M, const double* delta, const double* weight, int frame) {
  if (!r || !delta || !weight) return rfail(r, WF_E_INVALID, "wf_robust_set_members: NULL argument");
  if (M < 1 || M > WF_ROBUST_MAX_MEMBERS) return rfail(r, WF_E_INVALID, "the number of members must be in 1..33");
  if (frame != WF_ROBUST_RELATIVE && frame != WF_ROBUST_FIXED)
    return rfail(r, WF_E_INVALID, "frame must be WF_ROBUST_RELATIVE (0) or WF_ROBUST_FIXED (1)");
  double sum = 0.0;
  for (int m = 0; m < M; ++m) {
    if (!std::isfinite(delta[m]) || (m > 0 && !(delta[m] > delta[m - 1])))
      return rfail(r, WF_E_INVALID, "member offsets (delta) must be finite and strictly ascending");
    if (!std::isfinite(weight[m]) || !(weight[m] >= 0.0)) return rfail(r, WF_E_INVALID, "member weights must be finite and >= 0 (no negative weight)");
    sum += weight[m];
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) return rfail(r, WF_E_INVALID, "member weights must have a positive sum (they are all zero)");
  WFB_ON_DEVICE(r);
  hipStream_t st = r->h->stream;
  WFB_HIP(r, hipStreamSynchronize(st));  // (a previous upload may still read the host copy; running kernels read the device one)
  r->M = 0;
  if (!r->d_members) WFB_HIP(r, hipMalloc(&r->d_members, sizeof(r->members)));
  for (int m = 0; m < WF_ROBUST_MAX_MEMBERS; ++m) {
    r->members[m] = m < M ? delta[m] : 0.0;
    r->members[WF_ROBUST_MAX_MEMBERS + m] = m < M ? weight[m] / sum : 0.0;
  }
  WFB_HIP(r, hipMemcpyAsync(r->d_members, r->members, sizeof(r->members), hipMemcpyHostToDevice, st));
  WFB_HIP(r, hipStreamSynchronize(st));
  r->M = M; r->frame = frame;
  return WF_OK;
}

int wf_robust_config(wf_robust* r, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms) {
  if (!r || !K) return rfail(r, WF_E_INVALID, "wf_robust_config: NULL argument");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return rfail(r, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (n_passes < 1 || n_passes > WF_ROBUST_MAX_PASSES) return rfail(r, WF_E_INVALID, "the number of passes must be in 1..4");
  if (K[0] < 2 || K[0] > WF_ROBUST_MAX_K0) return rfail(r, WF_E_INVALID, "the first pass needs 2..31 candidates (K_0)");
  for (int p = 1; p < n_passes; ++p)
    if (K[p] < 1 || K[p] > WF_ROBUST_MAX_K) return rfail(r, WF_E_INVALID, "a refining pass needs 1..15 candidates (K_p)");
  int km = 0;
  for (int p = 0; p < n_passes; ++p) km = K[p] > km ? K[p] : km;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (max_eval_farms < (km + 1) * (r->M > 0 ? r->M : 1)) return rfail(r, WF_E_INVALID, kRowsMsg);
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
  int rc = check_call(r, "expected power under uncertainty", "wf_robust_evaluate", &n_farms, farms);
  if (rc != WF_OK) return rc;
  const int N = h->N, M = r->M;
  if (r->max_eval < M) return rfail(r, WF_E_INVALID, kRowsMsg);
  WFB_ON_DEVICE(r);
  int C = r->max_eval / M;
  if (C > n_farms) C = n_farms;
  const int E = C * M;
  wf_robust_evaluator_state& es = r->eval[0];
  rc = ensure_evaluator(r, es, E, r->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N, fm = (size_t)n_farms * M;
  rc = reserve(r, &r->d_yaw, &r->yaw_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_pow, &r->pow_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_rowsum, &r->rowsum_cap, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_wind, &r->wind_cap, 2 * (size_t)E);
  if (rc == WF_OK && farms) rc = reserve(r, &r->d_farms, &r->farms_cap, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw) rc = reserve(r, &r->d_in, &r->in_cap, fn);
  if (rc == WF_OK && !on_device) rc = reserve(r, &r->d_outd, &r->outd_cap, fn + (size_t)n_farms);
  if (rc == WF_OK && !on_device) rc = reserve(r, &r->d_outf, &r->outf_cap, fm);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(r, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw_in = yaw;
  if (yaw && !on_device) {
    WFB_HIP(r, hipMemcpyAsync(r->d_in, yaw, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw_in = r->d_in;
  }
  double* d_exp = expected_power ? (on_device ? expected_power : r->d_outd) : nullptr;
  double* d_turb = expected_turbine_power ? (on_device ? expected_turbine_power : r->d_outd + n_farms) : nullptr;
  float* d_mem = member_power ? (on_device ? member_power : r->d_outf) : nullptr;
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  r->n_ev = 0; r->timed = false;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfRobustSlots sl{farms ? r->d_farms : nullptr, base, n_slots, C};
    if ((rc = record(r)) != WF_OK) return rc;
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = device_members(r); la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = 1; la.N = N;
    la.ews = r->d_wind; la.ewd = r->d_wind + E; la.write_yaw = 1;
    la.yaw_in = d_yaw_in ? d_yaw_in + (size_t)base * N : nullptr; la.yaw = r->d_yaw;
    WFB_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
    WFB_EV(r, es.ev, wf_set_wind_counts(es.ev, la.ews, E, la.ewd, E, 1));
    WFB_EV(r, es.ev, wf_step(es.ev, r->d_yaw, r->d_pow, nullptr, nullptr, nullptr, 1));
    if ((rc = record(r)) != WF_OK) return rc;
    const WfRobustRowsumArgs sa{E, N, r->d_pow, r->d_rowsum};
    WFB_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
    WfRobustExpectArgs xa{};
    xa.sl = sl; xa.mb = la.mb; xa.N = N; xa.power = r->d_pow; xa.rowsum = r->d_rowsum;
    xa.expected = d_exp ? d_exp + base : nullptr;
    xa.turbine = d_turb ? d_turb + (size_t)base * N : nullptr;
    xa.member = d_mem ? d_mem + (size_t)base * M : nullptr;
    WFB_HIP(r, wfk_launch_robust_expect(&xa, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
  }
  r->timed = true; r->timed_kind = 0;
  if (!on_device) {
    if (expected_power) WFB_HIP(r, hipMemcpyAsync(expected_power, r->d_outd, sizeof(double) * n_farms, hipMemcpyDeviceToHost, h->stream));
    if (expected_turbine_power)
      WFB_HIP(r, hipMemcpyAsync(expected_turbine_power, r->d_outd + n_farms, sizeof(double) * fn, hipMemcpyDeviceToHost, h->stream));
    if (member_power) WFB_HIP(r, hipMemcpyAsync(member_power, r->d_outf, sizeof(float) * fm, hipMemcpyDeviceToHost, h->stream));
    WFB_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_robust_optimize(wf_robust* r, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                       float* power_init, int on_device) {
  if (!r || !yaw_opt || !power_opt || !power_init) return rfail(r, WF_E_INVALID, "wf_robust_optimize: NULL argument");
  wf_handle* h = r->h;
  int rc = check_call(r, "robust yaw optimisation", "wf_robust_optimize", &n_farms, farms);
  if (rc != WF_OK) return rc;
  const int N = h->N, M = r->M, R = k_max(r) + 1, RM = R * M;
  if (r->max_eval < RM) return rfail(r, WF_E_INVALID, kRowsMsg);
  WFB_ON_DEVICE(r);
  int C = r->max_eval / RM;
  if (C > n_farms) C = n_farms;
  const int E = C * RM;
  wf_robust_evaluator_state& es = r->eval[1];
  rc = ensure_evaluator(r, es, E, r->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N;
  rc = reserve(r, &r->d_yaw, &r->yaw_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_pow, &r->pow_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_rowsum, &r->rowsum_cap, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_wind, &r->wind_cap, 2 * (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_best, &r->best_cap, (size_t)C * N);
  if (rc == WF_OK) rc = reserve(r, &r->d_order, &r->order_cap, (size_t)C * N);
  if (rc == WF_OK && farms) rc = reserve(r, &r->d_farms, &r->farms_cap, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw0) rc = reserve(r, &r->d_in, &r->in_cap, fn);
  if (rc == WF_OK && !on_device) rc = reserve(r, &r->d_outf, &r->outf_cap, fn + 2 * (size_t)n_farms);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(r, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw0 = yaw0;
  if (yaw0 && !on_device) {
    WFB_HIP(r, hipMemcpyAsync(r->d_in, yaw0, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw0 = r->d_in;
  }
  float* d_oyaw = on_device ? yaw_opt : r->d_outf;
  float* d_opow = on_device ? power_opt : r->d_outf + fn;
  float* d_oini = on_device ? power_init : r->d_outf + fn + n_farms;

  // the passes' grids (include/wfyawopt.h): h_0 = (hi - lo) / (K_0 - 1), h_p = 2 h_{p-1} / (K_p + 1)
  WfRobustGrid grid[WF_ROBUST_MAX_PASSES];
  {
    double hp = (r->hi - r->lo) / (double)(r->K[0] - 1);
    grid[0] = WfRobustGrid{0, 0, r->K[0], r->lo, hp};
    for (int p = 1; p < r->P; ++p) {
      const double s = 2.0 * hp / (double)(r->K[p] + 1);
      grid[p] = WfRobustGrid{0, 1, r->K[p], hp, s};
      hp = s;
    }
  }
  const WfRobustGrid none{-1, 0, 0, 0.0, 0.0};
  const int V = r->P * N;  // visits
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  const WfRobustMembers mb = device_members(r);
  r->n_ev = 0; r->timed = false;
  const bool detail = r->detail != 0;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfRobustSlots sl{farms ? r->d_farms : nullptr, base, n_slots, C};
    if (base == 0 || detail) { rc = record(r); if (rc != WF_OK) return rc; }  // (detail: 2 V + 2 events per chunk)
    // every row's wind: its farm's speed and the farm's direction plus the member's offset — a wind per row
    WfRobustLayoutArgs la{};
    la.sl = sl; la.mb = mb; la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.R = R; la.N = N;
    la.ews = r->d_wind; la.ewd = r->d_wind + E;
    WFB_HIP(r, wfk_launch_robust_layout(&la, h->stream));
    WFB_EV(r, es.ev, wf_set_wind_counts(es.ev, la.ews, E, la.ewd, E, 1));
    const WfRobustOrderArgs oa{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, wind_stride, N, r->d_order};
    WFB_HIP(r, wfk_launch_robust_order(&oa, h->stream));
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
      if (v > 0) WFB_HIP(r, wfk_launch_robust_rowsum(&sa, h->stream));
      WFB_HIP(r, wfk_launch_robust_advance(&aa, h->stream));
      if (detail) { rc = record(r); if (rc != WF_OK) return rc; }
      if (v < V) {
        WFB_EV(r, es.ev, wf_step(es.ev, r->d_yaw, r->d_pow, nullptr, nullptr, nullptr, 1));
        if (detail) { rc = record(r); if (rc != WF_OK) return rc; }
      }
    }
  }
  if (!detail) { rc = record(r); if (rc != WF_OK) return rc; }
  r->timed = true; r->timed_detail = detail; r->timed_kind = 1; r->timed_V = V;
  if (!on_device) {
    WFB_HIP(r, hipMemcpyAsync(yaw_opt, r->d_outf, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    WFB_HIP(r, hipMemcpyAsync(power_opt, r->d_outf + fn, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFB_HIP(r, hipMemcpyAsync(power_init, r->d_outf + fn + n_farms, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFB_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_robust_last_timing(wf_robust* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  if (!r->timed || r->n_ev < 2) return rfail(r, WF_E_INVALID, "neither wf_robust_optimize nor wf_robust_evaluate has run yet");
  WFB_ON_DEVICE(r);
  WFB_HIP(r, hipEventSynchronize(r->ev_pool[r->n_ev - 1]));
  float total = 0.0f, step = 0.0f, glue = 0.0f;
  WFB_HIP(r, hipEventElapsedTime(&total, r->ev_pool[0], r->ev_pool[r->n_ev - 1]));
  if (r->timed_kind == 0 || r->timed_detail) {
    // an evaluation, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0.
    // a search, per chunk: e0 | glue e | step e | glue e | ... | glue e: V + 1 glue intervals (the first one holds the chunk's
    // lay-out and order kernels and the evaluator's wind too) and V step intervals, then the next chunk's e0
    const size_t per_chunk = r->timed_kind == 0 ? 4 : 2 * (size_t)r->timed_V + 2;
    for (size_t k = 1; k < r->n_ev; ++k) {
      float ms = 0.0f;
      WFB_HIP(r, hipEventElapsedTime(&ms, r->ev_pool[k - 1], r->ev_pool[k]));
      const size_t q = k % per_chunk;
      if (q != 0 && q % 2 == 0) step += ms;
      else glue += ms;
    }
  }
  if (total_ms) *total_ms = total;
  if (step_ms) *step_ms = step;
  if (glue_ms) *glue_ms = glue;
  return WF_OK;
}

wf_handle* wf_robust_evaluator(wf_robust* r) { return r ? r->eval[1].ev : nullptr; }

int wf_robust_kernel_info(wf_robust* r, int* info) {
  if (!r || !info) return rfail(r, WF_E_INVALID, "wf_robust_kernel_info: NULL argument");
  WFB_ON_DEVICE(r);
  for (int k = 0; k < WF_ROBUST_KERNELS; ++k) {
    hipFuncAttributes a{};
    WFB_HIP(r, wfk_robust_func_attributes(k, &a));
    info[3 * k] = a.numRegs; info[3 * k + 1] = (int)a.sharedSizeBytes; info[3 * k + 2] = (int)a.localSizeBytes;
  }
  return WF_OK;
}

const char* wf_robust_last_error(wf_robust* r) { return r ? r->err.c_str() : "wf_robust: NULL object"; }

}  // extern "C"
