// wf_grad_abi.hip — the C boundary of the gradient extension (include/wfgrad.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole sensitivity run on the parent's stream: per chunk one
// lay-out kernel, one wf_step on the evaluator and one reduce kernel (wf_grad_kernels.hip).  Reads the parent (layout, model,
// wind, kernel choice, resolve mode); stores nothing in it.  The evaluator follows the idea of ensure_evaluator in
// robust/wf_robust_abi.hip — a further handle configured through the public ABI of include/wfstep.h only — and shares no
// state with it.
#include "../../../include/wfgrad.h"
#include "../wf_handle.h"
#include "wf_grad.h"

using namespace wfi;

struct wf_grad {
  wf_handle* h = nullptr;
  std::string err;
  // configuration
  double step = 1.0, lo = -45.0, hi = 45.0;
  int strict = 0, max_eval = 65536;
  // the evaluator and what it was built from
  wf_handle* ev = nullptr;
  int E = 0, mode = -1;
  wf_model_params model{};
  std::vector<double> tws, tct, tcp, lx, ly;
  wf_kernel_choice choice{};
  double guard = 0.0;
  hipStream_t stream = nullptr;
  // device buffers (grow-only)
  float *d_yaw = nullptr, *d_pow = nullptr;  // [E][N], [E][N]
  double *d_wind = nullptr, *d_div = nullptr;  // [2][E], [C][N]
  int* d_farms = nullptr;
  size_t yaw_cap = 0, pow_cap = 0, wind_cap = 0, div_cap = 0, farms_cap = 0;
  std::vector<int> farms;  // host copy the upload reads from
  float *d_in = nullptr, *d_outf = nullptr;  // staging for host callers: yaw and cotangent rows; the float output
  double* d_outd = nullptr;                  // ... and the double outputs
  size_t in_cap = 0, outf_cap = 0, outd_cap = 0;
  // timing
  int detail = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t n_ev = 0;
  bool timed = false, timed_detail = false;
};

namespace {

int gfail(wf_grad* g, int code, const std::string& msg) {
  if (g) g->err = msg;
  return code;
}
#define WFG_HIP(g, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return gfail(g, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFG_EV(g, call)                                                      \
  do {                                                                       \
    int rc_ = (call);                                                        \
    if (rc_ != WF_OK) return gfail(g, rc_, std::string("evaluator: ") + wf_last_error((g)->ev)); \
  } while (0)
#define WFG_ON_DEVICE(g)                 \
  DeviceGuard guard_((g)->h->device);    \
  if (guard_.err != hipSuccess) return gfail(g, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer (the stream is drained before a buffer in use is released)
template <class T>
int reserve(wf_grad* g, T** buf, size_t* cap, size_t n) {
  if (n <= *cap) return WF_OK;
  WFG_HIP(g, hipStreamSynchronize(g->h->stream));
  hipFree(*buf);
  *buf = nullptr; *cap = 0;
  WFG_HIP(g, hipMalloc(buf, sizeof(T) * n));
  *cap = n;
  return WF_OK;
}

bool same_model(const wf_model_params& a, const wf_model_params& b) {  // (the tables are compared through the handle's vectors)
  return std::memcmp(&a, &b, offsetof(wf_model_params, n_table)) == 0 && a.n_table == b.n_table &&
         a.enable_secondary_steering == b.enable_secondary_steering && a.enable_yaw_added_recovery == b.enable_yaw_added_recovery &&
         a.enable_transverse_velocities == b.enable_transverse_velocities;
}

// The evaluator: a handle with the parent's model, layout, kernel choice and guard band on the parent's device and stream,
// E farms.  Rebuilt when any of these differs from what it was built from; the resolve mode and the stream are just set.
int ensure_evaluator(wf_grad* g, int E, int mode) {
  wf_handle* h = g->h;
  const size_t n = (size_t)h->N;
  const bool same = g->ev && g->E == E && same_model(g->model, h->model) && g->tws == h->tws && g->tct == h->tct && g->tcp == h->tcp &&
                    g->lx.size() == n && std::equal(g->lx.begin(), g->lx.end(), h->lx.begin()) &&
                    std::equal(g->ly.begin(), g->ly.end(), h->ly.begin()) &&
                    std::memcmp(&g->choice, &h->choice, sizeof(wf_kernel_choice)) == 0 && g->guard == h->guard_rel;
  if (same) {
    if (g->stream != h->stream) {
      WFG_EV(g, wf_set_stream(g->ev, (void*)h->stream, 1));
      g->stream = h->stream;
    }
    if (g->mode != mode) {
      WFG_EV(g, wf_set_risk_resolve(g->ev, mode));
      g->mode = mode;
    }
    return WF_OK;
  }
  WFG_HIP(g, hipStreamSynchronize(h->stream));
  if (g->ev) wf_destroy(g->ev);
  g->ev = nullptr;
  wf_handle* ev = nullptr;
  if (wf_create(h->device, &ev) != WF_OK) return gfail(g, WF_E_HIP, std::string("evaluator: ") + wf_last_error(nullptr));
  g->ev = ev;
  wf_model_params m = h->model;
  m.table_ws = h->tws.data(); m.table_ct = h->tct.data(); m.table_cp = h->tcp.data();
  WFG_EV(g, wf_set_stream(ev, (void*)h->stream, 1));
  WFG_EV(g, wf_set_model(ev, &m));
  WFG_EV(g, wf_set_kernel_choice(ev, &h->choice));
  if (h->guard_user) WFG_EV(g, wf_set_risk_guard(ev, h->guard_rel));
  WFG_EV(g, wf_set_layout(ev, h->N, h->lx.data(), h->ly.data()));
  WFG_EV(g, wf_set_batch(ev, E));
  WFG_EV(g, wf_set_risk_resolve(ev, mode));
  g->E = E; g->mode = mode; g->stream = h->stream;
  g->model = h->model; g->tws = h->tws; g->tct = h->tct; g->tcp = h->tcp;
  g->lx.assign(h->lx.begin(), h->lx.begin() + n); g->ly.assign(h->ly.begin(), h->ly.begin() + n);
  g->choice = h->choice; g->guard = h->guard_rel;
  return WF_OK;
}

int record(wf_grad* g) {
  if (g->n_ev == g->ev_pool.size()) {
    hipEvent_t e = nullptr;
    WFG_HIP(g, hipEventCreate(&e));
    g->ev_pool.push_back(e);
  }
  WFG_HIP(g, hipEventRecord(g->ev_pool[g->n_ev++], g->h->stream));
  return WF_OK;
}

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least 2 N + 1";

}  // namespace

extern "C" {

int wf_grad_create(wf_handle* h, wf_grad** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  wf_grad* g = new (std::nothrow) wf_grad();
  if (!g) return fail(h, WF_E_NOMEM, "out of host memory");
  g->h = h;
  *out = g;
  return WF_OK;
}

int wf_grad_destroy(wf_grad* g) {
  if (!g) return WF_OK;
  DeviceGuard guard(g->h->device);
  hipStreamSynchronize(g->h->stream);
  if (g->ev) wf_destroy(g->ev);
  hipFree(g->d_yaw); hipFree(g->d_pow); hipFree(g->d_wind); hipFree(g->d_div); hipFree(g->d_farms);
  hipFree(g->d_in); hipFree(g->d_outf); hipFree(g->d_outd);
  for (hipEvent_t e : g->ev_pool) hipEventDestroy(e);
  delete g;
  return WF_OK;
}

int wf_grad_config(wf_grad* g, double h, double lo, double hi, int strict, int max_eval_farms) {
  if (!g) return WF_E_INVALID;
  if (!std::isfinite(h) || !(h > 0.0)) return gfail(g, WF_E_INVALID, "the step h must be finite and positive (degrees)");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return gfail(g, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (g->h->N > 0 && max_eval_farms < 2 * g->h->N + 1) return gfail(g, WF_E_INVALID, kRowsMsg);
  g->step = h; g->lo = lo; g->hi = hi;
  g->strict = strict != 0; g->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_grad_set_timing(wf_grad* g, int detail) {
  if (!g) return WF_E_INVALID;
  g->detail = detail != 0;
  return WF_OK;
}

int wf_grad_run(wf_grad* g, const float* yaw, const float* cotangent, int n_farms, const int* farms, float* power,
                double* gradient, double* jacobian, int on_device) {
  if (!g) return WF_E_INVALID;
  wf_handle* h = g->h;
  if (h->N <= 0 || h->B <= 0) return gfail(g, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return gfail(g, WF_E_UNSUPPORTED, "yaw sensitivities serve a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return gfail(g, WF_E_UNSUPPORTED, "yaw sensitivities serve one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  if (h->wind_count == 0)
    return gfail(g, WF_E_INVALID, "no wind has been set: wf_set_wind (or wf_wind_*) must be called before wf_grad_run");
  if (farms) {
    if (n_farms < 1) return gfail(g, WF_E_INVALID, "n_farms must be >= 1");
    for (int k = 0; k < n_farms; ++k)
      if (farms[k] < 0 || farms[k] >= h->B) return gfail(g, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  } else {
    n_farms = h->B;
  }
  const int N = h->N, R = 2 * N + 1;
  if (g->max_eval < R) return gfail(g, WF_E_INVALID, kRowsMsg);
  WFG_ON_DEVICE(g);
  int C = g->max_eval / R;
  if (C > n_farms) C = n_farms;
  const int E = C * R;
  int rc = ensure_evaluator(g, E, g->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N, fnn = fn * N;
  const size_t n_in = (yaw ? fn : 0) + (cotangent ? fn : 0);
  const size_t n_outd = (gradient ? fn : 0) + (jacobian ? fnn : 0);
  rc = reserve(g, &g->d_yaw, &g->yaw_cap, en);
  if (rc == WF_OK) rc = reserve(g, &g->d_pow, &g->pow_cap, en);
  if (rc == WF_OK) rc = reserve(g, &g->d_wind, &g->wind_cap, 2 * (size_t)E);
  if (rc == WF_OK) rc = reserve(g, &g->d_div, &g->div_cap, (size_t)C * N);
  if (rc == WF_OK && farms) rc = reserve(g, &g->d_farms, &g->farms_cap, (size_t)n_farms);
  if (rc == WF_OK && !on_device && n_in) rc = reserve(g, &g->d_in, &g->in_cap, n_in);
  if (rc == WF_OK && !on_device && power) rc = reserve(g, &g->d_outf, &g->outf_cap, fn);
  if (rc == WF_OK && !on_device && n_outd) rc = reserve(g, &g->d_outd, &g->outd_cap, n_outd);
  if (rc != WF_OK) return rc;
  if (farms) {  // the farm list on the device (a previous upload may still read the host copy: drain first)
    WFG_HIP(g, hipStreamSynchronize(h->stream));
    g->farms.assign(farms, farms + n_farms);
    WFG_HIP(g, hipMemcpyAsync(g->d_farms, g->farms.data(), sizeof(int) * n_farms, hipMemcpyHostToDevice, h->stream));
  }
  const float *d_yaw_in = yaw, *d_cot = cotangent;
  if (!on_device) {
    if (yaw) {
      WFG_HIP(g, hipMemcpyAsync(g->d_in, yaw, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
      d_yaw_in = g->d_in;
    }
    if (cotangent) {
      float* dst = g->d_in + (yaw ? fn : 0);
      WFG_HIP(g, hipMemcpyAsync(dst, cotangent, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
      d_cot = dst;
    }
  }
  float* d_power = power ? (on_device ? power : g->d_outf) : nullptr;
  double* d_grad = gradient ? (on_device ? gradient : g->d_outd) : nullptr;
  double* d_jac = jacobian ? (on_device ? jacobian : g->d_outd + (gradient ? fn : 0)) : nullptr;
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool detail = g->detail != 0;
  g->n_ev = 0; g->timed = false;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const size_t off = (size_t)base * N;
    if (base == 0 || detail) { rc = record(g); if (rc != WF_OK) return rc; }  // (detail: four events per chunk)
    WfGradLayoutArgs la{};
    la.sl = WfGradSlots{farms ? g->d_farms : nullptr, base, n_slots, C};
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N;
    la.h = g->step; la.lo = g->lo; la.hi = g->hi;
    la.yaw_in = d_yaw_in ? d_yaw_in + off : nullptr; la.yaw = g->d_yaw;
    la.ews = g->d_wind; la.ewd = g->d_wind + E; la.d = g->d_div;
    WFG_HIP(g, wfk_launch_grad_layout(&la, h->stream));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
    WFG_EV(g, wf_set_wind_counts(g->ev, la.ews, E, la.ewd, E, 1));
    WFG_EV(g, wf_step(g->ev, g->d_yaw, g->d_pow, nullptr, nullptr, nullptr, 1));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
    WfGradReduceArgs ra{};
    ra.n_slots = n_slots; ra.N = N; ra.power_ev = g->d_pow; ra.d = g->d_div;
    ra.cot = d_cot ? d_cot + off : nullptr;
    ra.power = d_power ? d_power + off : nullptr;
    ra.gradient = d_grad ? d_grad + off : nullptr;
    ra.jacobian = d_jac ? d_jac + off * N : nullptr;
    WFG_HIP(g, wfk_launch_grad_reduce(&ra, h->stream));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
  }
  if (!detail) { rc = record(g); if (rc != WF_OK) return rc; }
  g->timed = true; g->timed_detail = detail;
  if (!on_device) {
    if (power) WFG_HIP(g, hipMemcpyAsync(power, g->d_outf, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    if (gradient) WFG_HIP(g, hipMemcpyAsync(gradient, g->d_outd, sizeof(double) * fn, hipMemcpyDeviceToHost, h->stream));
    if (jacobian) WFG_HIP(g, hipMemcpyAsync(jacobian, d_jac, sizeof(double) * fnn, hipMemcpyDeviceToHost, h->stream));
    WFG_HIP(g, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_grad_last_timing(wf_grad* g, float* total_ms, float* step_ms, float* glue_ms) {
  if (!g) return WF_E_INVALID;
  if (!g->timed || g->n_ev < 2) return gfail(g, WF_E_INVALID, "wf_grad_run has not run yet");
  WFG_ON_DEVICE(g);
  WFG_HIP(g, hipEventSynchronize(g->ev_pool[g->n_ev - 1]));
  float total = 0.0f, step = 0.0f, glue = 0.0f;
  WFG_HIP(g, hipEventElapsedTime(&total, g->ev_pool[0], g->ev_pool[g->n_ev - 1]));
  if (g->timed_detail) {  // per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
    for (size_t k = 1; k < g->n_ev; ++k) {
      float ms = 0.0f;
      WFG_HIP(g, hipEventElapsedTime(&ms, g->ev_pool[k - 1], g->ev_pool[k]));
      if (k % 4 == 2) step += ms;
      else glue += ms;
    }
  }
  if (total_ms) *total_ms = total;
  if (step_ms) *step_ms = step;
  if (glue_ms) *glue_ms = glue;
  return WF_OK;
}

wf_handle* wf_grad_evaluator(wf_grad* g) { return g ? g->ev : nullptr; }

int wf_grad_kernel_info(wf_grad* g, int* info) {
  if (!g || !info) return gfail(g, WF_E_INVALID, "wf_grad_kernel_info: NULL argument");
  WFG_ON_DEVICE(g);
  for (int k = 0; k < WF_GRAD_KERNELS; ++k) {
    hipFuncAttributes a{};
    WFG_HIP(g, wfk_grad_func_attributes(k, &a));
    info[3 * k] = a.numRegs; info[3 * k + 1] = (int)a.sharedSizeBytes; info[3 * k + 2] = (int)a.localSizeBytes;
  }
  return WF_OK;
}

const char* wf_grad_last_error(wf_grad* g) { return g ? g->err.c_str() : "wf_grad: NULL object"; }

}  // extern "C"
