// wf_yawopt_abi.hip — the C boundary of the yaw-optimiser extension (include/wfyawopt.h): an optimiser object that belongs
// to a parent handle, owns an evaluator handle and its device buffers, and enqueues a whole coordinate search on the parent's
// stream: per visit one glue kernel of wf_yawopt_kernels.hip and one wf_step on the evaluator.  Reads the parent (layout,
// model, wind, kernel choice, resolve mode); stores nothing in it.  The evaluator is configured through the public ABI of
// include/wfstep.h only.
#include "../../../include/wfyawopt.h"
#include "../wf_handle.h"
#include "wf_yawopt.h"

using namespace wfi;

struct wf_yawopt {
  wf_handle* h = nullptr;
  std::string err;
  // configuration
  double lo = -25.0, hi = 25.0;
  int P = 2, K[WF_YAWOPT_MAX_PASSES] = {5, 4, 0, 0};
  int strict = 0, max_eval = 65536;
  // the evaluator and what it was built from
  wf_handle* ev = nullptr;
  int ev_C = 0, ev_R = 0, ev_mode = -1;
  wf_model_params ev_model{};
  std::vector<double> ev_tws, ev_tct, ev_tcp, ev_lx, ev_ly;
  wf_kernel_choice ev_choice{};
  double ev_guard = 0.0;
  hipStream_t ev_stream = nullptr;
  // device buffers (grow-only)
  float *d_yaw = nullptr, *d_pow = nullptr, *d_best = nullptr;
  int* d_order = nullptr;
  double* d_wind = nullptr;  // [2][C R]
  size_t blk_cap = 0, pow_cap = 0, best_cap = 0, order_cap = 0, wind_cap = 0;
  int* d_farms = nullptr;
  size_t farms_cap = 0;
  std::vector<int> farms;  // host copy the upload reads from
  float *d_in = nullptr, *d_out = nullptr;  // staging for host callers: yaw0; yaw_opt, power_opt, power_init
  size_t in_cap = 0, out_cap = 0;
  // timing
  int detail = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t n_ev = 0;  // events the last run recorded: detail ? (glue, step)* boundaries : first and last
  bool timed = false, timed_detail = false;
};

namespace {

int ofail(wf_yawopt* o, int code, const std::string& msg) {
  if (o) o->err = msg;
  return code;
}
#define WFY_HIP(o, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return ofail(o, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFY_EV(o, call)                                                      \
  do {                                                                       \
    int rc_ = (call);                                                        \
    if (rc_ != WF_OK) return ofail(o, rc_, std::string("evaluator: ") + wf_last_error((o)->ev)); \
  } while (0)
#define WFY_ON_DEVICE(o)                 \
  DeviceGuard guard_((o)->h->device);    \
  if (guard_.err != hipSuccess) return ofail(o, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer (the stream is drained before a buffer in use is released)
template <class T>
int reserve(wf_yawopt* o, T** buf, size_t* cap, size_t n) {
  if (n <= *cap) return WF_OK;
  WFY_HIP(o, hipStreamSynchronize(o->h->stream));
  hipFree(*buf);
  *buf = nullptr; *cap = 0;
  WFY_HIP(o, hipMalloc(buf, sizeof(T) * n));
  *cap = n;
  return WF_OK;
}

int k_max(const wf_yawopt* o) {
  int k = 0;
  for (int p = 0; p < o->P; ++p) k = o->K[p] > k ? o->K[p] : k;
  return k;
}

bool same_model(const wf_model_params& a, const wf_model_params& b) {  // (the tables are compared through the handle's vectors)
  return std::memcmp(&a, &b, offsetof(wf_model_params, n_table)) == 0 && a.n_table == b.n_table &&
         a.enable_secondary_steering == b.enable_secondary_steering && a.enable_yaw_added_recovery == b.enable_yaw_added_recovery &&
         a.enable_transverse_velocities == b.enable_transverse_velocities;
}

// The evaluator: a handle with the parent's model, layout, kernel choice and guard band on the parent's device and stream,
// C x R farms.  Rebuilt when any of these, or the resolve mode asked for, differs from what it was built from.
int ensure_evaluator(wf_yawopt* o, int C, int R, int mode) {
  wf_handle* h = o->h;
  const size_t n = (size_t)h->N;
  const bool same = o->ev && o->ev_C == C && o->ev_R == R && same_model(o->ev_model, h->model) && o->ev_tws == h->tws &&
                    o->ev_tct == h->tct && o->ev_tcp == h->tcp && o->ev_lx.size() == n &&
                    std::equal(o->ev_lx.begin(), o->ev_lx.end(), h->lx.begin()) && std::equal(o->ev_ly.begin(), o->ev_ly.end(), h->ly.begin()) &&
                    std::memcmp(&o->ev_choice, &h->choice, sizeof(wf_kernel_choice)) == 0 && o->ev_guard == h->guard_rel;
  if (same) {
    if (o->ev_stream != h->stream) {
      WFY_EV(o, wf_set_stream(o->ev, (void*)h->stream, 1));
      o->ev_stream = h->stream;
    }
    if (o->ev_mode != mode) {
      WFY_EV(o, wf_set_risk_resolve(o->ev, mode));
      o->ev_mode = mode;
    }
    return WF_OK;
  }
  WFY_HIP(o, hipStreamSynchronize(h->stream));
  if (o->ev) wf_destroy(o->ev);
  o->ev = nullptr;
  wf_handle* ev = nullptr;
  if (wf_create(h->device, &ev) != WF_OK) return ofail(o, WF_E_HIP, std::string("evaluator: ") + wf_last_error(nullptr));
  o->ev = ev;
  wf_model_params m = h->model;
  m.table_ws = h->tws.data(); m.table_ct = h->tct.data(); m.table_cp = h->tcp.data();
  WFY_EV(o, wf_set_stream(ev, (void*)h->stream, 1));
  WFY_EV(o, wf_set_model(ev, &m));
  WFY_EV(o, wf_set_kernel_choice(ev, &h->choice));
  if (h->guard_user) WFY_EV(o, wf_set_risk_guard(ev, h->guard_rel));
  WFY_EV(o, wf_set_layout(ev, h->N, h->lx.data(), h->ly.data()));
  WFY_EV(o, wf_set_batch(ev, C * R));
  WFY_EV(o, wf_set_risk_resolve(ev, mode));
  o->ev_C = C; o->ev_R = R; o->ev_mode = mode; o->ev_stream = h->stream;
  o->ev_model = h->model; o->ev_tws = h->tws; o->ev_tct = h->tct; o->ev_tcp = h->tcp;
  o->ev_lx.assign(h->lx.begin(), h->lx.begin() + n); o->ev_ly.assign(h->ly.begin(), h->ly.begin() + n);
  o->ev_choice = h->choice; o->ev_guard = h->guard_rel;
  return WF_OK;
}

int record(wf_yawopt* o) {
  if (o->n_ev == o->ev_pool.size()) {
    hipEvent_t e = nullptr;
    WFY_HIP(o, hipEventCreate(&e));
    o->ev_pool.push_back(e);
  }
  WFY_HIP(o, hipEventRecord(o->ev_pool[o->n_ev++], o->h->stream));
  return WF_OK;
}

}  // namespace

extern "C" {

int wf_yawopt_create(wf_handle* h, wf_yawopt** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  wf_yawopt* o = new (std::nothrow) wf_yawopt();
  if (!o) return fail(h, WF_E_NOMEM, "out of host memory");
  o->h = h;
  *out = o;
  return WF_OK;
}

int wf_yawopt_destroy(wf_yawopt* o) {
  if (!o) return WF_OK;
  DeviceGuard guard(o->h->device);
  hipStreamSynchronize(o->h->stream);
  if (o->ev) wf_destroy(o->ev);
  hipFree(o->d_yaw); hipFree(o->d_pow); hipFree(o->d_best); hipFree(o->d_order); hipFree(o->d_wind); hipFree(o->d_farms);
  hipFree(o->d_in); hipFree(o->d_out);
  for (hipEvent_t e : o->ev_pool) hipEventDestroy(e);
  delete o;
  return WF_OK;
}

int wf_yawopt_config(wf_yawopt* o, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms) {
  if (!o || !K) return ofail(o, WF_E_INVALID, "wf_yawopt_config: NULL argument");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return ofail(o, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (n_passes < 1 || n_passes > WF_YAWOPT_MAX_PASSES) return ofail(o, WF_E_INVALID, "the number of passes must be in 1..4");
  if (K[0] < 2 || K[0] > WF_YAWOPT_MAX_K0) return ofail(o, WF_E_INVALID, "the first pass needs 2..31 candidates (K_0)");
  for (int p = 1; p < n_passes; ++p)
    if (K[p] < 1 || K[p] > WF_YAWOPT_MAX_K) return ofail(o, WF_E_INVALID, "a refining pass needs 1..15 candidates (K_p)");
  int km = 0;
  for (int p = 0; p < n_passes; ++p) km = K[p] > km ? K[p] : km;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (max_eval_farms < km + 1) return ofail(o, WF_E_INVALID, "max_eval_farms must hold one farm's candidates: at least K_max + 1");
  o->lo = lo; o->hi = hi; o->P = n_passes;
  for (int p = 0; p < WF_YAWOPT_MAX_PASSES; ++p) o->K[p] = p < n_passes ? K[p] : 0;
  o->strict = strict != 0; o->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_yawopt_set_timing(wf_yawopt* o, int detail) {
  if (!o) return WF_E_INVALID;
  o->detail = detail != 0;
  return WF_OK;
}

int wf_yawopt_run(wf_yawopt* o, const float* yaw0, int n_farms, const int* farms, float* yaw_opt, float* power_opt,
                  float* power_init, int on_device) {
  if (!o || !yaw_opt || !power_opt || !power_init) return ofail(o, WF_E_INVALID, "wf_yawopt_run: NULL argument");
  wf_handle* h = o->h;
  if (h->N <= 0 || h->B <= 0) return ofail(o, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return ofail(o, WF_E_UNSUPPORTED, "yaw optimisation serves a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return ofail(o, WF_E_UNSUPPORTED, "yaw optimisation serves one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  if (h->wind_count == 0) return ofail(o, WF_E_INVALID, "no wind has been set: wf_set_wind (or wf_wind_*) must be called before wf_yawopt_run");
  if (farms) {
    if (n_farms < 1) return ofail(o, WF_E_INVALID, "n_farms must be >= 1");
    for (int k = 0; k < n_farms; ++k)
      if (farms[k] < 0 || farms[k] >= h->B) return ofail(o, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  } else {
    n_farms = h->B;
  }
  WFY_ON_DEVICE(o);
  const int N = h->N, R = k_max(o) + 1;
  int C = o->max_eval / R;
  if (C > n_farms) C = n_farms;
  {
    int rc = ensure_evaluator(o, C, R, o->strict ? 2 : h->resolve_mode);
    if (rc != WF_OK) return rc;
  }
  const size_t blk = (size_t)C * R * N, fn = (size_t)n_farms * N;
  const bool per_farm = h->wind_count == h->B && h->B > 1;
  int rc = reserve(o, &o->d_yaw, &o->blk_cap, blk);
  if (rc == WF_OK) rc = reserve(o, &o->d_pow, &o->pow_cap, blk);
  if (rc == WF_OK) rc = reserve(o, &o->d_best, &o->best_cap, (size_t)C * N);
  if (rc == WF_OK) rc = reserve(o, &o->d_order, &o->order_cap, (size_t)C * N);
  if (rc == WF_OK && per_farm) rc = reserve(o, &o->d_wind, &o->wind_cap, 2 * (size_t)C * R);
  if (rc == WF_OK && farms) rc = reserve(o, &o->d_farms, &o->farms_cap, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw0) rc = reserve(o, &o->d_in, &o->in_cap, fn);
  if (rc == WF_OK && !on_device) rc = reserve(o, &o->d_out, &o->out_cap, fn + 2 * (size_t)n_farms);
  if (rc != WF_OK) return rc;
  if (farms) {
    WFY_HIP(o, hipStreamSynchronize(h->stream));  // (a previous upload may still read the host copy)
    o->farms.assign(farms, farms + n_farms);
    WFY_HIP(o, hipMemcpyAsync(o->d_farms, o->farms.data(), sizeof(int) * n_farms, hipMemcpyHostToDevice, h->stream));
  }
  const float* d_yaw0 = yaw0;
  if (yaw0 && !on_device) {
    WFY_HIP(o, hipMemcpyAsync(o->d_in, yaw0, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw0 = o->d_in;
  }
  float* d_oyaw = on_device ? yaw_opt : o->d_out;
  float* d_opow = on_device ? power_opt : o->d_out + fn;
  float* d_oini = on_device ? power_init : o->d_out + fn + n_farms;

  // the passes' grids (include/wfyawopt.h): h_0 = (hi - lo) / (K_0 - 1), h_p = 2 h_{p-1} / (K_p + 1)
  WfYawoptGrid grid[WF_YAWOPT_MAX_PASSES];
  {
    double hp = (o->hi - o->lo) / (double)(o->K[0] - 1);
    grid[0] = WfYawoptGrid{0, 0, o->K[0], o->lo, hp};
    for (int p = 1; p < o->P; ++p) {
      const double s = 2.0 * hp / (double)(o->K[p] + 1);
      grid[p] = WfYawoptGrid{0, 1, o->K[p], hp, s};
      hp = s;
    }
  }
  const WfYawoptGrid none{-1, 0, 0, 0.0, 0.0};
  const int V = o->P * N;  // visits
  o->n_ev = 0; o->timed = false;
  const bool detail = o->detail != 0;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfYawoptSlots sl{farms ? o->d_farms : nullptr, base, n_slots, C};
    if (base == 0 || detail) { rc = record(o); if (rc != WF_OK) return rc; }  // (detail: 2 V + 2 events per chunk)
    // the evaluator's wind: the parent's one wind as it is, or each farm's wind repeated over its rows
    if (!per_farm) {
      if (base == 0) WFY_EV(o, wf_set_wind_counts(o->ev, h->d_ws, 1, h->d_wd, 1, 1));
    } else {
      WfYawoptWindArgs wa{sl, h->d_ws, h->d_wd, R, o->d_wind, o->d_wind + (size_t)C * R};
      WFY_HIP(o, wfk_launch_yawopt_wind(&wa, h->stream));
      // (a parent whose farms share ONE direction keeps the shared geometry and the pair-table path on the evaluator too)
      if (h->shared_dir) WFY_EV(o, wf_set_wind_counts(o->ev, wa.ews, C * R, h->d_wd, 1, 1));
      else WFY_EV(o, wf_set_wind_counts(o->ev, wa.ews, C * R, wa.ewd, C * R, 1));
    }
    WfYawoptOrderArgs oa{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, per_farm ? 1 : 0, N, o->d_order};
    WFY_HIP(o, wfk_launch_yawopt_order(&oa, h->stream));
    WfYawoptAdvanceArgs aa{};
    aa.sl = sl; aa.N = N; aa.R = R; aa.lo = o->lo; aa.hi = o->hi;
    aa.order = o->d_order; aa.power = o->d_pow; aa.yaw = o->d_yaw; aa.best = o->d_best;
    aa.yaw0 = d_yaw0 ? d_yaw0 + (size_t)base * N : nullptr;
    aa.out_yaw = d_oyaw + (size_t)base * N; aa.out_power = d_opow + base; aa.out_init = d_oini + base;
    for (int v = 0; v <= V; ++v) {  // launch v lays out visit v (v < V) from the powers of visit v - 1 (v > 0)
      aa.prev = none; aa.next = none;
      if (v > 0) { aa.prev = grid[(v - 1) / N]; aa.prev.s = (v - 1) % N; }
      if (v < V) { aa.next = grid[v / N]; aa.next.s = v % N; }
      aa.first = v == 1;
      WFY_HIP(o, wfk_launch_yawopt_advance(&aa, h->stream));
      if (detail) { rc = record(o); if (rc != WF_OK) return rc; }
      if (v < V) {
        WFY_EV(o, wf_step(o->ev, o->d_yaw, o->d_pow, nullptr, nullptr, nullptr, 1));
        if (detail) { rc = record(o); if (rc != WF_OK) return rc; }
      }
    }
  }
  if (!detail) { rc = record(o); if (rc != WF_OK) return rc; }
  o->timed = true; o->timed_detail = detail;
  if (!on_device) {
    WFY_HIP(o, hipMemcpyAsync(yaw_opt, o->d_out, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    WFY_HIP(o, hipMemcpyAsync(power_opt, o->d_out + fn, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFY_HIP(o, hipMemcpyAsync(power_init, o->d_out + fn + n_farms, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFY_HIP(o, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_yawopt_last_timing(wf_yawopt* o, float* total_ms, float* step_ms, float* glue_ms) {
  if (!o) return WF_E_INVALID;
  if (!o->timed || o->n_ev < 2) return ofail(o, WF_E_INVALID, "wf_yawopt_run has not run yet");
  WFY_ON_DEVICE(o);
  WFY_HIP(o, hipEventSynchronize(o->ev_pool[o->n_ev - 1]));
  float total = 0.0f, step = 0.0f, glue = 0.0f;
  WFY_HIP(o, hipEventElapsedTime(&total, o->ev_pool[0], o->ev_pool[o->n_ev - 1]));
  if (o->timed_detail) {
    // per chunk the events are e0 | glue e | step e | glue e | ... | glue e: V + 1 glue intervals (the first one holds the
    // chunk's wind and order kernels too) and V step intervals, then the next chunk's e0 (an empty interval)
    const int V = o->P * o->h->N;
    const size_t per_chunk = 2 * (size_t)V + 2;
    for (size_t k = 1; k < o->n_ev; ++k) {
      float ms = 0.0f;
      WFY_HIP(o, hipEventElapsedTime(&ms, o->ev_pool[k - 1], o->ev_pool[k]));
      const size_t r = k % per_chunk;
      if (r != 0 && r % 2 == 0) step += ms;
      else glue += ms;
    }
  }
  if (total_ms) *total_ms = total;
  if (step_ms) *step_ms = step;
  if (glue_ms) *glue_ms = glue;
  return WF_OK;
}

wf_handle* wf_yawopt_evaluator(wf_yawopt* o) { return o ? o->ev : nullptr; }

const char* wf_yawopt_last_error(wf_yawopt* o) { return o ? o->err.c_str() : "wf_yawopt: NULL optimiser"; }

}  // extern "C"
