// wf_rose_abi.hip — the C boundary of the rose extension (include/wfrose.h): an object that belongs to a parent handle,
// owns yaw tables, a rose, an evaluator handle and its device buffers, and enqueues a whole expected-power evaluation on the
// parent's stream: per chunk one lay-out kernel, wf_set_wind_counts + wf_step on the evaluator, two reducing kernels
// (wf_rose_kernels.hip).  Reads the parent (layout, model, wind, env parameters and yaw state, kernel choice, resolve
// mode); stores nothing in it.  The evaluator follows the idea of ensure_evaluator in yawopt/wf_yawopt_abi.hip — a second
// handle configured through the public ABI of include/wfstep.h only — and shares no state with it.
#include "../../../include/wfrose.h"
#include "../wf_handle.h"
#include "wf_rose.h"

using namespace wfi;

struct wf_rose {
  wf_handle* h = nullptr;
  std::string err;
  int strict = 0, max_eval = 65536;
  // yaw tables
  struct Slot {
    double *d_twd = nullptr, *d_tws = nullptr;
    float* d_T = nullptr;
    size_t twd_cap = 0, tws_cap = 0, T_cap = 0;
    int Dt = 0, St = 0, N = 0, interp = 0;  // Dt == 0: empty
  } slot[WF_ROSE_SLOTS];
  // the rose
  int D = 0, S = 0;
  double cut_in = 0.001, cut_out = 0.0;
  double *d_wd = nullptr, *d_ws = nullptr, *d_freq = nullptr;
  size_t wd_cap = 0, ws_cap = 0, freq_cap = 0;
  // the evaluator and what it was built from
  wf_handle* ev = nullptr;
  int ev_E = 0, ev_mode = -1;
  wf_model_params ev_model{};
  std::vector<double> ev_tws, ev_tct, ev_tcp, ev_lx, ev_ly;
  wf_kernel_choice ev_choice{};
  double ev_guard = 0.0;
  hipStream_t ev_stream = nullptr;
  // device buffers (grow-only)
  double *d_ews = nullptr, *d_ewd = nullptr, *d_rowsum = nullptr;  // [E]
  float *d_yaw = nullptr, *d_pow = nullptr;                       // [E][N]
  double* d_acc = nullptr;                                        // [C][N] then [C]
  int* d_cases = nullptr;                                         // [2][C]
  float *d_fixed = nullptr, *d_cond = nullptr;                    // staging for host callers
  float* d_pol = nullptr;                                         // staging of wf_rose_policy: target, action
  size_t ews_cap = 0, ewd_cap = 0, rowsum_cap = 0, yaw_cap = 0, pow_cap = 0, acc_cap = 0, cases_cap = 0, fixed_cap = 0, cond_cap = 0,
         pol_cap = 0;
  std::vector<int> cases;  // host copy the upload reads from: [2][C]
  // timing: four events per chunk (start | lay-out | wind + step | reduce)
  std::vector<hipEvent_t> ev_pool;
  size_t n_ev = 0;
  bool timed = false;
};

namespace {

int rfail(wf_rose* r, int code, const std::string& msg) {
  if (r) r->err = msg;
  return code;
}
#define WFR_HIP(r, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return rfail(r, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFR_EV(r, call)                                                      \
  do {                                                                       \
    int rc_ = (call);                                                        \
    if (rc_ != WF_OK) return rfail(r, rc_, std::string("evaluator: ") + wf_last_error((r)->ev)); \
  } while (0)
#define WFR_ON_DEVICE(r)                 \
  DeviceGuard guard_((r)->h->device);    \
  if (guard_.err != hipSuccess) return rfail(r, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer (the stream is drained before a buffer in use is released)
template <class T>
int reserve(wf_rose* r, T** buf, size_t* cap, size_t n) {
  if (n <= *cap) return WF_OK;
  WFR_HIP(r, hipStreamSynchronize(r->h->stream));
  hipFree(*buf);
  *buf = nullptr; *cap = 0;
  WFR_HIP(r, hipMalloc(buf, sizeof(T) * n));
  *cap = n;
  return WF_OK;
}

int check_parent(wf_rose* r, const char* what) {
  wf_handle* h = r->h;
  if (h->N <= 0 || h->B <= 0) return rfail(r, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return rfail(r, WF_E_UNSUPPORTED, std::string(what) + " serves a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return rfail(r, WF_E_UNSUPPORTED, std::string(what) + " serves one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  return WF_OK;
}

bool same_model(const wf_model_params& a, const wf_model_params& b) {  // (the tables are compared through the handle's vectors)
  return std::memcmp(&a, &b, offsetof(wf_model_params, n_table)) == 0 && a.n_table == b.n_table &&
         a.enable_secondary_steering == b.enable_secondary_steering && a.enable_yaw_added_recovery == b.enable_yaw_added_recovery &&
         a.enable_transverse_velocities == b.enable_transverse_velocities;
}

// The evaluator: a handle with the parent's model, layout, kernel choice and guard band on the parent's device and stream,
// E farms.  Rebuilt when any of these differs from what it was built from; the resolve mode and the stream are just set.
int ensure_evaluator(wf_rose* r, int E, int mode) {
  wf_handle* h = r->h;
  const size_t n = (size_t)h->N;
  const bool same = r->ev && r->ev_E == E && same_model(r->ev_model, h->model) && r->ev_tws == h->tws && r->ev_tct == h->tct &&
                    r->ev_tcp == h->tcp && r->ev_lx.size() == n && std::equal(r->ev_lx.begin(), r->ev_lx.end(), h->lx.begin()) &&
                    std::equal(r->ev_ly.begin(), r->ev_ly.end(), h->ly.begin()) &&
                    std::memcmp(&r->ev_choice, &h->choice, sizeof(wf_kernel_choice)) == 0 && r->ev_guard == h->guard_rel;
  if (same) {
    if (r->ev_stream != h->stream) {
      WFR_EV(r, wf_set_stream(r->ev, (void*)h->stream, 1));
      r->ev_stream = h->stream;
    }
    if (r->ev_mode != mode) {
      WFR_EV(r, wf_set_risk_resolve(r->ev, mode));
      r->ev_mode = mode;
    }
    return WF_OK;
  }
  WFR_HIP(r, hipStreamSynchronize(h->stream));
  if (r->ev) wf_destroy(r->ev);
  r->ev = nullptr;
  wf_handle* ev = nullptr;
  if (wf_create(h->device, &ev) != WF_OK) return rfail(r, WF_E_HIP, std::string("evaluator: ") + wf_last_error(nullptr));
  r->ev = ev;
  wf_model_params m = h->model;
  m.table_ws = h->tws.data(); m.table_ct = h->tct.data(); m.table_cp = h->tcp.data();
  WFR_EV(r, wf_set_stream(ev, (void*)h->stream, 1));
  WFR_EV(r, wf_set_model(ev, &m));
  WFR_EV(r, wf_set_kernel_choice(ev, &h->choice));
  if (h->guard_user) WFR_EV(r, wf_set_risk_guard(ev, h->guard_rel));
  WFR_EV(r, wf_set_layout(ev, h->N, h->lx.data(), h->ly.data()));
  WFR_EV(r, wf_set_batch(ev, E));
  WFR_EV(r, wf_set_risk_resolve(ev, mode));
  r->ev_E = E; r->ev_mode = mode; r->ev_stream = h->stream;
  r->ev_model = h->model; r->ev_tws = h->tws; r->ev_tct = h->tct; r->ev_tcp = h->tcp;
  r->ev_lx.assign(h->lx.begin(), h->lx.begin() + n); r->ev_ly.assign(h->ly.begin(), h->ly.begin() + n);
  r->ev_choice = h->choice; r->ev_guard = h->guard_rel;
  return WF_OK;
}

int record(wf_rose* r) {
  if (r->n_ev == r->ev_pool.size()) {
    hipEvent_t e = nullptr;
    WFR_HIP(r, hipEventCreate(&e));
    r->ev_pool.push_back(e);
  }
  WFR_HIP(r, hipEventRecord(r->ev_pool[r->n_ev++], r->h->stream));
  return WF_OK;
}

WfRoseTable device_table(const wf_rose::Slot& s) {
  return WfRoseTable{s.d_twd, s.d_tws, s.Dt > 0 ? s.d_T : nullptr, s.Dt, s.St, s.interp};
}

}  // namespace

extern "C" {

int wf_rose_create(wf_handle* h, wf_rose** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  wf_rose* r = new (std::nothrow) wf_rose();
  if (!r) return fail(h, WF_E_NOMEM, "out of host memory");
  r->h = h;
  *out = r;
  return WF_OK;
}

int wf_rose_destroy(wf_rose* r) {
  if (!r) return WF_OK;
  DeviceGuard guard(r->h->device);
  hipStreamSynchronize(r->h->stream);
  if (r->ev) wf_destroy(r->ev);
  for (auto& s : r->slot) { hipFree(s.d_twd); hipFree(s.d_tws); hipFree(s.d_T); }
  hipFree(r->d_wd); hipFree(r->d_ws); hipFree(r->d_freq);
  hipFree(r->d_ews); hipFree(r->d_ewd); hipFree(r->d_rowsum); hipFree(r->d_yaw); hipFree(r->d_pow); hipFree(r->d_acc);
  hipFree(r->d_cases); hipFree(r->d_fixed); hipFree(r->d_cond); hipFree(r->d_pol);
  for (hipEvent_t e : r->ev_pool) hipEventDestroy(e);
  delete r;
  return WF_OK;
}

int wf_rose_set_table(wf_rose* r, int slot, int Dt, const double* twd, int St, const double* tws, const float* T, int interp,
                      int on_device) {
  if (!r || !twd || !tws || !T) return rfail(r, WF_E_INVALID, "wf_rose_set_table: NULL argument");
  if (slot < 0 || slot >= WF_ROSE_SLOTS) return rfail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
  if (Dt < 1 || St < 1) return rfail(r, WF_E_INVALID, "a yaw table needs at least one direction and one speed node");
  if (interp != WF_ROSE_LINEAR && interp != WF_ROSE_NEAREST) return rfail(r, WF_E_INVALID, "interp must be WF_ROSE_LINEAR (0) or WF_ROSE_NEAREST (1)");
  wf_handle* h = r->h;
  if (h->N <= 0) return rfail(r, WF_E_INVALID, "no layout: wf_set_layout comes first");
  const size_t nT = (size_t)Dt * St * h->N;
  if (nT > ((size_t)1 << 30)) return rfail(r, WF_E_INVALID, "the yaw table is too large");
  if (!on_device) {
    for (int i = 0; i < Dt; ++i)
      if (!(twd[i] >= 0.0) || !(twd[i] < 360.0) || (i > 0 && !(twd[i] > twd[i - 1])))
        return rfail(r, WF_E_INVALID, "table direction axis must be strictly ascending inside [0, 360)");
    for (int i = 0; i < St; ++i)
      if (!(tws[i] > 0.0) || !std::isfinite(tws[i]) || (i > 0 && !(tws[i] > tws[i - 1])))
        return rfail(r, WF_E_INVALID, "table speed axis must be strictly ascending and > 0");
    for (size_t i = 0; i < nT; ++i)
      if (!std::isfinite(T[i])) return rfail(r, WF_E_INVALID, "table yaw values must be finite");
  }
  WFR_ON_DEVICE(r);
  wf_rose::Slot& s = r->slot[slot];
  int rc = reserve(r, &s.d_twd, &s.twd_cap, (size_t)Dt);
  if (rc == WF_OK) rc = reserve(r, &s.d_tws, &s.tws_cap, (size_t)St);
  if (rc == WF_OK) rc = reserve(r, &s.d_T, &s.T_cap, nT);
  if (rc != WF_OK) { s.Dt = 0; return rc; }
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  s.Dt = 0;
  WFR_HIP(r, hipMemcpyAsync(s.d_twd, twd, sizeof(double) * Dt, kind, h->stream));
  WFR_HIP(r, hipMemcpyAsync(s.d_tws, tws, sizeof(double) * St, kind, h->stream));
  WFR_HIP(r, hipMemcpyAsync(s.d_T, T, sizeof(float) * nT, kind, h->stream));
  if (!on_device) WFR_HIP(r, hipStreamSynchronize(h->stream));  // caller's host arrays may go away
  s.Dt = Dt; s.St = St; s.N = h->N; s.interp = interp;
  return WF_OK;
}

int wf_rose_set_rose(wf_rose* r, int D, const double* wd, int S, const double* ws, const double* freq, double cut_in,
                     double cut_out) {
  if (!r || !wd || !ws || !freq) return rfail(r, WF_E_INVALID, "wf_rose_set_rose: NULL argument");
  if (D < 1 || S < 1) return rfail(r, WF_E_INVALID, "a rose needs at least one direction and one speed");
  if ((size_t)D * S > ((size_t)1 << 24)) return rfail(r, WF_E_INVALID, "the rose is too large (more than 2^24 conditions)");
  if (std::isnan(cut_in) || std::isnan(cut_out)) return rfail(r, WF_E_INVALID, "cut_in / cut_out must not be NaN");
  for (int i = 0; i < D; ++i)
    if (!std::isfinite(wd[i])) return rfail(r, WF_E_INVALID, "rose wind directions must be finite");
  for (int i = 0; i < S; ++i)
    if (!(ws[i] > 0.0) || !std::isfinite(ws[i])) return rfail(r, WF_E_INVALID, "rose wind speeds must be > 0");
  for (size_t i = 0; i < (size_t)D * S; ++i)
    if (!std::isfinite(freq[i]) || !(freq[i] >= 0.0)) return rfail(r, WF_E_INVALID, "rose frequencies must be finite and >= 0");
  WFR_ON_DEVICE(r);
  r->D = 0;
  int rc = reserve(r, &r->d_wd, &r->wd_cap, (size_t)D);
  if (rc == WF_OK) rc = reserve(r, &r->d_ws, &r->ws_cap, (size_t)S);
  if (rc == WF_OK) rc = reserve(r, &r->d_freq, &r->freq_cap, (size_t)D * S);
  if (rc != WF_OK) return rc;
  hipStream_t st = r->h->stream;
  WFR_HIP(r, hipMemcpyAsync(r->d_wd, wd, sizeof(double) * D, hipMemcpyHostToDevice, st));
  WFR_HIP(r, hipMemcpyAsync(r->d_ws, ws, sizeof(double) * S, hipMemcpyHostToDevice, st));
  WFR_HIP(r, hipMemcpyAsync(r->d_freq, freq, sizeof(double) * D * S, hipMemcpyHostToDevice, st));
  WFR_HIP(r, hipStreamSynchronize(st));
  r->D = D; r->S = S; r->cut_in = cut_in; r->cut_out = cut_out;
  return WF_OK;
}

int wf_rose_config(wf_rose* r, int strict, int max_eval_farms) {
  if (!r) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  r->strict = strict != 0;
  r->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_rose_evaluate(wf_rose* r, int n_cases, const int* case_kind, const int* case_arg, const float* fixed_yaw,
                     double* weighted_power, double* weighted_turbine_power, float* condition_power, int on_device) {
  if (!r || !case_kind || !case_arg) return rfail(r, WF_E_INVALID, "wf_rose_evaluate: NULL argument");
  wf_handle* h = r->h;
  int rc = check_parent(r, "a rose evaluation");
  if (rc != WF_OK) return rc;
  if (r->D <= 0) return rfail(r, WF_E_INVALID, "no rose: wf_rose_set_rose comes first");
  if (n_cases < 1 || n_cases > WF_ROSE_MAX_CASES) return rfail(r, WF_E_INVALID, "the number of cases must be in 1..64");
  const int N = h->N, C = n_cases, D = r->D, S = r->S;
  int n_fixed = 0;
  for (int c = 0; c < C; ++c) {
    const int kind = case_kind[c], arg = case_arg[c];
    if (kind == WF_ROSE_CASE_ZERO) continue;
    if (kind == WF_ROSE_CASE_FIXED) {
      if (arg < 0 || arg >= 65536) return rfail(r, WF_E_INVALID, "a fixed case names a row of fixed_yaw: 0 .. 65535");
      if (!fixed_yaw) return rfail(r, WF_E_INVALID, "a fixed case needs fixed_yaw");
      n_fixed = arg + 1 > n_fixed ? arg + 1 : n_fixed;
    } else if (kind == WF_ROSE_CASE_TABLE) {
      if (arg < 0 || arg >= WF_ROSE_SLOTS) return rfail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
      if (r->slot[arg].Dt <= 0) return rfail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
      if (r->slot[arg].N != N) return rfail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
    } else {
      return rfail(r, WF_E_INVALID, "unknown case kind (WF_ROSE_CASE_ZERO / _FIXED / _TABLE)");
    }
  }
  const long long rows = (long long)D * C * S;
  if (rows > (1LL << 30) / (N + 1)) return rfail(r, WF_E_INVALID, "too many rows: directions x cases x speeds x turbines must stay below 2^30");
  WFR_ON_DEVICE(r);
  const int R = (int)rows;
  const int E = R < r->max_eval ? R : r->max_eval;
  rc = ensure_evaluator(r, E, r->strict ? 2 : h->resolve_mode);
  if (rc != WF_OK) return rc;
  const size_t en = (size_t)E * N, cn = (size_t)C * N, cds = (size_t)C * D * S;
  rc = reserve(r, &r->d_ews, &r->ews_cap, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_ewd, &r->ewd_cap, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_rowsum, &r->rowsum_cap, (size_t)E);
  if (rc == WF_OK) rc = reserve(r, &r->d_yaw, &r->yaw_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_pow, &r->pow_cap, en);
  if (rc == WF_OK) rc = reserve(r, &r->d_acc, &r->acc_cap, cn + C);
  if (rc == WF_OK) rc = reserve(r, &r->d_cases, &r->cases_cap, 2 * (size_t)C);
  if (rc == WF_OK && !on_device && n_fixed) rc = reserve(r, &r->d_fixed, &r->fixed_cap, (size_t)n_fixed * N);
  if (rc == WF_OK && !on_device && condition_power) rc = reserve(r, &r->d_cond, &r->cond_cap, cds);
  if (rc != WF_OK) return rc;
  {  // the case list: uploaded when it differs from the one the device holds
    std::vector<int> cs(2 * (size_t)C);
    for (int c = 0; c < C; ++c) { cs[c] = case_kind[c]; cs[C + c] = case_arg[c]; }
    if (cs != r->cases) {
      WFR_HIP(r, hipStreamSynchronize(h->stream));  // (a previous upload may still read the host copy)
      r->cases.swap(cs);
      WFR_HIP(r, hipMemcpyAsync(r->d_cases, r->cases.data(), sizeof(int) * 2 * C, hipMemcpyHostToDevice, h->stream));
    }
  }
  const float* d_fixed = fixed_yaw;
  if (!on_device && n_fixed) {
    WFR_HIP(r, hipMemcpyAsync(r->d_fixed, fixed_yaw, sizeof(float) * n_fixed * N, hipMemcpyHostToDevice, h->stream));
    d_fixed = r->d_fixed;
  }
  WfRoseLayoutArgs la{};
  la.wd = r->d_wd; la.ws = r->d_ws; la.cases = r->d_cases; la.fixed_yaw = n_fixed ? d_fixed : nullptr;
  for (int i = 0; i < WF_ROSE_SLOTS; ++i) la.tab[i] = device_table(r->slot[i]);
  la.ews = r->d_ews; la.ewd = r->d_ewd; la.yaw = r->d_yaw;
  WfRoseReduceArgs ra{};
  ra.ws = r->d_ws; ra.freq = r->d_freq; ra.cut_in = r->cut_in; ra.cut_out = r->cut_out;
  ra.power = r->d_pow; ra.rowsum = r->d_rowsum;
  ra.condition_power = condition_power ? (on_device ? condition_power : r->d_cond) : nullptr;
  ra.acc_turbine = r->d_acc; ra.acc_farm = r->d_acc + cn;
  r->n_ev = 0; r->timed = false;
  for (int row0 = 0; row0 < R; row0 += E) {
    const WfRoseShape sh{D, C, S, N, row0, R - row0 < E ? R - row0 : E, E};
    la.sh = sh; ra.sh = sh; ra.first = row0 == 0;
    if ((rc = record(r)) != WF_OK) return rc;
    WFR_HIP(r, wfk_launch_rose_layout(&la, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
    WFR_EV(r, wf_set_wind_counts(r->ev, r->d_ews, E, r->d_ewd, E, 1));
    WFR_EV(r, wf_step(r->ev, r->d_yaw, r->d_pow, nullptr, nullptr, nullptr, 1));
    if ((rc = record(r)) != WF_OK) return rc;
    WFR_HIP(r, wfk_launch_rose_rowsum(&ra, h->stream));
    WFR_HIP(r, wfk_launch_rose_accumulate(&ra, h->stream));
    if ((rc = record(r)) != WF_OK) return rc;
  }
  r->timed = true;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (weighted_power) WFR_HIP(r, hipMemcpyAsync(weighted_power, r->d_acc + cn, sizeof(double) * C, kind, h->stream));
  if (weighted_turbine_power) WFR_HIP(r, hipMemcpyAsync(weighted_turbine_power, r->d_acc, sizeof(double) * cn, kind, h->stream));
  if (!on_device) {
    if (condition_power) WFR_HIP(r, hipMemcpyAsync(condition_power, r->d_cond, sizeof(float) * cds, hipMemcpyDeviceToHost, h->stream));
    WFR_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_rose_policy(wf_rose* r, int slot, float* target_yaw, float* action, int on_device) {
  if (!r) return WF_E_INVALID;
  if (!target_yaw && !action) return rfail(r, WF_E_INVALID, "wf_rose_policy: NULL argument");
  wf_handle* h = r->h;
  int rc = check_parent(r, "a yaw look-up-table policy");
  if (rc != WF_OK) return rc;
  if (slot < 0 || slot >= WF_ROSE_SLOTS) return rfail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
  if (r->slot[slot].Dt <= 0) return rfail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
  if (r->slot[slot].N != h->N) return rfail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
  if (h->wind_count == 0) return rfail(r, WF_E_INVALID, "no wind has been set: wf_set_wind (or wf_wind_*) must be called before wf_rose_policy");
  if (!h->d_env_yaw) return rfail(r, WF_E_INVALID, "no env state: wf_env_config and wf_env_reset come first");
  WFR_ON_DEVICE(r);
  const size_t bn = (size_t)h->B * h->N;
  if (!on_device && (rc = reserve(r, &r->d_pol, &r->pol_cap, 2 * bn)) != WF_OK) return rc;
  WfRosePolicyArgs pa{};
  pa.tab = device_table(r->slot[slot]);
  pa.B = h->B; pa.N = h->N; pa.wind_stride = h->wind_count == h->B ? 1 : 0;
  pa.ws = h->d_ws; pa.wd = h->d_wd; pa.yaw_state = h->d_env_yaw;
  pa.lo = h->env.yaw_lo; pa.hi = h->env.yaw_hi; pa.step = h->env.yaw_step; pa.discrete = h->env.discrete;
  pa.target = target_yaw ? (on_device ? target_yaw : r->d_pol) : nullptr;
  pa.action = action ? (on_device ? action : r->d_pol + bn) : nullptr;
  WFR_HIP(r, wfk_launch_rose_policy(&pa, h->stream));
  if (!on_device) {
    if (target_yaw) WFR_HIP(r, hipMemcpyAsync(target_yaw, r->d_pol, sizeof(float) * bn, hipMemcpyDeviceToHost, h->stream));
    if (action) WFR_HIP(r, hipMemcpyAsync(action, r->d_pol + bn, sizeof(float) * bn, hipMemcpyDeviceToHost, h->stream));
    WFR_HIP(r, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_rose_last_timing(wf_rose* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  if (!r->timed || r->n_ev < 4) return rfail(r, WF_E_INVALID, "wf_rose_evaluate has not run yet");
  WFR_ON_DEVICE(r);
  WFR_HIP(r, hipEventSynchronize(r->ev_pool[r->n_ev - 1]));
  float total = 0.0f, step = 0.0f, glue = 0.0f;
  WFR_HIP(r, hipEventElapsedTime(&total, r->ev_pool[0], r->ev_pool[r->n_ev - 1]));
  for (size_t k = 1; k < r->n_ev; ++k) {  // per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
    float ms = 0.0f;
    WFR_HIP(r, hipEventElapsedTime(&ms, r->ev_pool[k - 1], r->ev_pool[k]));
    if (k % 4 == 2) step += ms;
    else glue += ms;
  }
  if (total_ms) *total_ms = total;
  if (step_ms) *step_ms = step;
  if (glue_ms) *glue_ms = glue;
  return WF_OK;
}

int wf_rose_kernel_info(wf_rose* r, int* info) {
  if (!r || !info) return rfail(r, WF_E_INVALID, "wf_rose_kernel_info: NULL argument");
  WFR_ON_DEVICE(r);
  for (int k = 0; k < WF_ROSE_KERNELS; ++k) {
    hipFuncAttributes a{};
    WFR_HIP(r, wfk_rose_func_attributes(k, &a));
    info[3 * k] = a.numRegs; info[3 * k + 1] = (int)a.sharedSizeBytes; info[3 * k + 2] = (int)a.localSizeBytes;
  }
  return WF_OK;
}

const char* wf_rose_last_error(wf_rose* r) { return r ? r->err.c_str() : "wf_rose: NULL object"; }

}  // extern "C"
