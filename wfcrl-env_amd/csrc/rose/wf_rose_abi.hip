// wf_rose_abi.hip — the C boundary of the rose extension (include/wfrose.h): an object that belongs to a parent handle,
// owns yaw tables, a rose, an evaluator handle and its device buffers, and enqueues a whole expected-power evaluation on the
// parent's stream.  The run is the extensions' shared row driver's (ext/wf_ext.h: run_rows — chunks, the evaluator and its
// step, events), an item being one row: a (direction, case, speed); this file supplies the checks of the cases, their
// upload, a chunk's lay-out kernel and two reducing kernels (wf_rose_kernels.hip) and the copy of the sums.  Reads the
// parent (layout, model, wind, env parameters and yaw state, kernel choice, resolve mode); stores nothing in it.
#include "../../../include/wfrose.h"
#include "../ext/wf_ext.h"
#include "wf_rose.h"

using namespace wfi;

struct wf_rose : ext_base {
  int strict = 0, max_eval = 65536;
  // yaw tables
  struct Slot {
    dev_buf<double> d_twd, d_tws;
    dev_buf<float> d_T;
    int Dt = 0, St = 0, N = 0, interp = 0;  // Dt == 0: empty
  } slot[WF_ROSE_SLOTS];
  // the rose
  int D = 0, S = 0;
  double cut_in = 0.001, cut_out = 0.0;
  dev_buf<double> d_wd, d_ws, d_freq;
  // device buffers (grow-only)
  row_batch rows;            // E rows
  dev_buf<double> d_rowsum;  // [E]
  dev_buf<double> d_acc;     // [C][N] then [C]
  dev_buf<int> d_cases;      // [2][C]
  dev_buf<char> d_stage;     // staging for host callers: fixed_yaw, condition_power; wf_rose_policy's target, action
  std::vector<int> cases;  // host copy the upload reads from: [2][C]
  evaluator eval;  // timing: four events per chunk (start | lay-out | wind + step | reduce)
};

namespace {

WfRoseTable device_table(const wf_rose::Slot& s) {
  return WfRoseTable{s.d_twd, s.d_tws, s.Dt > 0 ? s.d_T.p : nullptr, s.Dt, s.St, s.interp};
}

}  // namespace

namespace wfi {

WfRoseTable rose_device_table(const wf_rose* r, int slot, int* N) {
  const wf_rose::Slot& s = r->slot[slot];
  if (N) *N = s.N;
  return device_table(s);
}

wf_handle* rose_parent(const wf_rose* r) { return r->h; }

}  // namespace wfi

extern "C" {

int wf_rose_create(wf_handle* h, wf_rose** out) { return ext_create(h, out); }

int wf_rose_destroy(wf_rose* r) { return ext_destroy(r); }

int wf_rose_set_table(wf_rose* r, int slot, int Dt, const double* twd, int St, const double* tws, const float* T, int interp,
                      int on_device) {
  if (!r || !twd || !tws || !T) return ext_fail(r, WF_E_INVALID, "wf_rose_set_table: NULL argument");
  if (slot < 0 || slot >= WF_ROSE_SLOTS) return ext_fail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
  if (Dt < 1 || St < 1) return ext_fail(r, WF_E_INVALID, "a yaw table needs at least one direction and one speed node");
  if (interp != WF_ROSE_LINEAR && interp != WF_ROSE_NEAREST) return ext_fail(r, WF_E_INVALID, "interp must be WF_ROSE_LINEAR (0) or WF_ROSE_NEAREST (1)");
  wf_handle* h = r->h;
  if (h->N <= 0) return ext_fail(r, WF_E_INVALID, "no layout: wf_set_layout comes first");
  const size_t nT = (size_t)Dt * St * h->N;
  if (nT > ((size_t)1 << 30)) return ext_fail(r, WF_E_INVALID, "the yaw table is too large");
  if (!on_device) {
    for (int i = 0; i < Dt; ++i)
      if (!(twd[i] >= 0.0) || !(twd[i] < 360.0) || (i > 0 && !(twd[i] > twd[i - 1])))
        return ext_fail(r, WF_E_INVALID, "table direction axis must be strictly ascending inside [0, 360)");
    for (int i = 0; i < St; ++i)
      if (!(tws[i] > 0.0) || !std::isfinite(tws[i]) || (i > 0 && !(tws[i] > tws[i - 1])))
        return ext_fail(r, WF_E_INVALID, "table speed axis must be strictly ascending and > 0");
    for (size_t i = 0; i < nT; ++i)
      if (!std::isfinite(T[i])) return ext_fail(r, WF_E_INVALID, "table yaw values must be finite");
  }
  WFX_ON_DEVICE(r);
  wf_rose::Slot& s = r->slot[slot];
  int rc = reserve(r, s.d_twd, (size_t)Dt);
  if (rc == WF_OK) rc = reserve(r, s.d_tws, (size_t)St);
  if (rc == WF_OK) rc = reserve(r, s.d_T, nT);
  if (rc != WF_OK) { s.Dt = 0; return rc; }
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  s.Dt = 0;
  WFX_HIP(r, hipMemcpyAsync(s.d_twd, twd, sizeof(double) * Dt, kind, h->stream));
  WFX_HIP(r, hipMemcpyAsync(s.d_tws, tws, sizeof(double) * St, kind, h->stream));
  WFX_HIP(r, hipMemcpyAsync(s.d_T, T, sizeof(float) * nT, kind, h->stream));
  if (!on_device) WFX_HIP(r, hipStreamSynchronize(h->stream));  // caller's host arrays may go away
  s.Dt = Dt; s.St = St; s.N = h->N; s.interp = interp;
  return WF_OK;
}

int wf_rose_set_rose(wf_rose* r, int D, const double* wd, int S, const double* ws, const double* freq, double cut_in,
                     double cut_out) {
  if (!r || !wd || !ws || !freq) return ext_fail(r, WF_E_INVALID, "wf_rose_set_rose: NULL argument");
  if (D < 1 || S < 1) return ext_fail(r, WF_E_INVALID, "a rose needs at least one direction and one speed");
  if ((size_t)D * S > ((size_t)1 << 24)) return ext_fail(r, WF_E_INVALID, "the rose is too large (more than 2^24 conditions)");
  if (std::isnan(cut_in) || std::isnan(cut_out)) return ext_fail(r, WF_E_INVALID, "cut_in / cut_out must not be NaN");
  for (int i = 0; i < D; ++i)
    if (!std::isfinite(wd[i])) return ext_fail(r, WF_E_INVALID, "rose wind directions must be finite");
  for (int i = 0; i < S; ++i)
    if (!(ws[i] > 0.0) || !std::isfinite(ws[i])) return ext_fail(r, WF_E_INVALID, "rose wind speeds must be > 0");
  for (size_t i = 0; i < (size_t)D * S; ++i)
    if (!std::isfinite(freq[i]) || !(freq[i] >= 0.0)) return ext_fail(r, WF_E_INVALID, "rose frequencies must be finite and >= 0");
  WFX_ON_DEVICE(r);
  r->D = 0;
  int rc = reserve(r, r->d_wd, (size_t)D);
  if (rc == WF_OK) rc = reserve(r, r->d_ws, (size_t)S);
  if (rc == WF_OK) rc = reserve(r, r->d_freq, (size_t)D * S);
  if (rc != WF_OK) return rc;
  hipStream_t st = r->h->stream;
  WFX_HIP(r, hipMemcpyAsync(r->d_wd, wd, sizeof(double) * D, hipMemcpyHostToDevice, st));
  WFX_HIP(r, hipMemcpyAsync(r->d_ws, ws, sizeof(double) * S, hipMemcpyHostToDevice, st));
  WFX_HIP(r, hipMemcpyAsync(r->d_freq, freq, sizeof(double) * D * S, hipMemcpyHostToDevice, st));
  WFX_HIP(r, hipStreamSynchronize(st));
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
  if (!r || !case_kind || !case_arg) return ext_fail(r, WF_E_INVALID, "wf_rose_evaluate: NULL argument");
  wf_handle* h = r->h;
  const int N = h->N, C = n_cases, D = r->D, S = r->S;
  const size_t cn = (size_t)C * N;
  row_batch& b = r->rows;
  int n_fixed = 0, R = 0;  // rows of fixed_yaw the cases name; rows of the run
  staging st(r, r->d_stage, on_device);
  WfRoseLayoutArgs la{};
  WfRoseReduceArgs ra{};
  row_policy k;
  k.what = "a rose evaluation serves"; k.name = nullptr;
  k.by_farm = false; k.split_always = true;
  k.strict = r->strict; k.max_eval = r->max_eval;
  k.check = [&]() -> int {
    if (D <= 0) return ext_fail(r, WF_E_INVALID, "no rose: wf_rose_set_rose comes first");
    if (C < 1 || C > WF_ROSE_MAX_CASES) return ext_fail(r, WF_E_INVALID, "the number of cases must be in 1..64");
    for (int c = 0; c < C; ++c) {
      const int kind = case_kind[c], arg = case_arg[c];
      if (kind == WF_ROSE_CASE_ZERO) continue;
      if (kind == WF_ROSE_CASE_FIXED) {
        if (arg < 0 || arg >= 65536) return ext_fail(r, WF_E_INVALID, "a fixed case names a row of fixed_yaw: 0 .. 65535");
        if (!fixed_yaw) return ext_fail(r, WF_E_INVALID, "a fixed case needs fixed_yaw");
        n_fixed = arg + 1 > n_fixed ? arg + 1 : n_fixed;
      } else if (kind == WF_ROSE_CASE_TABLE) {
        if (arg < 0 || arg >= WF_ROSE_SLOTS) return ext_fail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
        if (r->slot[arg].Dt <= 0) return ext_fail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
        if (r->slot[arg].N != N) return ext_fail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
      } else {
        return ext_fail(r, WF_E_INVALID, "unknown case kind (WF_ROSE_CASE_ZERO / _FIXED / _TABLE)");
      }
    }
    const long long rows = (long long)D * C * S;
    if (rows > (1LL << 30) / (N + 1)) return ext_fail(r, WF_E_INVALID, "too many rows: directions x cases x speeds x turbines must stay below 2^30");
    R = (int)rows;
    return WF_OK;
  };
  k.reserve = [&](int, int E) -> int {
    st.in(n_fixed ? fixed_yaw : nullptr, (size_t)n_fixed * N, &la.fixed_yaw);
    st.out(condition_power, (size_t)R, &ra.condition_power);
    int rc = reserve(r, r->d_rowsum, (size_t)E);
    if (rc == WF_OK) rc = reserve(r, r->d_acc, cn + C);
    if (rc == WF_OK) rc = reserve(r, r->d_cases, 2 * (size_t)C);
    if (rc != WF_OK) return rc;
    // the case list: uploaded when it differs from the one the device holds
    std::vector<int> cs(2 * (size_t)C);
    for (int c = 0; c < C; ++c) { cs[c] = case_kind[c]; cs[C + c] = case_arg[c]; }
    if (cs != r->cases) {
      WFX_HIP(r, hipStreamSynchronize(h->stream));  // (a previous upload may still read the host copy)
      r->cases.swap(cs);
      WFX_HIP(r, hipMemcpyAsync(r->d_cases, r->cases.data(), sizeof(int) * 2 * C, hipMemcpyHostToDevice, h->stream));
    }
    la.wd = r->d_wd; la.ws = r->d_ws; la.cases = r->d_cases;
    for (int i = 0; i < WF_ROSE_SLOTS; ++i) la.tab[i] = device_table(r->slot[i]);
    la.ews = b.d_wind; la.ewd = b.d_wind + E; la.yaw = b.d_yaw;
    ra.ws = r->d_ws; ra.freq = r->d_freq; ra.cut_in = r->cut_in; ra.cut_out = r->cut_out;
    ra.power = b.d_pow; ra.rowsum = r->d_rowsum;
    ra.acc_turbine = r->d_acc; ra.acc_farm = r->d_acc + cn;
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    la.sh = WfRoseShape{D, C, S, N, sl.base, sl.n_slots, E};
    WFX_HIP(r, wfk_launch_rose_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    ra.sh = la.sh; ra.first = sl.base == 0;
    WFX_HIP(r, wfk_launch_rose_rowsum(&ra, h->stream));
    WFX_HIP(r, wfk_launch_rose_accumulate(&ra, h->stream));
    return WF_OK;
  };
  k.finish = [&]() -> int {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (weighted_power) WFX_HIP(r, hipMemcpyAsync(weighted_power, r->d_acc + cn, sizeof(double) * C, kind, h->stream));
    if (weighted_turbine_power) WFX_HIP(r, hipMemcpyAsync(weighted_turbine_power, r->d_acc, sizeof(double) * cn, kind, h->stream));
    return WF_OK;
  };
  return run_rows(r, b, r->eval, k, st, &R, nullptr);
}

int wf_rose_policy(wf_rose* r, int slot, float* target_yaw, float* action, int on_device) {
  if (!r) return WF_E_INVALID;
  if (!target_yaw && !action) return ext_fail(r, WF_E_INVALID, "wf_rose_policy: NULL argument");
  wf_handle* h = r->h;
  int rc = check_parent(r, "a yaw look-up-table policy serves", nullptr);
  if (rc != WF_OK) return rc;
  if (slot < 0 || slot >= WF_ROSE_SLOTS) return ext_fail(r, WF_E_INVALID, "table slot out of range (0 .. 3)");
  if (r->slot[slot].Dt <= 0) return ext_fail(r, WF_E_INVALID, "no yaw table in that slot: wf_rose_set_table comes first");
  if (r->slot[slot].N != h->N) return ext_fail(r, WF_E_INVALID, "the yaw table was set for another turbine count: set it again");
  if ((rc = check_wind(r, "wf_rose_policy")) != WF_OK) return rc;
  if (!h->d_env_yaw) return ext_fail(r, WF_E_INVALID, "no env state: wf_env_config and wf_env_reset come first");
  WFX_ON_DEVICE(r);
  const size_t bn = (size_t)h->B * h->N;
  staging st(r, r->d_stage, on_device);
  WfRosePolicyArgs pa{};
  st.out(target_yaw, bn, &pa.target);
  st.out(action, bn, &pa.action);
  if ((rc = st.begin()) != WF_OK) return rc;
  pa.tab = device_table(r->slot[slot]);
  pa.B = h->B; pa.N = h->N; pa.wind_stride = h->wind_count == h->B ? 1 : 0;
  pa.ws = h->d_ws; pa.wd = h->d_wd; pa.yaw_state = h->d_env_yaw;
  pa.lo = h->env.yaw_lo; pa.hi = h->env.yaw_hi; pa.step = h->env.yaw_step; pa.discrete = h->env.discrete;
  WFX_HIP(r, wfk_launch_rose_policy(&pa, h->stream));
  return st.end();
}

// per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_rose_last_timing(wf_rose* r, float* total_ms, float* step_ms, float* glue_ms) {
  if (!r) return WF_E_INVALID;
  return last_timing(r, "wf_rose_evaluate has not run yet", total_ms, step_ms, glue_ms);
}

int wf_rose_kernel_info(wf_rose* r, int* info) {
  if (!r || !info) return ext_fail(r, WF_E_INVALID, "wf_rose_kernel_info: NULL argument");
  return kernel_info(r, WF_ROSE_KERNELS, wfk_rose_func_attributes, info);
}

const char* wf_rose_last_error(wf_rose* r) { return r ? r->err.c_str() : "wf_rose: NULL object"; }

}  // extern "C"
