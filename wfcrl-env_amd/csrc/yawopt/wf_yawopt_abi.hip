// wf_yawopt_abi.hip — the C boundary of the yaw-optimiser extension (include/wfyawopt.h): an optimiser object that belongs
// to a parent handle, owns an evaluator handle and its device buffers, and enqueues a whole coordinate search on the parent's
// stream: per visit one glue kernel of wf_yawopt_kernels.hip and one wf_step on the evaluator.  Reads the parent (layout,
// model, wind, kernel choice, resolve mode); stores nothing in it.  The object's scaffolding — base, buffers, the evaluator
// that follows the parent, checks, events — is the extensions' shared layer (ext/wf_ext.h).
#include "../../../include/wfyawopt.h"
#include "../ext/wf_ext.h"
#include "wf_yawopt.h"

using namespace wfi;

struct wf_yawopt : ext_base {
  // configuration
  double lo = -25.0, hi = 25.0;
  int P = 2, K[WF_YAWOPT_MAX_PASSES] = {5, 4, 0, 0};
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  dev_buf<float> d_yaw, d_pow, d_best;
  dev_buf<int> d_order;
  dev_buf<double> d_wind;  // [2][C R]
  farm_list farms;
  dev_buf<float> d_in, d_out;  // staging for host callers: yaw0; yaw_opt, power_opt, power_init
  evaluator eval;  // C x R farms
};

extern "C" {

int wf_yawopt_create(wf_handle* h, wf_yawopt** out) { return ext_create(h, out); }

int wf_yawopt_destroy(wf_yawopt* o) { return ext_destroy(o); }

int wf_yawopt_config(wf_yawopt* o, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms) {
  if (!o || !K) return ext_fail(o, WF_E_INVALID, "wf_yawopt_config: NULL argument");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return ext_fail(o, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (n_passes < 1 || n_passes > WF_YAWOPT_MAX_PASSES) return ext_fail(o, WF_E_INVALID, "the number of passes must be in 1..4");
  if (K[0] < 2 || K[0] > WF_YAWOPT_MAX_K0) return ext_fail(o, WF_E_INVALID, "the first pass needs 2..31 candidates (K_0)");
  for (int p = 1; p < n_passes; ++p)
    if (K[p] < 1 || K[p] > WF_YAWOPT_MAX_K) return ext_fail(o, WF_E_INVALID, "a refining pass needs 1..15 candidates (K_p)");
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (max_eval_farms < k_max(n_passes, K) + 1) return ext_fail(o, WF_E_INVALID, "max_eval_farms must hold one farm's candidates: at least K_max + 1");
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
  if (!o || !yaw_opt || !power_opt || !power_init) return ext_fail(o, WF_E_INVALID, "wf_yawopt_run: NULL argument");
  wf_handle* h = o->h;
  int rc = check_parent(o, "yaw optimisation serves", "wf_yawopt_run");
  if (rc == WF_OK) rc = check_farms(o, &n_farms, farms);
  if (rc != WF_OK) return rc;
  WFX_ON_DEVICE(o);
  const int N = h->N, R = k_max(o->P, o->K) + 1;
  int C = o->max_eval / R;
  if (C > n_farms) C = n_farms;
  if ((rc = ensure_evaluator(o, o->eval, C * R, o->strict ? 2 : h->resolve_mode)) != WF_OK) return rc;
  wf_handle* ev = o->eval.ev;
  const size_t blk = (size_t)C * R * N, fn = (size_t)n_farms * N;
  const bool per_farm = h->wind_count == h->B && h->B > 1;
  rc = reserve(o, o->d_yaw, blk);
  if (rc == WF_OK) rc = reserve(o, o->d_pow, blk);
  if (rc == WF_OK) rc = reserve(o, o->d_best, (size_t)C * N);
  if (rc == WF_OK) rc = reserve(o, o->d_order, (size_t)C * N);
  if (rc == WF_OK && per_farm) rc = reserve(o, o->d_wind, 2 * (size_t)C * R);
  if (rc == WF_OK && farms) rc = reserve(o, o->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw0) rc = reserve(o, o->d_in, fn);
  if (rc == WF_OK && !on_device) rc = reserve(o, o->d_out, fn + 2 * (size_t)n_farms);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(o, o->farms, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw0 = yaw0;
  if (yaw0 && !on_device) {
    WFX_HIP(o, hipMemcpyAsync(o->d_in, yaw0, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
    d_yaw0 = o->d_in;
  }
  float* d_oyaw = on_device ? yaw_opt : o->d_out;
  float* d_opow = on_device ? power_opt : o->d_out + fn;
  float* d_oini = on_device ? power_init : o->d_out + fn + n_farms;

  // the passes' grids (include/wfyawopt.h): h_0 = (hi - lo) / (K_0 - 1), h_p = 2 h_{p-1} / (K_p + 1)
  WfGrid grid[WF_YAWOPT_MAX_PASSES];
  pass_grids(o->lo, o->hi, o->P, o->K, grid);
  const WfGrid none{-1, 0, 0, 0.0, 0.0};
  const int V = o->P * N;  // visits
  o->n_ev = 0; o->timed = false;
  const bool detail = o->detail != 0;
  for (int base = 0; base < n_farms; base += C) {
    const int n_slots = n_farms - base < C ? n_farms - base : C;
    const WfSlots sl{farms ? o->farms.d.p : nullptr, base, n_slots, C};
    if (base == 0 || detail) { rc = record(o); if (rc != WF_OK) return rc; }  // (detail: 2 V + 2 events per chunk)
    // the evaluator's wind: the parent's one wind as it is, or each farm's wind repeated over its rows
    if (!per_farm) {
      if (base == 0) WFX_EV(o, ev, wf_set_wind_counts(ev, h->d_ws, 1, h->d_wd, 1, 1));
    } else {
      WfYawoptWindArgs wa{sl, h->d_ws, h->d_wd, R, o->d_wind, o->d_wind + (size_t)C * R};
      WFX_HIP(o, wfk_launch_yawopt_wind(&wa, h->stream));
      // (a parent whose farms share ONE direction keeps the shared geometry and the pair-table path on the evaluator too)
      if (h->shared_dir) WFX_EV(o, ev, wf_set_wind_counts(ev, wa.ews, C * R, h->d_wd, 1, 1));
      else WFX_EV(o, ev, wf_set_wind_counts(ev, wa.ews, C * R, wa.ewd, C * R, 1));
    }
    WfYawoptOrderArgs oa{{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, per_farm ? 1 : 0, N, o->d_order}};
    WFX_HIP(o, wfk_launch_yawopt_order(&oa, h->stream));
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
      WFX_HIP(o, wfk_launch_yawopt_advance(&aa, h->stream));
      if (detail) { rc = record(o); if (rc != WF_OK) return rc; }
      if (v < V) {
        WFX_EV(o, ev, wf_step(ev, o->d_yaw, o->d_pow, nullptr, nullptr, nullptr, 1));
        if (detail) { rc = record(o); if (rc != WF_OK) return rc; }
      }
    }
  }
  if (!detail) { rc = record(o); if (rc != WF_OK) return rc; }
  o->timed = true; o->per_chunk = detail ? 2 * (size_t)V + 2 : 0;
  if (!on_device) {
    WFX_HIP(o, hipMemcpyAsync(yaw_opt, o->d_out, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(o, hipMemcpyAsync(power_opt, o->d_out + fn, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(o, hipMemcpyAsync(power_init, o->d_out + fn + n_farms, sizeof(float) * n_farms, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(o, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

// with detail, per chunk the events are e0 | glue e | step e | glue e | ... | glue e: V + 1 glue intervals (the first one holds
// the chunk's wind and order kernels too) and V step intervals, then the next chunk's e0 (an empty interval)
int wf_yawopt_last_timing(wf_yawopt* o, float* total_ms, float* step_ms, float* glue_ms) {
  if (!o) return WF_E_INVALID;
  return last_timing(o, "wf_yawopt_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_yawopt_evaluator(wf_yawopt* o) { return o ? o->eval.ev : nullptr; }

const char* wf_yawopt_last_error(wf_yawopt* o) { return o ? o->err.c_str() : "wf_yawopt: NULL optimiser"; }

}  // extern "C"
