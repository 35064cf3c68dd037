// wf_yawopt_abi.hip — the C boundary of the yaw-optimiser extension (include/wfyawopt.h): an optimiser object that belongs
// to a parent handle, owns an evaluator handle and its device buffers, and enqueues a whole coordinate search on the parent's
// stream: per visit one glue kernel of wf_yawopt_kernels.hip and one wf_step on the evaluator.  Reads the parent (layout,
// model, wind, kernel choice, resolve mode); stores nothing in it.  The object's scaffolding — base, buffers, the evaluator
// that follows the parent, checks, events — and the search's driver (run_search: chunks, the visit loop, staging and
// copy-back) are the extensions' shared layer (ext/wf_ext.h); this file supplies the evaluator's wind and the launches.
#include "../../../include/wfyawopt.h"
#include "../ext/wf_ext.h"
#include "wf_yawopt.h"

using namespace wfi;

static_assert(WF_YAWOPT_MAX_PASSES == WF_SEARCH_MAX_PASSES && WF_YAWOPT_MAX_K0 == WF_SEARCH_MAX_K0 && WF_YAWOPT_MAX_K == WF_SEARCH_MAX_K &&
                  WF_YAWOPT_ROWS_MAX == WF_SEARCH_ROWS_MAX, "the shared search driver (ext/wf_ext.h) is built for these limits");

static const char* const kRowsMsg = "max_eval_farms must hold one farm's candidates: at least K_max + 1";

struct wf_yawopt : ext_base {
  yaw_search s;    // configuration and the buffers of every search; its wind [2][C R] is filled for per-farm winds only
  evaluator eval;  // C x R farms
};

extern "C" {

int wf_yawopt_create(wf_handle* h, wf_yawopt** out) { return ext_create(h, out); }

int wf_yawopt_destroy(wf_yawopt* o) { return ext_destroy(o); }

int wf_yawopt_config(wf_yawopt* o, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms) {
  if (!o || !K) return ext_fail(o, WF_E_INVALID, "wf_yawopt_config: NULL argument");
  return set_search_config(o, o->s.cfg, lo, hi, n_passes, K, strict, max_eval_farms, 1, kRowsMsg);
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
  const bool per_farm = h->wind_count == h->B && h->B > 1;
  search_policy k{"yaw optimisation serves", "wf_yawopt_run", 1, "", kRowsMsg, nullptr, nullptr, nullptr};
  k.reserve = [&](int E) -> int { return per_farm ? reserve(o, o->s.d_wind, 2 * (size_t)E) : WF_OK; };
  // the evaluator's wind: the parent's one wind as it is, or each farm's wind repeated over its rows; then the visit order
  k.begin_chunk = [&](const WfSlots& sl, int R, int E) -> int {
    wf_handle* ev = o->eval.ev;
    if (!per_farm) {
      if (sl.base == 0) WFX_EV(o, ev, wf_set_wind_counts(ev, h->d_ws, 1, h->d_wd, 1, 1));
    } else {
      WfYawoptWindArgs wa{sl, h->d_ws, h->d_wd, R, o->s.d_wind, o->s.d_wind + E};
      WFX_HIP(o, wfk_launch_yawopt_wind(&wa, h->stream));
      // (a parent whose farms share ONE direction keeps the shared geometry and the pair-table path on the evaluator too)
      if (h->shared_dir) WFX_EV(o, ev, wf_set_wind_counts(ev, wa.ews, E, h->d_wd, 1, 1));
      else WFX_EV(o, ev, wf_set_wind_counts(ev, wa.ews, E, wa.ewd, E, 1));
    }
    WfYawoptOrderArgs oa{{sl, h->d_lx, h->d_ly, h->xc, h->yc, h->d_wd, per_farm ? 1 : 0, h->N, o->s.d_order}};
    WFX_HIP(o, wfk_launch_yawopt_order(&oa, h->stream));
    return WF_OK;
  };
  k.visit = [&](const WfAdvanceArgs& a, int) -> int {
    const WfYawoptAdvanceArgs aa{a, o->s.d_pow};
    WFX_HIP(o, wfk_launch_yawopt_advance(&aa, h->stream));
    return WF_OK;
  };
  return run_search(o, o->s, o->eval, k, yaw0, n_farms, farms, yaw_opt, power_opt, power_init, on_device);
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
