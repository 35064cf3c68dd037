// wf_ensemble_host.h — the host side of the wind ensemble (ensemble/wf_ensemble.h), ONCE: what the *_run entry points of the
// four extensions that score something over M wind futures (scenario/, scenplan/, rollscen/, polscen/) check of the ensemble's
// arguments, with the refusals' texts, and how a chunk's WfEnsemble is filled from the parent handle.  The predicates are
// ext/wf_ext.h's (in_unit, non_negative), which the wind generator's process check uses too (windgen/wf_windgen_abi.hip).
//
// The checks come in three pieces because the entry points test other things of their own between them, and the order of the
// refusals is part of their behaviour: the statistics' arguments, the process and the bounds — check_ensemble is the two in a
// row, for the entry points that test nothing between them —, and the anchor, which every entry point tests after its env state.
#pragma once
#include <cmath>
#include <string>

#include "../../../include/wfwindgen.h"
#include "../ext/wf_ext.h"
#include "wf_ensemble.h"

namespace wfi {

inline int check_ensemble_statistics(ext_base* x, int M, int tail, double risk_weight, double gamma) {
  if (tail < 1 || tail > M) return ext_fail(x, WF_E_INVALID, "tail must be in 1..M: the number of lowest member returns the tail mean is over");
  if (!in_unit(risk_weight)) return ext_fail(x, WF_E_INVALID, "risk_weight must be finite and in [0, 1]");
  if (!in_unit(gamma)) return ext_fail(x, WF_E_INVALID, "gamma must be finite and in [0, 1]");
  return WF_OK;
}

// `call` is the entry point's name
inline int check_ensemble_process(ext_base* x, const char* call, const wf_wind_process* process, double ws_lo, double ws_hi) {
  if (!process) return ext_fail(x, WF_E_INVALID, std::string(call) + ": process is NULL");
  const wf_wind_process& p = *process;
  if (!in_unit(p.ws_revert) || !in_unit(p.wd_revert)) return ext_fail(x, WF_E_INVALID, "ws_revert and wd_revert must be in [0, 1]");
  if (!non_negative(p.ws_sigma) || !non_negative(p.wd_sigma) || !non_negative(p.wd_ramp))
    return ext_fail(x, WF_E_INVALID, "ws_sigma, wd_sigma and wd_ramp must be finite and >= 0");
  if (!std::isfinite(ws_lo) || !std::isfinite(ws_hi) || !(ws_lo > 0.0) || !(ws_lo < ws_hi))
    return ext_fail(x, WF_E_INVALID, "the speed bounds must be finite with 0 < ws_lo < ws_hi");
  return WF_OK;
}

inline int check_ensemble(ext_base* x, const char* call, int M, int tail, double risk_weight, double gamma, const wf_wind_process* process,
                          double ws_lo, double ws_hi) {
  const int rc = check_ensemble_statistics(x, M, tail, risk_weight, gamma);
  return rc != WF_OK ? rc : check_ensemble_process(x, call, process, ws_lo, ws_hi);
}

// a host caller's anchor is read here; a device caller's is not
inline int check_ensemble_anchor(ext_base* x, const double* anchor, int n_farms, int on_device) {
  if (anchor && !on_device)
    for (int i = 0; i < n_farms; ++i)
      if (!(anchor[2 * i] > 0.0) || !std::isfinite(anchor[2 * i]) || !std::isfinite(anchor[2 * i + 1]))
        return ext_fail(x, WF_E_INVALID, "the anchor's speed must be > 0 and its direction finite");
  return WF_OK;
}

// the ensemble of the chunk whose first farm is entry `first` of the list: d_anchor is the whole run's [n_farms][2], or null
inline WfEnsemble ensemble_args(const wf_handle* h, int M, int H, const wf_wind_process& p, double ws_lo, double ws_hi, unsigned long long seed,
                                const double* d_anchor, size_t first) {
  WfEnsemble e{};
  e.seed = seed;
  e.ws_revert = p.ws_revert; e.ws_sigma = p.ws_sigma; e.wd_revert = p.wd_revert; e.wd_sigma = p.wd_sigma; e.wd_ramp = p.wd_ramp;
  e.ws_lo = ws_lo; e.ws_hi = ws_hi;
  e.anchor = d_anchor ? d_anchor + first * 2 : nullptr;
  e.ws = h->d_ws; e.wd = h->d_wd; e.wind_stride = h->wind_count == 1 ? 0 : 1;
  e.M = M; e.H = H;
  return e;
}

}  // namespace wfi
