// wf_polsearch_abi.hip — the C boundary of the policy-search extension (include/wfpolsearch.h): an object that belongs to a
// parent handle, BORROWS the handle's policy object and, optionally, its polscen object, owns its device buffers and enqueues a
// whole search on the parent's stream.  It owns no evaluator and drives no step: per iteration it calls wf_policy_run or
// wf_polscen_run with on_device = 1 on its own candidate and score buffers, so network, strict, max_eval_farms, chunking and
// every refusal of a rollout are those objects'; between two such runs it launches its two kernels (wf_polsearch_kernels.hip).
// The host layer is the extensions' shared one (ext/wf_ext.h: checks of the parent and the farm list, dev_buf, reserve, staging,
// events and the split of a timed run, kernel attributes).  Reads the parent; stores nothing in it.
#include <cmath>
#include <string>

#include "../../../include/wfpolsearch.h"
#include "../ensemble/wf_ensemble_host.h"
#include "../ext/wf_ext.h"
#include "wf_polsearch.h"

using namespace wfi;

struct wf_polsearch : ext_base {
  wf_policy* policy = nullptr;  // borrowed: the held-wind scorer; it outlives this object
  wf_polscen* scen = nullptr;   // borrowed: the ensemble scorer, or null
  // device buffers (grow-only)
  dev_buf<float> d_cand;        // [2][K][P]
  dev_buf<double> d_scores;     // [n][K]
  dev_buf<double> d_tile;       // [T][K]
  dev_buf<char> d_stage;        // staging for host callers: mean0, sigma0, wind, anchor; the ten outputs
};

extern "C" {

int wf_polsearch_create(wf_handle* h, wf_policy* policy, wf_polscen* scen, wf_polsearch** out) {
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  if (!policy) return fail(h, WF_E_INVALID, "wf_polsearch_create: the policy object (the scorer) is NULL");
  const int rc = ext_create(h, out);
  if (rc != WF_OK) return rc;
  (*out)->policy = policy;
  (*out)->scen = scen;
  return WF_OK;
}

int wf_polsearch_destroy(wf_polsearch* s) { return ext_destroy(s); }

int wf_polsearch_set_timing(wf_polsearch* s, int detail) {
  if (!s) return WF_E_INVALID;
  s->detail = detail != 0;
  return WF_OK;
}

int wf_polsearch_run(wf_polsearch* s, const float* mean0, const float* sigma0, int P, int K, int E, int I, double sigma_min,
                     unsigned long long seed, int H, double gamma, const double* wind, int M, const wf_wind_process* process,
                     double ws_lo, double ws_hi, unsigned long long scenario_seed, int tail, double risk_weight, const double* anchor,
                     int n_farms, const int* farms, float* best_params, double* best_fitness, double* init_fitness, float* mean,
                     float* sigma, double* fitness, int* winner, float* candidates, float* sigma_history, double* farm_scores,
                     int on_device) {
  if (!s) return WF_E_INVALID;
  wf_handle* h = s->h;
  int rc = check_parent(s, "policy search serves", "wf_polsearch_run");
  if (rc != WF_OK) return rc;
  if ((rc = check_farms(s, &n_farms, farms)) != WF_OK) return rc;
  if (K < WF_POLSEARCH_MIN_K || K > WF_POLSEARCH_MAX_K)
    return ext_fail(s, WF_E_INVALID, "the number of candidates K must be in 3..64 (the incumbent, the mean, a draw)");
  if (E < 1 || E > K) return ext_fail(s, WF_E_INVALID, "the number of elites E must be in 1..K");
  if (I < 1 || I > WF_POLSEARCH_MAX_ITER) return ext_fail(s, WF_E_INVALID, "the number of iterations I must be in 1..16");
  if (!non_negative(sigma_min)) return ext_fail(s, WF_E_INVALID, "sigma_min must be finite and >= 0");
  if (P < 1) return ext_fail(s, WF_E_INVALID, "the number of parameters P must be >= 1");
  if (!mean0 || !sigma0) return ext_fail(s, WF_E_INVALID, "wf_polsearch_run: mean0 or sigma0 is NULL");
  if (M < 0) return ext_fail(s, WF_E_INVALID, "the number of members M must be >= 0 (0: the held-wind scorer)");
  if (M > 0 && !s->scen)
    return ext_fail(s, WF_E_INVALID, "members need the ensemble scorer: this object was created without a polscen object");
  if (M > 0 && wind) return ext_fail(s, WF_E_INVALID, "a wind per step and members exclude each other: the members' paths are the wind");
  if (!on_device) {  // a host caller's vectors are read here; a device caller's are not
    for (int p = 0; p < P; ++p)
      if (!std::isfinite(mean0[p])) return ext_fail(s, WF_E_INVALID, "every entry of the start vector mean0 must be finite");
    for (int p = 0; p < P; ++p)
      if (!std::isfinite(sigma0[p]) || sigma0[p] < 0.0f) return ext_fail(s, WF_E_INVALID, "every width sigma0 must be finite and >= 0");
    if (M > 0 && (rc = check_ensemble_anchor(s, anchor, n_farms, 0)) != WF_OK) return rc;
  }
  WFX_ON_DEVICE(s);
  const int n = n_farms, T = (n + WF_POLSEARCH_TILE - 1) / WF_POLSEARCH_TILE;
  const size_t kp = (size_t)K * P, nk = (size_t)n * K;
  rc = reserve(s, s->d_cand, 2 * kp);
  if (rc == WF_OK) rc = reserve(s, s->d_scores, nk);
  if (rc == WF_OK) rc = reserve(s, s->d_tile, (size_t)T * K);
  if (rc != WF_OK) return rc;
  WfPolSearchRun r{};
  const double *d_wind = nullptr, *d_anchor = nullptr;
  staging st(s, s->d_stage, on_device);
  st.in(mean0, (size_t)P, &r.mean0); st.in(sigma0, (size_t)P, &r.sigma0);
  st.in(wind, (size_t)n * (H > 0 ? H : 0) * 2, &d_wind); st.in(anchor, (size_t)n * 2, &d_anchor);
  st.out(best_params, (size_t)P, &r.best_params); st.out(best_fitness, 1, &r.best_fitness); st.out(init_fitness, 1, &r.init_fitness);
  st.out(mean, (size_t)P, &r.mean); st.out(sigma, (size_t)P, &r.sigma);
  st.out(fitness, (size_t)I * K, &r.fitness); st.out(winner, (size_t)I, &r.winner);
  st.out(candidates, (size_t)I * kp, &r.candidates); st.out(sigma_history, (size_t)I * P, &r.sigma_history);
  st.out(farm_scores, (size_t)I * nk, &r.farm_scores);
  if ((rc = st.begin()) != WF_OK) return rc;
  r.K = K; r.P = P; r.E = E; r.I = I; r.n = n; r.T = T;
  r.sigma_min = sigma_min; r.seed = seed;
  r.cand = s->d_cand; r.scores = s->d_scores; r.tile = s->d_tile;

  // events: the run's first and last, or with detail e0 | advance 0 e | scorer e | tiles + advance 1 e | scorer e | ... | tiles +
  // advance I e: last_timing's layout with one chunk of 2 I + 2 events, the scorer's intervals in the step's places
  const bool detail = s->detail != 0;
  s->n_ev = 0; s->timed = false;
  if ((rc = record(s)) != WF_OK) return rc;
  for (int v = 0; v <= I; ++v) {
    if (v > 0) WFX_HIP(s, wfk_launch_polsearch_tiles(&r, v - 1, h->stream));
    WFX_HIP(s, wfk_launch_polsearch_advance(&r, v, h->stream));
    if (v == I) break;
    if (detail && (rc = record(s)) != WF_OK) return rc;
    const float* const c = s->d_cand.p + (size_t)(v & 1) * kp;
    if (M > 0) {
      rc = wf_polscen_run(s->scen, c, K, P, H, M, process, ws_lo, ws_hi, scenario_seed, gamma, tail, risk_weight, d_anchor, n, farms,
                          nullptr, nullptr, s->d_scores, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, 1);
      if (rc != WF_OK) return ext_fail(s, rc, wf_polscen_last_error(s->scen));
    } else {
      rc = wf_policy_run(s->policy, c, K, P, H, d_wind, gamma, n, farms, s->d_scores, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, 1);
      if (rc != WF_OK) return ext_fail(s, rc, wf_policy_last_error(s->policy));
    }
    if (detail && (rc = record(s)) != WF_OK) return rc;
  }
  if ((rc = record(s)) != WF_OK) return rc;
  s->timed = true; s->per_chunk = detail ? 2 * (size_t)I + 2 : 0;
  return st.end();
}

int wf_polsearch_last_timing(wf_polsearch* s, float* total_ms, float* scorer_ms, float* own_ms) {
  if (!s) return WF_E_INVALID;
  return last_timing(s, "wf_polsearch_run has not run yet", total_ms, scorer_ms, own_ms);
}

int wf_polsearch_kernel_info(wf_polsearch* s, int* info) {
  if (!s || !info) return ext_fail(s, WF_E_INVALID, "wf_polsearch_kernel_info: NULL argument");
  return kernel_info(s, WF_POLSEARCH_KERNELS, wfk_polsearch_func_attributes, info);
}

const char* wf_polsearch_last_error(wf_polsearch* s) { return s ? s->err.c_str() : "wf_polsearch: NULL object"; }

}  // extern "C"
