// wf_credit_abi.hip — the C boundary of the credit extension (include/wfcredit.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole counterfactual run on the parent's stream: per chunk
// one lay-out kernel, one wf_step on the evaluator (power and load) and one reduce kernel (wf_credit_kernels.hip).  Reads the
// parent (layout, model, wind, env parameters and env state, kernel choice, resolve mode); stores nothing in it — in
// particular the speed a wf_env_set_prev_wind left for the next env step stays for that step.  The object's scaffolding is
// the extensions' shared layer (ext/wf_ext.h).
#include "../../../include/wfcredit.h"
#include "../ext/wf_ext.h"
#include "wf_credit.h"

using namespace wfi;

struct wf_credit : ext_base {
  // configuration
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  dev_buf<float> d_yaw, d_pow, d_load;  // [E][N], [E][N], [E][N][4]
  dev_buf<double> d_wind;               // [2][E]
  farm_list farms;
  dev_buf<float> d_in;    // staging for host callers: base and alt rows
  dev_buf<double> d_out;  // ... and the outputs
  evaluator eval;  // E = C (1 + N K) farms
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least 1 + N K";
const char* const kNoEnv = "no env state: wf_env_config and wf_env_reset come first (an action, or base == NULL, is taken at the fused env's state)";

bool is_kind(int k) { return k == WF_CREDIT_YAW || k == WF_CREDIT_ACTION; }

}  // namespace

extern "C" {

int wf_credit_create(wf_handle* h, wf_credit** out) { return ext_create(h, out); }

int wf_credit_destroy(wf_credit* c) { return ext_destroy(c); }

int wf_credit_config(wf_credit* c, int strict, int max_eval_farms) {
  if (!c) return WF_E_INVALID;
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (c->h->N > 0 && max_eval_farms < c->h->N + 1) return ext_fail(c, WF_E_INVALID, kRowsMsg);
  c->strict = strict != 0; c->max_eval = max_eval_farms;
  return WF_OK;
}

int wf_credit_set_timing(wf_credit* c, int detail) {
  if (!c) return WF_E_INVALID;
  c->detail = detail != 0;
  return WF_OK;
}

int wf_credit_run(wf_credit* c, int base_kind, const float* base, int alt_kind, const float* alt, int K, int n_farms,
                  const int* farms, double* reward, double* farm_power, double* difference, int on_device) {
  if (!c) return WF_E_INVALID;
  wf_handle* h = c->h;
  int rc = check_parent(c, "counterfactual rewards serve", "wf_credit_run");
  if (rc == WF_OK) rc = check_farms(c, &n_farms, farms);
  if (rc != WF_OK) return rc;
  if (K < 1 || K > WF_CREDIT_MAX_ALT) return ext_fail(c, WF_E_INVALID, "the number of alternatives K must be in 1..8");
  if (!is_kind(base_kind) || !is_kind(alt_kind)) return ext_fail(c, WF_E_INVALID, "base_kind and alt_kind are WF_CREDIT_YAW (0) or WF_CREDIT_ACTION (1)");
  if (!alt && K != 1) return ext_fail(c, WF_E_INVALID, "alt == NULL (hold / zero yaw) is one alternative: K must be 1");
  const bool needs_env = !base || base_kind == WF_CREDIT_ACTION || alt_kind == WF_CREDIT_ACTION;
  if (needs_env && !h->d_env_yaw) return ext_fail(c, WF_E_INVALID, kNoEnv);
  const int N = h->N, R = 1 + N * K;
  if (c->max_eval < R) return ext_fail(c, WF_E_INVALID, kRowsMsg);
  WFX_ON_DEVICE(c);
  int C = c->max_eval / R;
  if (C > n_farms) C = n_farms;
  const int E = C * R;
  if ((rc = ensure_evaluator(c, c->eval, E, c->strict ? 2 : h->resolve_mode)) != WF_OK) return rc;
  wf_handle* ev = c->eval.ev;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N, fr = (size_t)n_farms * R, fnk = fn * K;
  const size_t n_in = (base ? fn : 0) + (alt ? fnk : 0);
  const size_t n_out = (reward ? fr : 0) + (farm_power ? fr : 0) + (difference ? fnk : 0);
  rc = reserve(c, c->d_yaw, en);
  if (rc == WF_OK) rc = reserve(c, c->d_pow, en);
  if (rc == WF_OK) rc = reserve(c, c->d_load, 4 * en);
  if (rc == WF_OK) rc = reserve(c, c->d_wind, 2 * (size_t)E);
  if (rc == WF_OK && farms) rc = reserve(c, c->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && n_in) rc = reserve(c, c->d_in, n_in);
  if (rc == WF_OK && !on_device && n_out) rc = reserve(c, c->d_out, n_out);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(c, c->farms, farms, n_farms)) != WF_OK) return rc;
  const float *d_base = base, *d_alt = alt;
  if (!on_device) {
    if (base) {
      WFX_HIP(c, hipMemcpyAsync(c->d_in, base, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
      d_base = c->d_in;
    }
    if (alt) {
      float* dst = c->d_in + (base ? fn : 0);
      WFX_HIP(c, hipMemcpyAsync(dst, alt, sizeof(float) * fnk, hipMemcpyHostToDevice, h->stream));
      d_alt = dst;
    }
  }
  double* d_rew = out_ptr(reward, c->d_out, 0, on_device);
  double* d_fp = out_ptr(farm_power, c->d_out, reward ? fr : 0, on_device);
  double* d_dif = out_ptr(difference, c->d_out, (reward ? fr : 0) + (farm_power ? fr : 0), on_device);
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  WfCreditEnv env{};
  env.yaw = h->d_env_yaw; env.acc = h->d_env_acc; env.moves = h->d_env_moves;
  env.lo = h->env.yaw_lo; env.hi = h->env.yaw_hi; env.step = h->env.yaw_step;
  env.rate = h->env.actuator_rate; env.dt = h->env.dt; env.budget = h->env.budget; env.discrete = h->env.discrete;
  const bool detail = c->detail != 0;
  c->n_ev = 0; c->timed = false;
  for (int first = 0; first < n_farms; first += C) {
    if (first == 0 || detail) { rc = record(c); if (rc != WF_OK) return rc; }  // (detail: four events per chunk)
    WfCreditLayoutArgs la{};
    la.sl = chunk_slots(c->farms, farms, first, n_farms, C);
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N; la.K = K;
    la.env = env; la.base_kind = base_kind; la.alt_kind = alt_kind;
    la.base = d_base ? d_base + (size_t)first * N : nullptr;
    la.alt = d_alt ? d_alt + (size_t)first * N * K : nullptr;
    la.yaw = c->d_yaw; la.ews = c->d_wind; la.ewd = c->d_wind + E;
    WFX_HIP(c, wfk_launch_credit_layout(&la, h->stream));
    if (detail) { rc = record(c); if (rc != WF_OK) return rc; }
    WFX_EV(c, ev, wf_set_wind_counts(ev, la.ews, E, la.ewd, E, 1));
    WFX_EV(c, ev, wf_step(ev, c->d_yaw, c->d_pow, nullptr, nullptr, c->d_load, 1));
    if (detail) { rc = record(c); if (rc != WF_OK) return rc; }
    WfCreditReduceArgs ra{};
    ra.sl = la.sl; ra.N = N; ra.K = K;
    ra.ws = h->d_ws; ra.wind_stride = wind_stride;
    ra.ws_prev = (h->ws_prev_valid && h->d_ws_prev) ? h->d_ws_prev : nullptr;  // read, not consumed
    ra.load_coef = h->env.load_coef;
    ra.yaw_ev = c->d_yaw; ra.power_ev = c->d_pow; ra.load_ev = c->d_load;
    ra.reward = d_rew ? d_rew + (size_t)first * R : nullptr;
    ra.farm_power = d_fp ? d_fp + (size_t)first * R : nullptr;
    ra.difference = d_dif ? d_dif + (size_t)first * N * K : nullptr;
    WFX_HIP(c, wfk_launch_credit_reduce(&ra, h->stream));
    if (detail) { rc = record(c); if (rc != WF_OK) return rc; }
  }
  if (!detail) { rc = record(c); if (rc != WF_OK) return rc; }
  c->timed = true; c->per_chunk = detail ? 4 : 0;
  if (!on_device) {
    if (reward) WFX_HIP(c, hipMemcpyAsync(reward, d_rew, sizeof(double) * fr, hipMemcpyDeviceToHost, h->stream));
    if (farm_power) WFX_HIP(c, hipMemcpyAsync(farm_power, d_fp, sizeof(double) * fr, hipMemcpyDeviceToHost, h->stream));
    if (difference) WFX_HIP(c, hipMemcpyAsync(difference, d_dif, sizeof(double) * fnk, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(c, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_credit_last_timing(wf_credit* c, float* total_ms, float* step_ms, float* glue_ms) {
  if (!c) return WF_E_INVALID;
  return last_timing(c, "wf_credit_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_credit_evaluator(wf_credit* c) { return c ? c->eval.ev : nullptr; }

int wf_credit_kernel_info(wf_credit* c, int* info) {
  if (!c || !info) return ext_fail(c, WF_E_INVALID, "wf_credit_kernel_info: NULL argument");
  return kernel_info(c, WF_CREDIT_KERNELS, wfk_credit_func_attributes, info);
}

const char* wf_credit_last_error(wf_credit* c) { return c ? c->err.c_str() : "wf_credit: NULL object"; }

}  // extern "C"
