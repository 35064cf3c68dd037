// wf_grad_abi.hip — the C boundary of the gradient extension (include/wfgrad.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole sensitivity run on the parent's stream: per chunk one
// lay-out kernel, one wf_step on the evaluator and one reduce kernel (wf_grad_kernels.hip).  Reads the parent (layout, model,
// wind, kernel choice, resolve mode); stores nothing in it.  The object's scaffolding — base, buffers, the evaluator that
// follows the parent, checks, events — is the extensions' shared layer (ext/wf_ext.h).
#include "../../../include/wfgrad.h"
#include "../ext/wf_ext.h"
#include "wf_grad.h"

using namespace wfi;

struct wf_grad : ext_base {
  // configuration
  double step = 1.0, lo = -45.0, hi = 45.0;
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  dev_buf<float> d_yaw, d_pow;    // [E][N], [E][N]
  dev_buf<double> d_wind, d_div;  // [2][E], [C][N]
  farm_list farms;
  dev_buf<float> d_in, d_outf;  // staging for host callers: yaw and cotangent rows; the float output
  dev_buf<double> d_outd;       // ... and the double outputs
  evaluator eval;  // E = C (2 N + 1) farms
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one farm's rows: at least 2 N + 1";

}  // namespace

extern "C" {

int wf_grad_create(wf_handle* h, wf_grad** out) { return ext_create(h, out); }

int wf_grad_destroy(wf_grad* g) { return ext_destroy(g); }

int wf_grad_config(wf_grad* g, double h, double lo, double hi, int strict, int max_eval_farms) {
  if (!g) return WF_E_INVALID;
  if (!std::isfinite(h) || !(h > 0.0)) return ext_fail(g, WF_E_INVALID, "the step h must be finite and positive (degrees)");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return ext_fail(g, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (g->h->N > 0 && max_eval_farms < 2 * g->h->N + 1) return ext_fail(g, WF_E_INVALID, kRowsMsg);
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
  int rc = check_parent(g, "yaw sensitivities serve", "wf_grad_run");
  if (rc == WF_OK) rc = check_farms(g, &n_farms, farms);
  if (rc != WF_OK) return rc;
  const int N = h->N, R = 2 * N + 1;
  if (g->max_eval < R) return ext_fail(g, WF_E_INVALID, kRowsMsg);
  WFX_ON_DEVICE(g);
  int C = g->max_eval / R;
  if (C > n_farms) C = n_farms;
  const int E = C * R;
  if ((rc = ensure_evaluator(g, g->eval, E, g->strict ? 2 : h->resolve_mode)) != WF_OK) return rc;
  wf_handle* ev = g->eval.ev;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N, fnn = fn * N;
  const size_t n_in = (yaw ? fn : 0) + (cotangent ? fn : 0);
  const size_t n_outd = (gradient ? fn : 0) + (jacobian ? fnn : 0);
  rc = reserve(g, g->d_yaw, en);
  if (rc == WF_OK) rc = reserve(g, g->d_pow, en);
  if (rc == WF_OK) rc = reserve(g, g->d_wind, 2 * (size_t)E);
  if (rc == WF_OK) rc = reserve(g, g->d_div, (size_t)C * N);
  if (rc == WF_OK && farms) rc = reserve(g, g->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && n_in) rc = reserve(g, g->d_in, n_in);
  if (rc == WF_OK && !on_device && power) rc = reserve(g, g->d_outf, fn);
  if (rc == WF_OK && !on_device && n_outd) rc = reserve(g, g->d_outd, n_outd);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(g, g->farms, farms, n_farms)) != WF_OK) return rc;
  const float *d_yaw_in = yaw, *d_cot = cotangent;
  if (!on_device) {
    if (yaw) {
      WFX_HIP(g, hipMemcpyAsync(g->d_in, yaw, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
      d_yaw_in = g->d_in;
    }
    if (cotangent) {
      float* dst = g->d_in + (yaw ? fn : 0);
      WFX_HIP(g, hipMemcpyAsync(dst, cotangent, sizeof(float) * fn, hipMemcpyHostToDevice, h->stream));
      d_cot = dst;
    }
  }
  float* d_power = out_ptr(power, g->d_outf, 0, on_device);
  double* d_grad = out_ptr(gradient, g->d_outd, 0, on_device);
  double* d_jac = out_ptr(jacobian, g->d_outd, gradient ? fn : 0, on_device);
  const int wind_stride = h->wind_count == 1 ? 0 : 1;
  const bool detail = g->detail != 0;
  g->n_ev = 0; g->timed = false;
  for (int base = 0; base < n_farms; base += C) {
    const size_t off = (size_t)base * N;
    if (base == 0 || detail) { rc = record(g); if (rc != WF_OK) return rc; }  // (detail: four events per chunk)
    WfGradLayoutArgs la{};
    la.sl = chunk_slots(g->farms, farms, base, n_farms, C);
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N;
    la.h = g->step; la.lo = g->lo; la.hi = g->hi;
    la.yaw_in = d_yaw_in ? d_yaw_in + off : nullptr; la.yaw = g->d_yaw;
    la.ews = g->d_wind; la.ewd = g->d_wind + E; la.d = g->d_div;
    WFX_HIP(g, wfk_launch_grad_layout(&la, h->stream));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
    WFX_EV(g, ev, wf_set_wind_counts(ev, la.ews, E, la.ewd, E, 1));
    WFX_EV(g, ev, wf_step(ev, g->d_yaw, g->d_pow, nullptr, nullptr, nullptr, 1));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
    WfGradReduceArgs ra{};
    ra.n_slots = la.sl.n_slots; ra.N = N; ra.power_ev = g->d_pow; ra.d = g->d_div;
    ra.cot = d_cot ? d_cot + off : nullptr;
    ra.power = d_power ? d_power + off : nullptr;
    ra.gradient = d_grad ? d_grad + off : nullptr;
    ra.jacobian = d_jac ? d_jac + off * N : nullptr;
    WFX_HIP(g, wfk_launch_grad_reduce(&ra, h->stream));
    if (detail) { rc = record(g); if (rc != WF_OK) return rc; }
  }
  if (!detail) { rc = record(g); if (rc != WF_OK) return rc; }
  g->timed = true; g->per_chunk = detail ? 4 : 0;
  if (!on_device) {
    if (power) WFX_HIP(g, hipMemcpyAsync(power, g->d_outf, sizeof(float) * fn, hipMemcpyDeviceToHost, h->stream));
    if (gradient) WFX_HIP(g, hipMemcpyAsync(gradient, g->d_outd, sizeof(double) * fn, hipMemcpyDeviceToHost, h->stream));
    if (jacobian) WFX_HIP(g, hipMemcpyAsync(jacobian, d_jac, sizeof(double) * fnn, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(g, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

// with detail, per chunk: e0 | lay-out e1 | wind + step e2 | reduce e3, then the next chunk's e0
int wf_grad_last_timing(wf_grad* g, float* total_ms, float* step_ms, float* glue_ms) {
  if (!g) return WF_E_INVALID;
  return last_timing(g, "wf_grad_run has not run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_grad_evaluator(wf_grad* g) { return g ? g->eval.ev : nullptr; }

int wf_grad_kernel_info(wf_grad* g, int* info) {
  if (!g || !info) return ext_fail(g, WF_E_INVALID, "wf_grad_kernel_info: NULL argument");
  return kernel_info(g, WF_GRAD_KERNELS, wfk_grad_func_attributes, info);
}

const char* wf_grad_last_error(wf_grad* g) { return g ? g->err.c_str() : "wf_grad: NULL object"; }

}  // extern "C"
