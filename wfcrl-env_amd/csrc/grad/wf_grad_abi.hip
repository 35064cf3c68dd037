// wf_grad_abi.hip — the C boundary of the gradient extension (include/wfgrad.h): an object that belongs to a parent handle,
// owns an evaluator handle and its device buffers, and enqueues a whole sensitivity run on the parent's stream.  The run is
// the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of 2 N + 1 rows per farm, the evaluator and
// its step, events); this file supplies a chunk's lay-out and reduce launches (wf_grad_kernels.hip) and names the caller's
// arrays to stage.  Reads the parent (layout, model, wind, kernel choice, resolve mode); stores nothing in it.
#include "../../../include/wfgrad.h"
#include "../ext/wf_ext.h"
#include "wf_grad.h"

using namespace wfi;

struct wf_grad : ext_base {
  // configuration
  double step = 1.0, lo = -45.0, hi = 45.0;
  int strict = 0, max_eval = 65536;
  // device buffers (grow-only)
  row_batch rows;         // E = C (2 N + 1) farms
  dev_buf<double> d_div;  // [C][N]
  dev_buf<char> d_stage;  // staging for host callers: yaw and cotangent rows; power, gradient, jacobian
  evaluator eval;
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
  const int N = h->N, wind_stride = h->wind_count == 1 ? 0 : 1;
  row_batch& b = g->rows;
  const float *d_yaw_in = nullptr, *d_cot = nullptr;
  float* d_power = nullptr;
  double *d_grad = nullptr, *d_jac = nullptr;
  staging st(g, g->d_stage, on_device);
  row_policy k;
  k.what = "yaw sensitivities serve"; k.name = "wf_grad_run";
  k.rows = 2 * N + 1; k.rows_msg = kRowsMsg;
  k.strict = g->strict; k.max_eval = g->max_eval;
  k.reserve = [&](int C, int) -> int {
    const size_t fn = (size_t)n_farms * N;
    st.in(yaw, fn, &d_yaw_in); st.in(cotangent, fn, &d_cot);
    st.out(power, fn, &d_power); st.out(gradient, fn, &d_grad); st.out(jacobian, fn * N, &d_jac);
    return reserve(g, g->d_div, (size_t)C * N);
  };
  k.layout = [&](const WfSlots& sl, int E) -> int {
    WfGradLayoutArgs la{};
    la.sl = sl;
    la.ws = h->d_ws; la.wd = h->d_wd; la.wind_stride = wind_stride; la.N = N;
    la.h = g->step; la.lo = g->lo; la.hi = g->hi;
    la.yaw_in = d_yaw_in ? d_yaw_in + (size_t)sl.base * N : nullptr; la.yaw = b.d_yaw;
    la.ews = b.d_wind; la.ewd = b.d_wind + E; la.d = g->d_div;
    WFX_HIP(g, wfk_launch_grad_layout(&la, h->stream));
    return WF_OK;
  };
  k.reduce = [&](const WfSlots& sl, int) -> int {
    const size_t off = (size_t)sl.base * N;
    WfGradReduceArgs ra{};
    ra.n_slots = sl.n_slots; ra.N = N; ra.power_ev = b.d_pow; ra.d = g->d_div;
    ra.cot = d_cot ? d_cot + off : nullptr;
    ra.power = d_power ? d_power + off : nullptr;
    ra.gradient = d_grad ? d_grad + off : nullptr;
    ra.jacobian = d_jac ? d_jac + off * N : nullptr;
    WFX_HIP(g, wfk_launch_grad_reduce(&ra, h->stream));
    return WF_OK;
  };
  return run_rows(g, b, g->eval, k, st, &n_farms, farms);
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
