// wf_calib_abi.hip — the C boundary of the calib extension (include/wfcalib.h): an object that belongs to a parent handle, owns
// an evaluator handle WITH PARAMETER SETS and its device buffers, and enqueues a whole scoring or fitting run on the parent's
// stream.  The run is the extensions' shared row driver's (ext/wf_ext.h: run_rows — checks, chunks of S C rows per problem, the
// evaluator and its steps, events) with by_farm off and I rounds per chunk: this file supplies its own checks, gives the
// evaluator its sets (every one the parent's model: the host code then fills what a set does not own) and fetches the device
// table the kernel writes into (modelset/wf_modelset.h: modelset_device_table), and supplies the I + 1 launches of the one
// kernel (wf_calib_kernels.hip) as the driver's lay-out, advance and reduce.  What the launches of a run share goes to the
// device once, before the first of them (WfCalibRun).  Reads the parent (layout, model, kernel choice); stores nothing in it.
#include <cmath>
#include <vector>

#include "../../../include/wfcalib.h"
#include "../ext/wf_ext.h"
#include "../modelset/wf_modelset.h"
#include "wf_calib.h"

using namespace wfi;

static_assert(WF_CALIB_FIELDS == 18, "wf_model_set has eighteen fields (include/wfmodelset.h)");

struct wf_calib : ext_base {
  // configuration
  int max_eval = 65536;
  // the evaluator's sets were given for these S and C (its msets.size() tells the slots)
  int ev_S = 0, ev_C = 0;
  // device buffers (grow-only)
  row_batch rows;                // E = Cs S C farms
  dev_buf<wf_model_set> d_sets;  // the caller's sets (score) or starting sets (fit) ...
  std::vector<wf_model_set> sets_host;  // ... their host copy: the upload reads it
  dev_buf<wf_model_set> d_cand;  // [Cs][S] the candidates of an iteration, kept from its lay-out to its reduce
  dev_buf<double> d_row_loss;    // [E]
  dev_buf<WfCalibSlot> d_state;  // [Cs]
  dev_buf<float> d_fit_rows;     // [Cs][C][N] the best set's rows
  dev_buf<char> d_stage;         // staging for host callers: the observations and the outputs
  dev_buf<WfCalibRun> d_run;     // what the launches of a run share ...
  WfCalibRun run{};              // ... its host copy: the upload reads it ...
  hipEvent_t run_read = nullptr;  // ... and has done so, and read sets_host, when this event is reached
  evaluator eval;
  ~wf_calib() { if (run_read) hipEventDestroy(run_read); }
};

namespace {

const char* const kRowsMsg = "max_eval_farms must hold one problem's rows: at least S C";

// one call's arguments: wf_calib_score and wf_calib_fit fill it
struct calib_call {
  int G, C, S, E, I, fit;
  const double* sigma;
  unsigned long long seed;
  const double *lo, *hi;
  const wf_model_set* sets;  // HOST: score [G][S] or [S]; fit [G], [1] or null
  int per_problem;
  const double *ws, *wd;
  const float* yaw;
  const double *power, *weight;
  double scale;
  double* loss; int* best; float* row_power;
  wf_model_set *best_set, *mean;
  double *best_loss, *init_loss, *history;
  float* fit_power;
  int* n_invalid;
  int on_device;
  const char* name;
};

bool all_finite(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

int calib_run(wf_calib* p, const calib_call& q) {
  if (!p) return WF_E_INVALID;
  wf_handle* h = p->h;
  const int N = h->N, G = q.G, C = q.C, S = q.S, I = q.I;
  row_batch& b = p->rows;
  const double *d_ws = nullptr, *d_wd = nullptr, *d_power = nullptr, *d_weight = nullptr;
  const float* d_yaw = nullptr;
  double *d_loss = nullptr, *d_bl = nullptr, *d_il = nullptr, *d_hist = nullptr;
  int *d_best = nullptr, *d_ninv = nullptr;
  float *d_rp = nullptr, *d_fp = nullptr;
  wf_model_set *d_bs = nullptr, *d_mean = nullptr;
  std::vector<double> sg;  // the caller's sigma, copied: a launch takes its entry by value
  staging st(p, p->d_stage, q.on_device);
  bool uploaded = false;
  int n_items = G, n_sets = 0;
  wf_model_set model_set{};
  WfResolveConsts* tab = nullptr;
  row_policy k;
  k.what = "calibration serves"; k.name = nullptr;  // (no wind of the parent's is needed)
  k.rows_msg = kRowsMsg; k.by_farm = false;
  k.strict = 1;  // (an evaluator that holds sets solves every row in float64, and refuses any other mode)
  k.max_eval = p->max_eval;
  k.check = [&]() -> int {
    const std::string nm = q.name;
    if (G < 1) return ext_fail(p, WF_E_INVALID, nm + ": the number of problems G must be >= 1");
    if (C < 1) return ext_fail(p, WF_E_INVALID, nm + ": the number of conditions C must be >= 1");
    if (q.fit && S < WF_CALIB_MIN_S)
      return ext_fail(p, WF_E_INVALID, "the number of candidates S must be >= 3 (the best so far, the mean, a draw)");
    if (S < 1 || S > WF_CALIB_MAX_S) return ext_fail(p, WF_E_INVALID, "the number of candidates S must be in 1..1024");
    if ((long long)S * C > p->max_eval) return ext_fail(p, WF_E_INVALID, kRowsMsg);
    if (!q.ws || !q.wd || !q.yaw || !q.power) return ext_fail(p, WF_E_INVALID, nm + ": ws, wd, yaw or power is NULL");
    if (!std::isfinite(q.scale) || !(q.scale > 0.0)) return ext_fail(p, WF_E_INVALID, "scale must be finite and > 0 (watts)");
    wf_model_set_from_model(h, &model_set);
    std::string why;
    if (q.fit) {
      if (q.E < 1 || q.E > S) return ext_fail(p, WF_E_INVALID, "the number of elites E must be in 1..S");
      if (I < 1 || I > WF_CALIB_MAX_ITER) return ext_fail(p, WF_E_INVALID, "the number of iterations I must be in 1..16");
      if (!q.sigma) return ext_fail(p, WF_E_INVALID, nm + ": sigma is NULL");
      for (int i = 0; i < I; ++i)
        if (!std::isfinite(q.sigma[i]) || q.sigma[i] < 0.0) return ext_fail(p, WF_E_INVALID, "every sigma must be finite and non-negative");
      if (!q.lo || !q.hi) return ext_fail(p, WF_E_INVALID, nm + ": lo or hi is NULL");
      for (int f = 0; f < WF_CALIB_FIELDS; ++f)
        if (!std::isfinite(q.lo[f]) || !std::isfinite(q.hi[f]) || q.lo[f] > q.hi[f])
          return ext_fail(p, WF_E_INVALID, "bounds: lo and hi must be finite with lo <= hi, field " + std::to_string(f));
      n_sets = q.sets && q.per_problem ? G : 1;
      const wf_model_set* init = q.sets ? q.sets : &model_set;
      if (!modelset_validate(init, n_sets, &why)) return ext_fail(p, WF_E_INVALID, "init: " + why);
      for (int g = 0; g < n_sets; ++g) {
        const double* x = reinterpret_cast<const double*>(init + g);
        for (int f = 0; f < WF_CALIB_FIELDS; ++f)
          if (x[f] < q.lo[f] || x[f] > q.hi[f])
            return ext_fail(p, WF_E_INVALID, "init: starting set " + std::to_string(g) + " is outside the bounds [lo, hi] in field " + std::to_string(f));
      }
      sg.assign(q.sigma, q.sigma + I);
    } else {
      if (!q.sets) return ext_fail(p, WF_E_INVALID, nm + ": sets is NULL");
      n_sets = q.per_problem ? G * S : S;
      if (!modelset_validate(q.sets, n_sets, &why)) return ext_fail(p, WF_E_INVALID, why);
    }
    if (!q.on_device) {  // a host caller's observations are read here; a device caller's are not
      const size_t gc = (size_t)G * C;
      if (!all_finite(q.ws, gc) || !all_finite(q.wd, gc)) return ext_fail(p, WF_E_INVALID, "observations: a wind speed or direction is not finite");
      for (size_t i = 0; i < gc * N; ++i)  // (under a weight of 0 anything may stand: an off-line turbine recorded as NaN)
        if (!std::isfinite(q.power[i]) && !(q.weight && q.weight[i] == 0.0))
          return ext_fail(p, WF_E_INVALID, "observations: a measured power is not finite (and its weight is not 0)");
      for (size_t i = 0; i < gc * N; ++i)
        if (!std::isfinite(q.yaw[i])) return ext_fail(p, WF_E_INVALID, "observations: a yaw is not finite");
      if (q.weight)
        for (size_t i = 0; i < gc * N; ++i)
          if (!std::isfinite(q.weight[i]) || q.weight[i] < 0.0) return ext_fail(p, WF_E_INVALID, "weight must be finite and >= 0");
    }
    k.rows = S * C; k.rounds = I;
    return WF_OK;
  };
  k.reserve = [&](int Cs, int Ev) -> int {
    // the evaluator's sets: Cs S copies of the parent's model, row (slot, s, c) on set slot S + s — given once per evaluator
    wf_handle* ev = p->eval.ev;
    if ((int)ev->msets.size() != Cs * S || p->ev_S != S || p->ev_C != C) {
      const std::vector<wf_model_set> sets((size_t)Cs * S, model_set);
      std::vector<int> of((size_t)Ev);
      for (int r = 0; r < Ev; ++r) of[(size_t)r] = r / C;
      WFX_EV(p, ev, wf_set_model_sets(ev, Cs * S, sets.data(), of.data()));
      p->ev_S = S; p->ev_C = C;
    }
    WFX_EV(p, ev, modelset_device_table(ev, &tab));  // (uploads a stale table: the members a set does not own)
    int rc = reserve(p, p->d_sets, (size_t)n_sets);
    if (rc == WF_OK) rc = reserve(p, p->d_cand, (size_t)Cs * S);
    if (rc == WF_OK) rc = reserve(p, p->d_row_loss, (size_t)Ev);
    if (rc == WF_OK) rc = reserve(p, p->d_state, (size_t)Cs);
    if (rc == WF_OK) rc = reserve(p, p->d_fit_rows, (size_t)Cs * C * N);
    if (rc == WF_OK) rc = reserve(p, p->d_run, 1);
    if (rc != WF_OK) return rc;
    const size_t gc = (size_t)G * C;
    st.in(q.ws, gc, &d_ws); st.in(q.wd, gc, &d_wd); st.in(q.yaw, gc * N, &d_yaw);
    st.in(q.power, gc * N, &d_power); st.in(q.weight, gc * N, &d_weight);
    st.out(q.loss, (size_t)G * S, &d_loss); st.out(q.best, (size_t)G, &d_best); st.out(q.row_power, (size_t)G * S * C * N, &d_rp);
    st.out(q.best_set, (size_t)G, &d_bs); st.out(q.best_loss, (size_t)G, &d_bl); st.out(q.init_loss, (size_t)G, &d_il);
    st.out(q.history, (size_t)G * I, &d_hist); st.out(q.mean, (size_t)G, &d_mean); st.out(q.fit_power, gc * N, &d_fp);
    st.out(q.n_invalid, (size_t)G, &d_ninv);
    return WF_OK;
  };
  // the run's block and the sets, once the staging has given the caller's arrays their device pointers: before the first launch
  auto upload = [&](int Ev) -> int {
    if (!p->run_read) WFX_HIP(p, hipEventCreateWithFlags(&p->run_read, hipEventDisableTiming));
    else WFX_HIP(p, hipEventSynchronize(p->run_read));  // (the previous run's uploads have read the host copies)
    const wf_model_set* src = q.sets ? q.sets : &model_set;
    p->sets_host.assign(src, src + n_sets);
    WFX_HIP(p, hipMemcpyAsync(p->d_sets, p->sets_host.data(), sizeof(wf_model_set) * (size_t)n_sets, hipMemcpyHostToDevice, h->stream));
    WfCalibRun& r = p->run;
    r = WfCalibRun{};
    r.N = N; r.S = S; r.C = C; r.E = q.fit ? q.E : 1; r.I = I; r.fit = q.fit;
    r.sets_stride = q.sets && q.per_problem ? (q.fit ? 1 : S) : 0;
    r.scale = q.scale; r.kappa = h->model.kappa; r.seed = q.seed;
    for (int f = 0; f < WF_CALIB_FIELDS; ++f) { r.lo[f] = q.fit ? q.lo[f] : 0.0; r.hi[f] = q.fit ? q.hi[f] : 0.0; }
    r.sets = p->d_sets;
    r.ws = d_ws; r.wd = d_wd; r.yaw = d_yaw; r.power = d_power; r.weight = d_weight;
    r.yaw_ev = b.d_yaw; r.ews = b.d_wind; r.ewd = b.d_wind + Ev; r.power_ev = b.d_pow; r.tab = tab;
    r.cand = p->d_cand; r.row_loss = p->d_row_loss; r.state = p->d_state; r.fit_rows = p->d_fit_rows;
    r.loss = d_loss; r.best = d_best; r.row_power = d_rp;
    r.best_set = d_bs; r.mean = d_mean; r.best_loss = d_bl; r.init_loss = d_il; r.history = d_hist; r.fit_power = d_fp;
    r.n_invalid = d_ninv;
    WFX_HIP(p, hipMemcpyAsync(p->d_run, &r, sizeof(WfCalibRun), hipMemcpyHostToDevice, h->stream));
    WFX_HIP(p, hipEventRecord(p->run_read, h->stream));
    uploaded = true;
    return WF_OK;
  };
  // launch v of a chunk: the driver's lay-out is v = 0, its advance of round r is v = r, its reduce is v = I
  auto launch = [&](const WfSlots& sl, int Ev, int v) -> int {
    if (!uploaded) {
      const int rc = upload(Ev);
      if (rc != WF_OK) return rc;
    }
    // (the kernel writes into the table the evaluator's steps read: nothing may have marked it for a rebuild from the host sets)
    if (p->eval.ev->model_dirty || p->eval.ev->msets_dirty)
      return ext_fail(p, WF_E_INVALID, std::string(q.name) + ": the evaluator's table of constants went stale during the run");
    WFX_HIP(p, wfk_launch_calib_advance(&p->run, p->d_run, &sl, v, q.fit && v < I ? sg[(size_t)v] : 0.0, h->stream));
    return WF_OK;
  };
  k.layout = [&](const WfSlots& sl, int Ev) -> int { return launch(sl, Ev, 0); };
  k.advance = [&](const WfSlots& sl, int Ev, int r) -> int { return launch(sl, Ev, r); };
  k.reduce = [&](const WfSlots& sl, int Ev) -> int { return launch(sl, Ev, I); };
  return run_rows(p, b, p->eval, k, st, &n_items, nullptr);
}

}  // namespace

extern "C" {

int wf_calib_create(wf_handle* h, wf_calib** out) { return ext_create(h, out); }

int wf_calib_destroy(wf_calib* p) { return ext_destroy(p); }

int wf_calib_config(wf_calib* p, int max_eval_farms) {
  if (!p) return WF_E_INVALID;
  p->max_eval = max_eval_farms <= 0 ? 65536 : max_eval_farms;
  return WF_OK;
}

int wf_calib_set_timing(wf_calib* p, int detail) {
  if (!p) return WF_E_INVALID;
  p->detail = detail != 0;
  return WF_OK;
}

int wf_calib_score(wf_calib* p, int G, int C, int S, const wf_model_set* sets, int per_problem, const double* ws, const double* wd,
                   const float* yaw, const double* power, const double* weight, double scale, double* loss, int* best,
                   float* row_power, int on_device) {
  calib_call q{};
  q.G = G; q.C = C; q.S = S; q.E = 1; q.I = 1; q.fit = 0;
  q.sets = sets; q.per_problem = per_problem;
  q.ws = ws; q.wd = wd; q.yaw = yaw; q.power = power; q.weight = weight; q.scale = scale;
  q.loss = loss; q.best = best; q.row_power = row_power;
  q.on_device = on_device; q.name = "wf_calib_score";
  return calib_run(p, q);
}

int wf_calib_fit(wf_calib* p, int G, int C, int S, int E, int I, const double* sigma, unsigned long long seed, const double* lo,
                 const double* hi, const wf_model_set* init, int init_per_problem, const double* ws, const double* wd,
                 const float* yaw, const double* power, const double* weight, double scale, wf_model_set* best_set,
                 double* best_loss, double* init_loss, double* history, wf_model_set* mean, float* fit_power, int* n_invalid,
                 int on_device) {
  calib_call q{};
  q.G = G; q.C = C; q.S = S; q.E = E; q.I = I; q.fit = 1;
  q.sigma = sigma; q.seed = seed; q.lo = lo; q.hi = hi;
  q.sets = init; q.per_problem = init_per_problem;
  q.ws = ws; q.wd = wd; q.yaw = yaw; q.power = power; q.weight = weight; q.scale = scale;
  q.best_set = best_set; q.best_loss = best_loss; q.init_loss = init_loss; q.history = history; q.mean = mean;
  q.fit_power = fit_power; q.n_invalid = n_invalid;
  q.on_device = on_device; q.name = "wf_calib_fit";
  return calib_run(p, q);
}

// with detail, per chunk: e0 | launch 0 e1 | wind + step e2 | launch 1 e3 | step e4 | ... | launch I e
int wf_calib_last_timing(wf_calib* p, float* total_ms, float* step_ms, float* glue_ms) {
  if (!p) return WF_E_INVALID;
  return last_timing(p, "neither wf_calib_score nor wf_calib_fit has run yet", total_ms, step_ms, glue_ms);
}

wf_handle* wf_calib_evaluator(wf_calib* p) { return p ? p->eval.ev : nullptr; }

int wf_calib_kernel_info(wf_calib* p, int* info) {
  if (!p || !info) return ext_fail(p, WF_E_INVALID, "wf_calib_kernel_info: NULL argument");
  return kernel_info(p, WF_CALIB_KERNELS, wfk_calib_func_attributes, info);
}

const char* wf_calib_last_error(wf_calib* p) { return p ? p->err.c_str() : "wf_calib: NULL object"; }

}  // extern "C"
