// wf_ext.hip — the non-template parts of the extensions' shared host layer (wf_ext.h).
#include "wf_ext.h"

namespace wfi {

ext_base::~ext_base() {
  for (hipEvent_t e : ev_pool) hipEventDestroy(e);
}

namespace {

bool same_model(const wf_model_params& a, const wf_model_params& b) {  // (the tables are compared through the handle's vectors)
  return std::memcmp(&a, &b, offsetof(wf_model_params, n_table)) == 0 && a.n_table == b.n_table &&
         a.enable_secondary_steering == b.enable_secondary_steering && a.enable_yaw_added_recovery == b.enable_yaw_added_recovery &&
         a.enable_transverse_velocities == b.enable_transverse_velocities;
}

}  // namespace

int ensure_evaluator(ext_base* x, evaluator& s, int E, int mode) {
  wf_handle* h = x->h;
  const size_t n = (size_t)h->N;
  const bool same = s.ev && s.E == E && same_model(s.model, h->model) && s.tws == h->tws && s.tct == h->tct && s.tcp == h->tcp &&
                    s.lx.size() == n && std::equal(s.lx.begin(), s.lx.end(), h->lx.begin()) &&
                    std::equal(s.ly.begin(), s.ly.end(), h->ly.begin()) &&
                    std::memcmp(&s.choice, &h->choice, sizeof(wf_kernel_choice)) == 0 && s.own_stage == h->own_stage && s.guard == h->guard_rel;
  if (same) {
    if (s.stream != h->stream) {
      WFX_EV(x, s.ev, wf_set_stream(s.ev, (void*)h->stream, 1));
      s.stream = h->stream;
    }
    if (s.mode != mode) {
      WFX_EV(x, s.ev, wf_set_risk_resolve(s.ev, mode));
      s.mode = mode;
    }
    return WF_OK;
  }
  WFX_HIP(x, hipStreamSynchronize(h->stream));
  if (s.ev) wf_destroy(s.ev);
  s.ev = nullptr;
  wf_handle* ev = nullptr;
  if (wf_create(h->device, &ev) != WF_OK) return ext_fail(x, WF_E_HIP, std::string("evaluator: ") + wf_last_error(nullptr));
  s.ev = ev;
  wf_model_params m = h->model;
  m.table_ws = h->tws.data(); m.table_ct = h->tct.data(); m.table_cp = h->tcp.data();
  WFX_EV(x, ev, wf_set_stream(ev, (void*)h->stream, 1));
  WFX_EV(x, ev, wf_set_model(ev, &m));
  WFX_EV(x, ev, wf_set_kernel_choice(ev, &h->choice));
  WFX_EV(x, ev, wf_set_own_stage(ev, h->own_stage));
  if (h->guard_user) WFX_EV(x, ev, wf_set_risk_guard(ev, h->guard_rel));
  WFX_EV(x, ev, wf_set_layout(ev, h->N, h->lx.data(), h->ly.data()));
  WFX_EV(x, ev, wf_set_batch(ev, E));
  WFX_EV(x, ev, wf_set_risk_resolve(ev, mode));
  s.E = E; s.mode = mode; s.stream = h->stream;
  s.model = h->model; s.tws = h->tws; s.tct = h->tct; s.tcp = h->tcp;
  s.lx.assign(h->lx.begin(), h->lx.begin() + n); s.ly.assign(h->ly.begin(), h->ly.begin() + n);
  s.choice = h->choice; s.own_stage = h->own_stage; s.guard = h->guard_rel;
  return WF_OK;
}

int check_wind(ext_base* x, const char* call) {
  if (x->h->wind_count == 0)
    return ext_fail(x, WF_E_INVALID, std::string("no wind has been set: wf_set_wind (or wf_wind_*) must be called before ") + call);
  return WF_OK;
}

int check_parent(ext_base* x, const char* what, const char* call) {
  wf_handle* h = x->h;
  if (h->N <= 0 || h->B <= 0) return ext_fail(x, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return ext_fail(x, WF_E_UNSUPPORTED, std::string(what) + " a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return ext_fail(x, WF_E_UNSUPPORTED, std::string(what) + " one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  if (!h->msets.empty())
    return ext_fail(x, WF_E_UNSUPPORTED, std::string(what) + " one wake model: this handle holds wake-model parameter sets per farm (wf_set_model_sets)");
  return call ? check_wind(x, call) : WF_OK;
}

int check_farms(ext_base* x, int* n_farms, const int* farms) {
  if (!farms) {
    *n_farms = x->h->B;
    return WF_OK;
  }
  if (*n_farms < 1) return ext_fail(x, WF_E_INVALID, "n_farms must be >= 1");
  for (int k = 0; k < *n_farms; ++k)
    if (farms[k] < 0 || farms[k] >= x->h->B) return ext_fail(x, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  return WF_OK;
}

int upload_farms(ext_base* x, farm_list& fl, const int* farms, int n_farms) {
  WFX_HIP(x, hipStreamSynchronize(x->h->stream));
  fl.host.assign(farms, farms + n_farms);
  WFX_HIP(x, hipMemcpyAsync(fl.d, fl.host.data(), sizeof(int) * n_farms, hipMemcpyHostToDevice, x->h->stream));
  return WF_OK;
}

int staging::begin() {
  const int rc = reserve(x, buf, total);
  if (rc != WF_OK) return rc;
  for (int i = 0; i < n_segs; ++i) {
    const seg& s = segs[i];
    s.set(s.d, buf.p + s.off);
    if (s.src) WFX_HIP(x, hipMemcpyAsync(buf.p + s.off, s.src, s.bytes, hipMemcpyHostToDevice, x->h->stream));
  }
  return WF_OK;
}

int staging::end() {
  if (!host) return WF_OK;
  for (int i = 0; i < n_segs; ++i)
    if (segs[i].user) WFX_HIP(x, hipMemcpyAsync(segs[i].user, buf.p + segs[i].off, segs[i].bytes, hipMemcpyDeviceToHost, x->h->stream));
  WFX_HIP(x, hipStreamSynchronize(x->h->stream));
  return WF_OK;
}

int record(ext_base* x) {
  if (x->n_ev == x->ev_pool.size()) {
    hipEvent_t e = nullptr;
    WFX_HIP(x, hipEventCreate(&e));
    x->ev_pool.push_back(e);
  }
  WFX_HIP(x, hipEventRecord(x->ev_pool[x->n_ev++], x->h->stream));
  return WF_OK;
}

int last_timing(ext_base* x, const char* not_run, float* total_ms, float* step_ms, float* glue_ms) {
  if (!x->timed || x->n_ev < 2) return ext_fail(x, WF_E_INVALID, not_run);
  WFX_ON_DEVICE(x);
  WFX_HIP(x, hipEventSynchronize(x->ev_pool[x->n_ev - 1]));
  float total = 0.0f, step = 0.0f, glue = 0.0f;
  WFX_HIP(x, hipEventElapsedTime(&total, x->ev_pool[0], x->ev_pool[x->n_ev - 1]));
  for (size_t k = 1; x->per_chunk && k < x->n_ev; ++k) {
    float ms = 0.0f;
    WFX_HIP(x, hipEventElapsedTime(&ms, x->ev_pool[k - 1], x->ev_pool[k]));
    const size_t q = k % x->per_chunk;
    if (q != 0 && q % 2 == 0) step += ms;
    else glue += ms;
  }
  if (total_ms) *total_ms = total;
  if (step_ms) *step_ms = step;
  if (glue_ms) *glue_ms = glue;
  return WF_OK;
}

int kernel_info(ext_base* x, int n, hipError_t (*attributes)(int, hipFuncAttributes*), int* info) {
  WFX_ON_DEVICE(x);
  for (int k = 0; k < n; ++k) {
    hipFuncAttributes a{};
    WFX_HIP(x, attributes(k, &a));
    info[3 * k] = a.numRegs; info[3 * k + 1] = (int)a.sharedSizeBytes; info[3 * k + 2] = (int)a.localSizeBytes;
  }
  return WF_OK;
}

int run_rows(ext_base* x, row_batch& b, evaluator& es, row_policy& k, staging& st, int* n_items, const int* farms) {
  wf_handle* h = x->h;
  int rc = check_parent(x, k.what, k.name);
  if (rc != WF_OK) return rc;
  if (k.rows <= 0) return ext_fail(x, WF_E_INVALID, k.no_rows);
  if (k.by_farm && (rc = check_farms(x, n_items, farms)) != WF_OK) return rc;
  if (k.check && (rc = k.check()) != WF_OK) return rc;
  const int N = h->N, R = k.rows, n = *n_items;
  if (k.max_eval < R) return ext_fail(x, WF_E_INVALID, k.rows_msg);
  WFX_ON_DEVICE(x);
  int C = k.max_eval / R;
  if (C > n) C = n;
  const int E = C * R;
  if ((rc = ensure_evaluator(x, es, E, k.strict ? 2 : h->resolve_mode)) != WF_OK) return rc;
  const size_t en = (size_t)E * N;
  rc = reserve(x, b.d_yaw, en);
  if (rc == WF_OK) rc = reserve(x, b.d_pow, en);
  if (rc == WF_OK && k.loads) rc = reserve(x, b.d_load, 4 * en);
  if (rc == WF_OK && k.local_wind) rc = reserve(x, b.d_lws, en);
  if (rc == WF_OK && k.local_wind) rc = reserve(x, b.d_lwd, en);
  if (rc == WF_OK) rc = reserve(x, b.d_wind, 2 * (size_t)E);
  if (rc == WF_OK && farms) rc = reserve(x, b.farms.d, (size_t)n);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(x, b.farms, farms, n)) != WF_OK) return rc;
  if ((rc = k.reserve(C, E)) != WF_OK || (rc = st.begin()) != WF_OK) return rc;
  const bool split = k.split_always || x->detail != 0;
  x->n_ev = 0; x->timed = false;
  for (int first = 0; first < n; first += C) {
    const WfSlots sl = chunk_slots(b.farms, farms, first, n, C);
    if (first == 0 || split) { rc = record(x); if (rc != WF_OK) return rc; }  // (split: four events per chunk)
    if ((rc = k.layout(sl, E)) != WF_OK) return rc;
    if (split) { rc = record(x); if (rc != WF_OK) return rc; }
    WFX_EV(x, es.ev, wf_set_wind_counts(es.ev, b.d_wind, E, b.d_wind + E, E, 1));
    float* const lws = k.local_wind ? b.d_lws.p : nullptr;
    float* const lwd = k.local_wind ? b.d_lwd.p : nullptr;
    WFX_EV(x, es.ev, wf_step(es.ev, b.d_yaw, b.d_pow, lws, lwd, k.loads ? b.d_load.p : nullptr, 1));
    if (split) { rc = record(x); if (rc != WF_OK) return rc; }
    for (int r = 1; r < k.rounds; ++r) {  // (the rows' wind stays what the lay-out wrote, unless the advance hook itself sets another)
      if ((rc = k.advance(sl, E, r)) != WF_OK) return rc;
      if (split) { rc = record(x); if (rc != WF_OK) return rc; }
      WFX_EV(x, es.ev, wf_step(es.ev, b.d_yaw, b.d_pow, lws, lwd, k.loads ? b.d_load.p : nullptr, 1));
      if (split) { rc = record(x); if (rc != WF_OK) return rc; }
    }
    if ((rc = k.reduce(sl, E)) != WF_OK) return rc;
    if (split) { rc = record(x); if (rc != WF_OK) return rc; }
  }
  if (!split) { rc = record(x); if (rc != WF_OK) return rc; }
  x->timed = true; x->per_chunk = split ? 2 * (size_t)k.rounds + 2 : 0;
  if (k.finish && (rc = k.finish()) != WF_OK) return rc;
  return st.end();
}

int set_search_config(ext_base* x, search_config& c, double lo, double hi, int n_passes, const int* K, int strict, int max_eval_farms,
                      int rows_per_candidate, const char* rows_msg) {
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return ext_fail(x, WF_E_INVALID, "yaw bounds must be finite with lo < hi");
  if (n_passes < 1 || n_passes > WF_SEARCH_MAX_PASSES) return ext_fail(x, WF_E_INVALID, "the number of passes must be in 1..4");
  if (K[0] < 2 || K[0] > WF_SEARCH_MAX_K0) return ext_fail(x, WF_E_INVALID, "the first pass needs 2..31 candidates (K_0)");
  for (int p = 1; p < n_passes; ++p)
    if (K[p] < 1 || K[p] > WF_SEARCH_MAX_K) return ext_fail(x, WF_E_INVALID, "a refining pass needs 1..15 candidates (K_p)");
  if (max_eval_farms <= 0) max_eval_farms = 65536;
  if (max_eval_farms < (k_max(n_passes, K) + 1) * rows_per_candidate) return ext_fail(x, WF_E_INVALID, rows_msg);
  c.lo = lo; c.hi = hi; c.P = n_passes;
  for (int p = 0; p < WF_SEARCH_MAX_PASSES; ++p) c.K[p] = p < n_passes ? K[p] : 0;
  c.strict = strict != 0; c.max_eval = max_eval_farms;
  return WF_OK;
}

int k_max(int P, const int* K) {
  int k = 0;
  for (int p = 0; p < P; ++p) k = K[p] > k ? K[p] : k;
  return k;
}

void pass_grids(double lo, double hi, int P, const int* K, WfGrid* grid) {
  double hp = (hi - lo) / (double)(K[0] - 1);
  grid[0] = WfGrid{0, 0, K[0], lo, hp};
  for (int p = 1; p < P; ++p) {
    const double s = 2.0 * hp / (double)(K[p] + 1);
    grid[p] = WfGrid{0, 1, K[p], hp, s};
    hp = s;
  }
}

int run_search(ext_base* x, yaw_search& s, evaluator& es, const search_policy& k, const float* yaw0, int n_farms, const int* farms,
               float* yaw_opt, float* power_opt, float* power_init, int on_device) {
  wf_handle* h = x->h;
  const search_config& cf = s.cfg;
  int rc = check_parent(x, k.what, k.name);
  if (rc != WF_OK) return rc;
  if (k.rows_per_candidate <= 0) return ext_fail(x, WF_E_INVALID, k.no_rows);
  if ((rc = check_farms(x, &n_farms, farms)) != WF_OK) return rc;
  const int N = h->N, R = k_max(cf.P, cf.K) + 1, rows = R * k.rows_per_candidate;
  if (cf.max_eval < rows) return ext_fail(x, WF_E_INVALID, k.rows_msg);
  WFX_ON_DEVICE(x);
  int C = cf.max_eval / rows;
  if (C > n_farms) C = n_farms;
  const int E = C * rows;
  if ((rc = ensure_evaluator(x, es, E, cf.strict ? 2 : h->resolve_mode)) != WF_OK) return rc;
  const size_t en = (size_t)E * N, fn = (size_t)n_farms * N;
  rc = reserve(x, s.d_yaw, en);
  if (rc == WF_OK) rc = reserve(x, s.d_pow, en);
  if (rc == WF_OK) rc = k.reserve(E);
  if (rc == WF_OK) rc = reserve(x, s.d_best, (size_t)C * N);
  if (rc == WF_OK) rc = reserve(x, s.d_order, (size_t)C * N);
  if (rc == WF_OK && farms) rc = reserve(x, s.farms.d, (size_t)n_farms);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(x, s.farms, farms, n_farms)) != WF_OK) return rc;
  staging st(x, s.d_stage, on_device);
  const float* d_yaw0 = nullptr;
  float *d_oyaw = nullptr, *d_opow = nullptr, *d_oini = nullptr;
  st.in(yaw0, fn, &d_yaw0);
  st.out(yaw_opt, fn, &d_oyaw);
  st.out(power_opt, (size_t)n_farms, &d_opow);
  st.out(power_init, (size_t)n_farms, &d_oini);
  if ((rc = st.begin()) != WF_OK) return rc;

  WfGrid grid[WF_SEARCH_MAX_PASSES];
  pass_grids(cf.lo, cf.hi, cf.P, cf.K, grid);
  const WfGrid none{-1, 0, 0, 0.0, 0.0};
  const int V = cf.P * N;  // visits
  x->n_ev = 0; x->timed = false;
  const bool detail = x->detail != 0;
  for (int base = 0; base < n_farms; base += C) {
    if (base == 0 || detail) { rc = record(x); if (rc != WF_OK) return rc; }  // (detail: 2 V + 2 events per chunk)
    WfAdvanceArgs aa{};
    aa.sl = chunk_slots(s.farms, farms, base, n_farms, C);
    if ((rc = k.begin_chunk(aa.sl, R, E)) != WF_OK) return rc;
    aa.N = N; aa.R = R; aa.lo = cf.lo; aa.hi = cf.hi;
    aa.order = s.d_order; aa.yaw = s.d_yaw; aa.best = s.d_best;
    aa.yaw0 = d_yaw0 ? d_yaw0 + (size_t)base * N : nullptr;
    aa.out_yaw = d_oyaw + (size_t)base * N; aa.out_power = d_opow + base; aa.out_init = d_oini + base;
    for (int v = 0; v <= V; ++v) {  // launch v lays out visit v (v < V) from the powers of visit v - 1 (v > 0)
      aa.prev = none; aa.next = none;
      if (v > 0) { aa.prev = grid[(v - 1) / N]; aa.prev.s = (v - 1) % N; }
      if (v < V) { aa.next = grid[v / N]; aa.next.s = v % N; }
      aa.first = v == 1;
      if ((rc = k.visit(aa, v)) != WF_OK) return rc;
      if (detail) { rc = record(x); if (rc != WF_OK) return rc; }
      if (v < V) {
        WFX_EV(x, es.ev, wf_step(es.ev, s.d_yaw, s.d_pow, nullptr, nullptr, nullptr, 1));
        if (detail) { rc = record(x); if (rc != WF_OK) return rc; }
      }
    }
  }
  if (!detail) { rc = record(x); if (rc != WF_OK) return rc; }
  x->timed = true; x->per_chunk = detail ? 2 * (size_t)V + 2 : 0;
  return st.end();
}

}  // namespace wfi
