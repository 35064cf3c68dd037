// wf_modelset.hip — the host side of wake-model parameter sets per farm (include/wfmodelset.h): validation, storage in the
// handle, the device table of WfResolveConsts (one per set, built by wf_model.hip's fill_resolve_consts — the code behind
// h->rconsts) and the launch of the float64 kernels of wf_resolve_ms.hip / wf_resolve4_ms.hip behind every step.
#include <cmath>
#include <string>
#include <vector>

#include "../wf_handle.h"
#include "wf_modelset.h"

extern "C" hipError_t wfk_launch_resolve_ms(const WfResolveConsts* c, const WfResolveArgs* a, int B, int all, int* raw_flags, int n_cu,
                                            hipStream_t s, const WfResolveConsts* ms_sets, const int* ms_set_of);
extern "C" int wfk_resolve_ms_last_waves();

namespace {

#define WF_MS_FIELDS(X) \
  X(ambient_ti) X(shear) X(veer) X(alpha) X(beta) X(ka) X(kb) X(ad) X(bd) X(dm) X(ch_initial) X(ch_constant) X(ch_ai) X(ch_downstream) \
  X(defl_alpha) X(defl_beta) X(defl_ka) X(defl_kb)

wf_model_params with_set(wf_model_params m, const wf_model_set& s) {
#define X(f) m.f = s.f;
  WF_MS_FIELDS(X)
#undef X
  return m;
}

}  // namespace

namespace wfi {

int modelset_check(wf_handle* h) {
  if (h->mset_batch != h->B || (int)h->mset_of.size() != h->B)
    return fail(h, WF_E_INVALID, "wf_set_model_sets was given for another env_batch than the handle's: set the parameter sets again");
  return WF_OK;
}

void modelset_free(wf_handle* h) {
  hipFree(h->d_msets); hipFree(h->d_mset_of); hipFree(h->d_mset_type); hipFree(h->d_mset_type_of);
  h->d_msets = nullptr; h->d_mset_of = nullptr; h->d_mset_type = nullptr; h->d_mset_type_of = nullptr;
}

static int modelset_upload(wf_handle* h) {
  const int S = (int)h->msets.size(), N = h->N, B = h->B;
  const int n_table = (int)h->tws.size();
  std::vector<WfResolveConsts> tab((size_t)S);  // (value-initialised: the padding bytes too are those of h->rconsts)
  for (int k = 0; k < S; ++k) fill_resolve_consts(with_set(h->model, h->msets[(size_t)k]), N, n_table, &tab[(size_t)k]);
  // a handle without turbine definitions: its model as the one definition the kernels look up (wf_model.hip: type_consts)
  const wf_model_params& m = h->model;
  const double type1[1 + WF_TYPE_CONSTS] = {(double)n_table, 1.0 / m.tsr, m.pP / 3.0, std::pow(m.air_density / m.ref_density, 1.0 / 3.0),
                                            m.ref_density};
  const std::vector<int> zeros((size_t)N, 0);
  // (on the handle's stream and behind whatever still runs there, as the tables of wf_model.hip)
  WF_HIP(h, hipStreamSynchronize(h->stream));
  modelset_free(h);
  WF_HIP(h, hipMalloc(&h->d_msets, sizeof(WfResolveConsts) * (size_t)S));
  WF_HIP(h, hipMalloc(&h->d_mset_of, sizeof(int) * (size_t)B));
  WF_HIP(h, hipMalloc(&h->d_mset_type, sizeof(type1)));
  WF_HIP(h, hipMalloc(&h->d_mset_type_of, sizeof(int) * (size_t)N));
  WF_HIP(h, hipMemcpyAsync(h->d_msets, tab.data(), sizeof(WfResolveConsts) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  WF_HIP(h, hipMemcpyAsync(h->d_mset_of, h->mset_of.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
  WF_HIP(h, hipMemcpyAsync(h->d_mset_type, type1, sizeof(type1), hipMemcpyHostToDevice, h->stream));
  WF_HIP(h, hipMemcpyAsync(h->d_mset_type_of, zeros.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, h->stream));
  WF_HIP(h, hipStreamSynchronize(h->stream));
  h->msets_dirty = false;
  return WF_OK;
}

bool modelset_validate(const wf_model_set* sets, int n, std::string* why) {
  for (int k = 0; k < n; ++k) {
    const wf_model_set& s = sets[k];
#define X(f) if (!std::isfinite(s.f)) { *why = "parameter set " + std::to_string(k) + ": " #f " is not finite"; return false; }
    WF_MS_FIELDS(X)
#undef X
    if (!(s.ambient_ti > 0.0)) { *why = "parameter set " + std::to_string(k) + ": ambient_ti must be > 0"; return false; }
    const struct { double v; const char* name; } positive[] = {  // what wf_set_model asks of these fields
        {s.alpha, "alpha"}, {s.defl_alpha, "deflection alpha"}, {s.ka * s.ambient_ti + s.kb, "ka*TI + kb"},
        {s.defl_ka * s.ambient_ti + s.defl_kb, "deflection ka*TI + kb"}, {s.ch_constant, "crespo_hernandez.constant"}};
    for (const auto& q : positive)
      if (!(q.v > 0.0)) { *why = "parameter set " + std::to_string(k) + ": must be > 0: " + q.name; return false; }
  }
  return true;
}

int modelset_device_table(wf_handle* h, WfResolveConsts** tab) {
  int rc = modelset_check(h);
  if (rc != WF_OK) return rc;
  // (what a step does first: the model's own constants — building them marks the sets' table stale, so a table handed out before
  // them would be built over again by the first step)
  if (h->model_dirty && h->N > 0 && (rc = build_consts(h)) != WF_OK) return rc;
  if (h->msets_dirty || !h->d_msets) {
    if ((rc = modelset_upload(h)) != WF_OK) return rc;
  }
  *tab = h->d_msets;
  return WF_OK;
}

int modelset_launch(wf_handle* h, WfResolveArgs* ra) {
  int rc = modelset_check(h);
  if (rc != WF_OK) return rc;
  if (h->msets_dirty || !h->d_msets) {
    if ((rc = modelset_upload(h)) != WF_OK) return rc;
  }
  if (!h->types.empty()) {
    ra->tab64 = h->d_tab64_mt; ra->n_types = (int)h->types.size(); ra->type_of = h->d_type_of; ra->type_consts = h->d_type_consts;
  } else {  // (d_tab64 is [3][WF_TABLE_PAD]: the table of definition 0)
    ra->tab64 = h->d_tab64; ra->n_types = 1; ra->type_of = h->d_mset_type_of; ra->type_consts = h->d_mset_type;
  }
  WF_HIP(h, wfk_launch_resolve_ms(&h->rconsts, ra, h->B, 1, h->d_flags_raw, h->n_cu, h->stream, h->d_msets, h->d_mset_of));
  h->mset_waves = wfk_resolve_ms_last_waves();
  return WF_OK;
}

}  // namespace wfi

using namespace wfi;

extern "C" {

int wf_model_set_from_model(wf_handle* h, wf_model_set* out) {
  if (!h || !out) return WF_E_INVALID;
#define X(f) out->f = h->model.f;
  WF_MS_FIELDS(X)
#undef X
  return WF_OK;
}

int wf_set_model_sets(wf_handle* h, int n_sets, const wf_model_set* sets, const int* set_of) {
  if (!h) return WF_E_INVALID;
  if (n_sets == 0) {  // back to the one model (and to the re-solve mode set before)
    h->msets.clear(); h->mset_of.clear(); h->mset_batch = 0; h->mset_waves = 0;
    return WF_OK;
  }
  if (h->B <= 0) return fail(h, WF_E_INVALID, "wf_set_batch must be called first (the parameter sets are assigned per farm)");
  if (n_sets < 1 || n_sets > h->B || !sets) return fail(h, WF_E_INVALID, "parameter sets: 1..env_batch of them");
  if (!set_of && n_sets != h->B) return fail(h, WF_E_INVALID, "parameter sets: without set_of, n_sets must equal env_batch (farm b takes set b)");
  std::string why;
  if (!modelset_validate(sets, n_sets, &why)) return fail(h, WF_E_INVALID, why);
  if (set_of)
    for (int b = 0; b < h->B; ++b)
      if (set_of[b] < 0 || set_of[b] >= n_sets) return fail(h, WF_E_INVALID, "parameter sets: a farm's set_of entry is outside 0..n_sets-1");
  h->msets.assign(sets, sets + n_sets);
  h->mset_of.resize((size_t)h->B);
  for (int b = 0; b < h->B; ++b) h->mset_of[(size_t)b] = set_of ? set_of[b] : b;
  h->mset_batch = h->B;
  h->msets_dirty = true;  // (uploaded before the next step)
  return WF_OK;
}

int wf_get_model_sets(wf_handle* h, int* n_sets, wf_model_set* sets, int* set_of) {
  if (!h || !n_sets) return WF_E_INVALID;
  *n_sets = (int)h->msets.size();
  if (sets) for (size_t k = 0; k < h->msets.size(); ++k) sets[k] = h->msets[k];
  if (set_of) for (size_t b = 0; b < h->mset_of.size(); ++b) set_of[b] = h->mset_of[b];
  return WF_OK;
}

int wf_model_sets_last_kernel(wf_handle* h, int* waves_per_farm) {
  if (!h || !waves_per_farm) return WF_E_INVALID;
  *waves_per_farm = h->msets.empty() ? 0 : h->mset_waves;
  return WF_OK;
}

}  // extern "C"
