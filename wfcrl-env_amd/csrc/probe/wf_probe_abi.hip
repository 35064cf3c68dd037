// wf_probe_abi.hip — the C boundary of the probe extension (include/wfprobe.h): a probe object that belongs to a handle,
// owns its device buffers and launches the two kernels of wf_probe_kernels.hip on the handle's stream.  Reads the handle
// (layout, wind, model constants, float64 tables, the fused env's yaw state); stores nothing in it.  Base, buffers and the
// checks of the handle and the farm list are the extensions' shared layer (ext/wf_ext.h); a probe has no evaluator.
#include "../../../include/wfprobe.h"
#include "../ext/wf_ext.h"
#include "wf_probe.h"

using namespace wfi;

// (the event pool holds three events, made at creation: before the state kernel, between the two kernels, after the sampler)
struct wf_probe : ext_base {
  int P = 0, n_sets = 0;
  dev_buf<double> d_xyz, d_rec, d_hdr;
  farm_list farms;
  dev_buf<float> d_yaw, d_uvw;  // staging for host callers
};

namespace {

void fill_consts(const wf_handle* h, WfProbeConsts* c) {
  const wf_model_params& m = h->model;
  c->r = h->rconsts;
  c->shear = m.shear; c->kappa = m.kappa; c->lm_c = m.rotor_diameter / 8.0;
  c->dudz_c = m.shear * std::pow(1.0 / m.hub_height, m.shear);
  c->inv_HH = 1.0 / m.hub_height;
  c->xc = h->xc; c->yc = h->yc;
}

}  // namespace

extern "C" {

int wf_probe_create(wf_handle* h, wf_probe** out) {
  int rc = ext_create(h, out);
  if (rc != WF_OK) return rc;
  wf_probe* p = *out;
  DeviceGuard guard(h->device);
  hipError_t e = guard.err;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    hipEvent_t ev = nullptr;
    if ((e = hipEventCreate(&ev)) == hipSuccess) p->ev_pool.push_back(ev);
  }
  if (e != hipSuccess) {
    delete p;
    *out = nullptr;
    return fail(h, WF_E_HIP, std::string("wf_probe_create: ") + hipGetErrorString(e));
  }
  return WF_OK;
}

int wf_probe_destroy(wf_probe* p) { return ext_destroy(p); }

int wf_probe_set_points(wf_probe* p, int n_points, const double* xyz, int n_sets, int on_device) {
  if (!p || !xyz) return ext_fail(p, WF_E_INVALID, "wf_probe_set_points: NULL argument");
  wf_handle* h = p->h;
  if (n_points < 1 || n_points > 65535 * 256) return ext_fail(p, WF_E_INVALID, "n_points must be in 1..16776960");
  if (n_sets != 1 && (h->B <= 0 || n_sets != h->B)) return ext_fail(p, WF_E_INVALID, "n_sets must be 1 or env_batch (a set of points per farm)");
  const size_t n = (size_t)n_sets * n_points * 3;
  if (!on_device)
    for (size_t k = 0; k < n; ++k)
      if (!std::isfinite(xyz[k]) || (k % 3 == 2 && !(xyz[k] > 0.0)))
        return ext_fail(p, WF_E_INVALID, "probe points must be finite with z > 0 (height above ground)");
  WFX_ON_DEVICE(p);
  p->P = 0;
  {
    int rc = reserve(p, p->d_xyz, n);
    if (rc != WF_OK) return rc;
  }
  WFX_HIP(p, hipMemcpyAsync(p->d_xyz, xyz, sizeof(double) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  if (!on_device) WFX_HIP(p, hipStreamSynchronize(h->stream));  // the caller's host array may go away
  p->P = n_points; p->n_sets = n_sets;
  return WF_OK;
}

int wf_probe_sample(wf_probe* p, const float* yaw, int n_farms, const int* farms, float* uvw, int on_device) {
  if (!p || !uvw) return ext_fail(p, WF_E_INVALID, "wf_probe_sample: NULL argument");
  wf_handle* h = p->h;
  int rc = check_parent(p, "flow sampling serves", "wf_probe_sample");
  if (rc != WF_OK) return rc;
  if (p->P <= 0) return ext_fail(p, WF_E_INVALID, "no points have been set: wf_probe_set_points must be called before wf_probe_sample");
  if (p->n_sets != 1 && p->n_sets != h->B) return ext_fail(p, WF_E_INVALID, "the per-farm point sets were given for another env_batch: set the points again");
  if (!yaw && !h->d_env_yaw) return ext_fail(p, WF_E_INVALID, "yaw == NULL samples at the fused env's yaw state, but the handle has none (wf_env_reset)");
  if ((rc = check_farms(p, &n_farms, farms)) != WF_OK) return rc;
  WFX_ON_DEVICE(p);
  if (h->model_dirty && (rc = build_consts(h)) != WF_OK) return ext_fail(p, rc, h->err);
  const int N = h->N, P = p->P;
  const size_t bn = (size_t)h->B * N, out_n = (size_t)n_farms * P * 3;
  rc = reserve(p, p->d_rec, (size_t)n_farms * N * WF_PROBE_REC);
  if (rc == WF_OK) rc = reserve(p, p->d_hdr, (size_t)n_farms * WF_PROBE_HDR);
  if (rc == WF_OK && farms) rc = reserve(p, p->farms.d, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw) rc = reserve(p, p->d_yaw, bn);
  if (rc == WF_OK && !on_device) rc = reserve(p, p->d_uvw, out_n);
  if (rc != WF_OK) return rc;
  if (farms && (rc = upload_farms(p, p->farms, farms, n_farms)) != WF_OK) return rc;
  const float* d_yaw = yaw ? yaw : h->d_env_yaw;
  if (yaw && !on_device) {
    WFX_HIP(p, hipMemcpyAsync(p->d_yaw, yaw, sizeof(float) * bn, hipMemcpyHostToDevice, h->stream));
    d_yaw = p->d_yaw;
  }
  WfProbeConsts c;
  fill_consts(h, &c);
  WfProbeStateArgs sa{};
  sa.tab64 = h->d_tab64; sa.lx = h->d_lx; sa.ly = h->d_ly;
  sa.ws = h->d_ws; sa.wd = h->d_wd; sa.wind_stride = h->wind_count == h->B ? 1 : 0;
  sa.yaw = d_yaw; sa.farms = farms ? p->farms.d.p : nullptr; sa.rec = p->d_rec; sa.hdr = p->d_hdr;
  WfProbeSampleArgs pa{};
  pa.rec = p->d_rec; pa.hdr = p->d_hdr; pa.farms = sa.farms; pa.xyz = p->d_xyz; pa.per_farm = p->n_sets != 1 ? 1 : 0; pa.P = P;
  pa.uvw = on_device ? uvw : p->d_uvw;
  WFX_HIP(p, hipEventRecord(p->ev_pool[0], h->stream));
  WFX_HIP(p, wfk_launch_probe_state(&c, &sa, n_farms, h->stream));
  WFX_HIP(p, hipEventRecord(p->ev_pool[1], h->stream));
  WFX_HIP(p, wfk_launch_probe_sample(&c, &pa, n_farms, h->stream));
  WFX_HIP(p, hipEventRecord(p->ev_pool[2], h->stream));
  p->timed = true;
  if (!on_device) {
    WFX_HIP(p, hipMemcpyAsync(uvw, p->d_uvw, sizeof(float) * out_n, hipMemcpyDeviceToHost, h->stream));
    WFX_HIP(p, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_probe_last_timing(wf_probe* p, float* state_ms, float* sample_ms) {
  if (!p) return WF_E_INVALID;
  if (!p->timed) return ext_fail(p, WF_E_INVALID, "wf_probe_sample has not run yet");
  WFX_ON_DEVICE(p);
  WFX_HIP(p, hipEventSynchronize(p->ev_pool[2]));
  if (state_ms) WFX_HIP(p, hipEventElapsedTime(state_ms, p->ev_pool[0], p->ev_pool[1]));
  if (sample_ms) WFX_HIP(p, hipEventElapsedTime(sample_ms, p->ev_pool[1], p->ev_pool[2]));
  return WF_OK;
}

int wf_probe_kernel_info(wf_probe* p, int* info) {
  if (!p || !info) return WF_E_INVALID;
  return kernel_info(p, 2, wfk_probe_func_attributes, info);
}

const char* wf_probe_last_error(wf_probe* p) { return p ? p->err.c_str() : "wf_probe: NULL probe"; }

}  // extern "C"
