// wf_probe_abi.hip — the C boundary of the probe extension (include/wfprobe.h): a probe object that belongs to a handle,
// owns its device buffers and launches the two kernels of wf_probe_kernels.hip on the handle's stream.  Reads the handle
// (layout, wind, model constants, float64 tables, the fused env's yaw state); stores nothing in it.
#include "../../../include/wfprobe.h"
#include "../wf_handle.h"
#include "wf_probe.h"

using namespace wfi;

struct wf_probe {
  wf_handle* h = nullptr;
  std::string err;
  int P = 0, n_sets = 0;
  double* d_xyz = nullptr;
  size_t xyz_cap = 0;
  double *d_rec = nullptr, *d_hdr = nullptr;
  size_t rec_cap = 0, hdr_cap = 0;
  int* d_farms = nullptr;
  size_t farms_cap = 0;
  std::vector<int> farms;  // host copy the upload reads from
  float *d_yaw = nullptr, *d_uvw = nullptr;  // staging for host callers
  size_t yaw_cap = 0, uvw_cap = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool timed = false;
};

namespace {

int pfail(wf_probe* p, int code, const std::string& msg) {
  if (p) p->err = msg;
  return code;
}
#define WFP_HIP(p, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return pfail(p, WF_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WFP_ON_DEVICE(p)                 \
  DeviceGuard guard_((p)->h->device);    \
  if (guard_.err != hipSuccess) return pfail(p, WF_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err))

// grow-only device buffer (the stream is drained before a buffer in use is released)
template <class T>
int reserve(wf_probe* p, T** buf, size_t* cap, size_t n) {
  if (n <= *cap) return WF_OK;
  WFP_HIP(p, hipStreamSynchronize(p->h->stream));
  hipFree(*buf);
  *buf = nullptr; *cap = 0;
  WFP_HIP(p, hipMalloc(buf, sizeof(T) * n));
  *cap = n;
  return WF_OK;
}

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
  if (!h || !out) return WF_E_INVALID;
  *out = nullptr;
  wf_probe* p = new (std::nothrow) wf_probe();
  if (!p) return fail(h, WF_E_NOMEM, "out of host memory");
  p->h = h;
  DeviceGuard guard(h->device);
  hipError_t e = guard.err;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&p->ev[k]);
  if (e != hipSuccess) {
    for (int k = 0; k < 3; ++k)
      if (p->ev[k]) hipEventDestroy(p->ev[k]);
    delete p;
    return fail(h, WF_E_HIP, std::string("wf_probe_create: ") + hipGetErrorString(e));
  }
  *out = p;
  return WF_OK;
}

int wf_probe_destroy(wf_probe* p) {
  if (!p) return WF_OK;
  DeviceGuard guard(p->h->device);
  hipStreamSynchronize(p->h->stream);
  hipFree(p->d_xyz); hipFree(p->d_rec); hipFree(p->d_hdr); hipFree(p->d_farms); hipFree(p->d_yaw); hipFree(p->d_uvw);
  for (int k = 0; k < 3; ++k) hipEventDestroy(p->ev[k]);
  delete p;
  return WF_OK;
}

int wf_probe_set_points(wf_probe* p, int n_points, const double* xyz, int n_sets, int on_device) {
  if (!p || !xyz) return pfail(p, WF_E_INVALID, "wf_probe_set_points: NULL argument");
  wf_handle* h = p->h;
  if (n_points < 1 || n_points > 65535 * 256) return pfail(p, WF_E_INVALID, "n_points must be in 1..16776960");
  if (n_sets != 1 && (h->B <= 0 || n_sets != h->B)) return pfail(p, WF_E_INVALID, "n_sets must be 1 or env_batch (a set of points per farm)");
  const size_t n = (size_t)n_sets * n_points * 3;
  if (!on_device)
    for (size_t k = 0; k < n; ++k)
      if (!std::isfinite(xyz[k]) || (k % 3 == 2 && !(xyz[k] > 0.0)))
        return pfail(p, WF_E_INVALID, "probe points must be finite with z > 0 (height above ground)");
  WFP_ON_DEVICE(p);
  p->P = 0;
  {
    int rc = reserve(p, &p->d_xyz, &p->xyz_cap, n);
    if (rc != WF_OK) return rc;
  }
  WFP_HIP(p, hipMemcpyAsync(p->d_xyz, xyz, sizeof(double) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  if (!on_device) WFP_HIP(p, hipStreamSynchronize(h->stream));  // the caller's host array may go away
  p->P = n_points; p->n_sets = n_sets;
  return WF_OK;
}

int wf_probe_sample(wf_probe* p, const float* yaw, int n_farms, const int* farms, float* uvw, int on_device) {
  if (!p || !uvw) return pfail(p, WF_E_INVALID, "wf_probe_sample: NULL argument");
  wf_handle* h = p->h;
  if (h->N <= 0 || h->B <= 0) return pfail(p, WF_E_INVALID, "no layout / batch: wf_set_layout and wf_set_batch come first");
  if (h->n_layouts > 1 || !h->layout_n.empty())
    return pfail(p, WF_E_UNSUPPORTED, "flow sampling serves a handle with ONE layout: this one holds several layouts (wf_set_layouts / wf_set_layouts_counts)");
  if (!h->types.empty())
    return pfail(p, WF_E_UNSUPPORTED, "flow sampling serves one turbine definition: this handle holds several turbine definitions (wf_set_turbine_types)");
  if (h->wind_count == 0) return pfail(p, WF_E_INVALID, "no wind has been set: wf_set_wind (or wf_wind_*) must be called before wf_probe_sample");
  if (p->P <= 0) return pfail(p, WF_E_INVALID, "no points have been set: wf_probe_set_points must be called before wf_probe_sample");
  if (p->n_sets != 1 && p->n_sets != h->B) return pfail(p, WF_E_INVALID, "the per-farm point sets were given for another env_batch: set the points again");
  if (!yaw && !h->d_env_yaw) return pfail(p, WF_E_INVALID, "yaw == NULL samples at the fused env's yaw state, but the handle has none (wf_env_reset)");
  if (farms) {
    if (n_farms < 1) return pfail(p, WF_E_INVALID, "n_farms must be >= 1");
    for (int k = 0; k < n_farms; ++k)
      if (farms[k] < 0 || farms[k] >= h->B) return pfail(p, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  } else {
    n_farms = h->B;
  }
  WFP_ON_DEVICE(p);
  if (h->model_dirty) {
    int rc = build_consts(h);
    if (rc != WF_OK) return pfail(p, rc, h->err);
  }
  const int N = h->N, P = p->P;
  const size_t bn = (size_t)h->B * N, out_n = (size_t)n_farms * P * 3;
  int rc = reserve(p, &p->d_rec, &p->rec_cap, (size_t)n_farms * N * WF_PROBE_REC);
  if (rc == WF_OK) rc = reserve(p, &p->d_hdr, &p->hdr_cap, (size_t)n_farms * WF_PROBE_HDR);
  if (rc == WF_OK && farms) rc = reserve(p, &p->d_farms, &p->farms_cap, (size_t)n_farms);
  if (rc == WF_OK && !on_device && yaw) rc = reserve(p, &p->d_yaw, &p->yaw_cap, bn);
  if (rc == WF_OK && !on_device) rc = reserve(p, &p->d_uvw, &p->uvw_cap, out_n);
  if (rc != WF_OK) return rc;
  if (farms) {
    WFP_HIP(p, hipStreamSynchronize(h->stream));  // (a previous upload may still read the host copy)
    p->farms.assign(farms, farms + n_farms);
    WFP_HIP(p, hipMemcpyAsync(p->d_farms, p->farms.data(), sizeof(int) * n_farms, hipMemcpyHostToDevice, h->stream));
  }
  const float* d_yaw = yaw ? yaw : h->d_env_yaw;
  if (yaw && !on_device) {
    WFP_HIP(p, hipMemcpyAsync(p->d_yaw, yaw, sizeof(float) * bn, hipMemcpyHostToDevice, h->stream));
    d_yaw = p->d_yaw;
  }
  WfProbeConsts c;
  fill_consts(h, &c);
  WfProbeStateArgs sa{};
  sa.tab64 = h->d_tab64; sa.lx = h->d_lx; sa.ly = h->d_ly;
  sa.ws = h->d_ws; sa.wd = h->d_wd; sa.wind_stride = h->wind_count == h->B ? 1 : 0;
  sa.yaw = d_yaw; sa.farms = farms ? p->d_farms : nullptr; sa.rec = p->d_rec; sa.hdr = p->d_hdr;
  WfProbeSampleArgs pa{};
  pa.rec = p->d_rec; pa.hdr = p->d_hdr; pa.farms = sa.farms; pa.xyz = p->d_xyz; pa.per_farm = p->n_sets != 1 ? 1 : 0; pa.P = P;
  pa.uvw = on_device ? uvw : p->d_uvw;
  WFP_HIP(p, hipEventRecord(p->ev[0], h->stream));
  WFP_HIP(p, wfk_launch_probe_state(&c, &sa, n_farms, h->stream));
  WFP_HIP(p, hipEventRecord(p->ev[1], h->stream));
  WFP_HIP(p, wfk_launch_probe_sample(&c, &pa, n_farms, h->stream));
  WFP_HIP(p, hipEventRecord(p->ev[2], h->stream));
  p->timed = true;
  if (!on_device) {
    WFP_HIP(p, hipMemcpyAsync(uvw, p->d_uvw, sizeof(float) * out_n, hipMemcpyDeviceToHost, h->stream));
    WFP_HIP(p, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_probe_last_timing(wf_probe* p, float* state_ms, float* sample_ms) {
  if (!p) return WF_E_INVALID;
  if (!p->timed) return pfail(p, WF_E_INVALID, "wf_probe_sample has not run yet");
  WFP_ON_DEVICE(p);
  WFP_HIP(p, hipEventSynchronize(p->ev[2]));
  if (state_ms) WFP_HIP(p, hipEventElapsedTime(state_ms, p->ev[0], p->ev[1]));
  if (sample_ms) WFP_HIP(p, hipEventElapsedTime(sample_ms, p->ev[1], p->ev[2]));
  return WF_OK;
}

int wf_probe_kernel_info(wf_probe* p, int* info) {
  if (!p || !info) return WF_E_INVALID;
  WFP_ON_DEVICE(p);
  for (int k = 0; k < 2; ++k) {
    hipFuncAttributes a;
    WFP_HIP(p, wfk_probe_func_attributes(k, &a));
    info[3 * k] = a.numRegs; info[3 * k + 1] = (int)a.sharedSizeBytes; info[3 * k + 2] = (int)a.localSizeBytes;
  }
  return WF_OK;
}

const char* wf_probe_last_error(wf_probe* p) { return p ? p->err.c_str() : "wf_probe: NULL probe"; }

}  // extern "C"
