// wf_windgen_abi.hip — the C boundary of the wind generator extension (include/wfwindgen.h): an object that belongs to a parent
// handle, owns the series of every farm of the parent's batch on the device (tick-major, one grow-only buffer) and the cursor,
// and plays the series through the parent's PUBLIC ABI — wf_set_wind and wf_env_set_prev_wind with device pointers, as any
// caller with device arrays would.  It stores nothing in the handle and reads of it only the batch, the stream and whether
// its wind was meanwhile set another way.  The window and the read-back are the series extension's kernel over a series_view
// of this object's arrays (series/wf_series.h), which is also what the row extensions' series-ahead mode reads.
#include <cmath>
#include <cstdint>

#include "../ext/wf_ext.h"
#include "../series/wf_series.h"
#include "wf_windgen.h"

using namespace wfi;

struct wf_windgen : ext_base {
  // the series: ws = d_series, wd = d_series + T B
  dev_buf<double> d_series;
  int T = 0, t = 0, B = 0;  // T == 0: no series; B: the batch it was generated for
  int kernel = -1;          // wf_windgen_set_kernel: -1 the library's choice, 0 wf_windgen_kernel, 1 wf_windgen_tiled_kernel
  unsigned long long seed = 0;
  wf_wind_dist dist{};
  wf_wind_process process{};
  const double* ws() const { return d_series.p; }
  const double* wd() const { return d_series.p + (size_t)T * B; }
};

namespace {

const wf_wind_dist kDefaultDist{8.0, 8.0, 3.0, 28.0, 270.0, 20.0, 0.0, 360.0};  // wf_wind_sample's
const char* const kNoSeries = "the generator holds no series: wf_windgen_generate comes first";
const char* const kElsewhere = "the parent's wind was set another way since the series was generated: generate (or seek) again";

// device memory of one call
struct call_buf {
  void* p = nullptr;
  ~call_buf() { hipFree(p); }
};

// the parent still holds a wind per farm and is not in wf_wind_series mode (the cheap check of include/wfwindgen.h)
bool parent_plays(const wf_windgen* g) {
  const wf_handle* h = g->h;
  return g->T > 0 && h->B == g->B && h->series_T <= 0 && h->wind_count == h->B;
}

series_view view_of(const wf_windgen* g) {
  series_view v;
  v.T = g->T; v.t = g->t;
  v.start = nullptr; v.ws = g->ws(); v.wd = g->wd();
  v.row_stride = (size_t)g->B; v.farm_stride = 1;
  return v;
}

#define WFG_PARENT(g, call)                                                                  \
  do {                                                                                       \
    int rc_ = (call);                                                                        \
    if (rc_ != WF_OK) return ext_fail(g, rc_, std::string("parent: ") + wf_last_error((g)->h)); \
  } while (0)

// the parent's wind becomes row t; the speeds of row t - 1 wait for the next reward iff pending (the order matters:
// wf_set_wind clears the pending speed)
int put_row(wf_windgen* g, int t, bool pending) {
  const size_t B = (size_t)g->B;
  WFG_PARENT(g, wf_set_wind(g->h, g->ws() + (size_t)t * B, g->wd() + (size_t)t * B, g->B, 1));
  if (pending) WFG_PARENT(g, wf_env_set_prev_wind(g->h, g->ws() + (size_t)(t - 1) * B, 1));
  return WF_OK;
}

int check_list(wf_windgen* g, int* n_farms, const int* farms) {
  if (!farms) { *n_farms = g->B; return WF_OK; }
  if (*n_farms < 1) return ext_fail(g, WF_E_INVALID, "n_farms must be >= 1");
  for (int k = 0; k < *n_farms; ++k)
    if (farms[k] < 0 || farms[k] >= g->B) return ext_fail(g, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  return WF_OK;
}

// The window (first, H) at cursor `t` of the listed farms into `wind` — a host array, or with on_device a device array.
int window_at(wf_windgen* g, int t, int first, int H, int n_farms, const int* farms, double* wind, int on_device) {
  wf_handle* h = g->h;
  call_buf d_farms, d_wind;
  const size_t bytes = sizeof(double) * 2 * (size_t)n_farms * H;
  if (farms) {
    WFX_HIP(g, hipMalloc(&d_farms.p, sizeof(int) * (size_t)n_farms));
    WFX_HIP(g, hipMemcpyAsync(d_farms.p, farms, sizeof(int) * (size_t)n_farms, hipMemcpyHostToDevice, h->stream));
  }
  if (!on_device) WFX_HIP(g, hipMalloc(&d_wind.p, bytes));
  series_view v = view_of(g);
  v.t = t;
  WFX_HIP(g, series_window_enqueue(v, h->stream, first, H, n_farms, (const int*)d_farms.p, on_device ? wind : (double*)d_wind.p));
  if (!on_device) WFX_HIP(g, hipMemcpyAsync(wind, d_wind.p, bytes, hipMemcpyDeviceToHost, h->stream));
  if (!on_device || farms) WFX_HIP(g, hipStreamSynchronize(h->stream));  // (before the call's own buffers go)
  return WF_OK;
}

}  // namespace

namespace wfi {

bool windgen_series(const wf_windgen* g, const wf_handle* parent, series_view* v, const char** why) {
  if (g->h != parent) { *why = "the wind source belongs to another handle"; return false; }
  if (g->T <= 0) { *why = kNoSeries; return false; }
  if (!parent_plays(g)) { *why = kElsewhere; return false; }
  *v = view_of(g);
  return true;
}

}  // namespace wfi

extern "C" {

int wf_windgen_create(wf_handle* h, wf_windgen** out) { return ext_create(h, out); }

int wf_windgen_destroy(wf_windgen* g) { return ext_destroy(g); }

int wf_windgen_generate(wf_windgen* g, int T, unsigned long long seed, const wf_wind_dist* dist, const wf_wind_process* process,
                        const double* ws0, const double* wd0) {
  if (!g) return WF_E_INVALID;
  wf_handle* h = g->h;
  if (!process) return ext_fail(g, WF_E_INVALID, "wf_windgen_generate: process is NULL");
  if (h->B <= 0) return ext_fail(g, WF_E_INVALID, "wf_set_batch must be called before wf_windgen_generate");
  if (T < 1) return ext_fail(g, WF_E_INVALID, "the wind series needs at least one tick");
  const wf_wind_dist d = dist ? *dist : kDefaultDist;
  if (!(d.ws_scale > 0) || !(d.ws_shape > 0) || !(d.ws_lo > 0) || !(d.ws_lo <= d.ws_hi) || !(d.wd_std >= 0))
    return ext_fail(g, WF_E_INVALID, "invalid wind distribution parameters");
  const wf_wind_process& p = *process;
  if (!in_unit(p.ws_revert) || !in_unit(p.wd_revert)) return ext_fail(g, WF_E_INVALID, "ws_revert and wd_revert must be in [0, 1]");
  if (!non_negative(p.ws_sigma) || !non_negative(p.wd_sigma) || !non_negative(p.wd_ramp))
    return ext_fail(g, WF_E_INVALID, "ws_sigma, wd_sigma and wd_ramp must be finite and >= 0");
  if ((ws0 == nullptr) != (wd0 == nullptr)) return ext_fail(g, WF_E_INVALID, "ws0 and wd0 come together: tick 0 is given whole or drawn whole");
  const int B = h->B;
  std::vector<double> row0;
  if (ws0) {
    row0.resize(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
      if (!(ws0[b] > 0.0) || !std::isfinite(ws0[b]) || !std::isfinite(wd0[b]))
        return ext_fail(g, WF_E_INVALID, "wind speed must be > 0 and direction finite");
      double w = std::fmod(wd0[b], 360.0);
      if (w < 0.0) w += 360.0;
      row0[b] = ws0[b];
      row0[(size_t)B + b] = w;
    }
  }
  WFX_ON_DEVICE(g);
  // T B 16 bytes, in one buffer
  const size_t rows = (size_t)T, per = (size_t)B;
  if (rows > SIZE_MAX / 16 / per) return ext_fail(g, WF_E_NOMEM, "the wind series does not fit: T * env_batch * 16 bytes");
  const size_t n = 2 * rows * per;
  g->T = 0;  // (no series while the buffer may change)
  if (n > g->d_series.cap) {
    WFX_HIP(g, hipStreamSynchronize(h->stream));
    hipFree(g->d_series.p);
    g->d_series.p = nullptr; g->d_series.cap = 0;
    const hipError_t e = hipMalloc(&g->d_series.p, sizeof(double) * n);
    if (e != hipSuccess) {
      g->d_series.p = nullptr;
      (void)hipGetLastError();
      if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
        return ext_fail(g, WF_E_NOMEM, "the wind series does not fit on the device: T * env_batch * 16 bytes");
      return ext_fail(g, WF_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    g->d_series.cap = n;
  }
  double* const ws = g->d_series.p;
  double* const wd = ws + rows * per;
  if (ws0) {
    WFX_HIP(g, hipMemcpyAsync(ws, row0.data(), sizeof(double) * per, hipMemcpyHostToDevice, h->stream));
    WFX_HIP(g, hipMemcpyAsync(wd, row0.data() + per, sizeof(double) * per, hipMemcpyHostToDevice, h->stream));
  } else {  // the reset draw's own kernel, straight into row 0
    const double dv[8] = {d.ws_scale, d.ws_shape, d.ws_lo, d.ws_hi, d.wd_mean, d.wd_std, d.wd_lo, d.wd_hi};
    WFX_HIP(g, wfk_launch_wind_sample(B, seed, dv, ws, wd, h->stream));
  }
  WfWindgenArgs a{};
  a.B = B; a.T = T; a.seed = seed;
  a.ws_revert = p.ws_revert; a.ws_sigma = p.ws_sigma; a.wd_revert = p.wd_revert; a.wd_sigma = p.wd_sigma; a.wd_ramp = p.wd_ramp;
  a.ws_lo = d.ws_lo; a.ws_hi = d.ws_hi;
  a.ws = ws; a.wd = wd;
  // Which kernel: the tiled one parallelises the draws and shortens the serial chain per tick, at three barriers a tile; it is
  // ahead on both recorded workloads, 4096 and 65 536 farms (profiles/windgen_timing.json)
  const int tiled = g->kernel >= 0 ? g->kernel : 1;
  WFX_HIP(g, wfk_launch_windgen(&a, tiled, h->stream));
  if (ws0) WFX_HIP(g, hipStreamSynchronize(h->stream));  // (row0 goes with this call)
  g->T = T; g->t = 0; g->B = B;
  g->seed = seed; g->dist = d; g->process = p;
  const int rc = put_row(g, 0, false);
  if (rc != WF_OK) g->T = 0;
  return rc;
}

int wf_windgen_set_kernel(wf_windgen* g, int kernel) {
  if (!g) return WF_E_INVALID;
  if (kernel < -1 || kernel > 1) return ext_fail(g, WF_E_INVALID, "wf_windgen_set_kernel: -1 (the library's choice), 0 (a thread per farm) or 1 (tiled)");
  g->kernel = kernel;
  return WF_OK;
}

int wf_windgen_step(wf_windgen* g) {
  if (!g) return WF_E_INVALID;
  if (g->T <= 0) return ext_fail(g, WF_E_INVALID, kNoSeries);
  if (!parent_plays(g)) return ext_fail(g, WF_E_INVALID, kElsewhere);
  if (g->t + 1 >= g->T) return ext_fail(g, WF_E_INVALID, "wind series exhausted");
  WFX_ON_DEVICE(g);
  const int rc = put_row(g, g->t + 1, true);
  if (rc != WF_OK) return rc;
  g->t += 1;
  return WF_OK;
}

int wf_windgen_get(wf_windgen* g, int* T, int* t, int* prev_pending, unsigned long long* seed, wf_wind_dist* dist,
                   wf_wind_process* process) {
  if (!g) return WF_E_INVALID;
  if (g->T <= 0) return ext_fail(g, WF_E_INVALID, kNoSeries);
  const wf_handle* h = g->h;
  if (T) *T = g->T;
  if (t) *t = g->t;
  if (prev_pending) *prev_pending = (h->ws_prev_valid && h->d_ws_prev) ? 1 : 0;
  if (seed) *seed = g->seed;
  if (dist) *dist = g->dist;
  if (process) *process = g->process;
  return WF_OK;
}

int wf_windgen_seek(wf_windgen* g, int t, int prev_pending) {
  if (!g) return WF_E_INVALID;
  if (g->T <= 0) return ext_fail(g, WF_E_INVALID, kNoSeries);
  if (g->h->B != g->B) return ext_fail(g, WF_E_INVALID, kElsewhere);
  if (t < 0 || t >= g->T) return ext_fail(g, WF_E_INVALID, "wf_windgen_seek: the tick must be in 0 .. T - 1");
  if (prev_pending && t == 0) return ext_fail(g, WF_E_INVALID, "wf_windgen_seek: no tick precedes tick 0, so no speed can be pending there");
  WFX_ON_DEVICE(g);
  const int rc = put_row(g, t, prev_pending != 0);
  if (rc != WF_OK) return rc;
  g->t = t;
  return WF_OK;
}

int wf_windgen_window(wf_windgen* g, int first, int H, int n_farms, const int* farms, double* wind, int* available, int on_device) {
  if (!g) return WF_E_INVALID;
  if (g->T <= 0) return ext_fail(g, WF_E_INVALID, kNoSeries);
  if (!parent_plays(g)) return ext_fail(g, WF_E_INVALID, kElsewhere);
  if (!wind) return ext_fail(g, WF_E_INVALID, "wf_windgen_window: wind is NULL");
  if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return ext_fail(g, WF_E_INVALID, "the window length H must be in 1..64");
  if (first < 0) return ext_fail(g, WF_E_INVALID, "the window's first tick must be >= 0");
  int rc = check_list(g, &n_farms, farms);
  if (rc != WF_OK) return rc;
  WFX_ON_DEVICE(g);
  if ((rc = window_at(g, g->t, first, H, n_farms, farms, wind, on_device)) != WF_OK) return rc;
  if (available) *available = series_available(g->T, g->t, first, H);
  return WF_OK;
}

int wf_windgen_read(wf_windgen* g, int tick0, int n, int n_farms, const int* farms, double* wind) {
  if (!g) return WF_E_INVALID;
  if (g->T <= 0) return ext_fail(g, WF_E_INVALID, kNoSeries);
  if (g->h->B != g->B) return ext_fail(g, WF_E_INVALID, kElsewhere);
  if (!wind) return ext_fail(g, WF_E_INVALID, "wf_windgen_read: wind is NULL");
  if (tick0 < 0 || n < 1 || tick0 >= g->T || n > g->T - tick0)
    return ext_fail(g, WF_E_INVALID, "wf_windgen_read: the ticks must lie in 0 .. T - 1, at least one");
  const int rc = check_list(g, &n_farms, farms);
  if (rc != WF_OK) return rc;
  WFX_ON_DEVICE(g);
  return window_at(g, tick0, 0, n, n_farms, farms, wind, 0);  // (no tick past T - 1: nothing is held)
}

int wf_windgen_kernel_info(wf_windgen* g, int* info) {
  if (!g) return WF_E_INVALID;
  if (!info) return ext_fail(g, WF_E_INVALID, "wf_windgen_kernel_info: NULL argument");
  return kernel_info(g, WF_WINDGEN_KERNELS, wfk_windgen_func_attributes, info);
}

const char* wf_windgen_last_error(wf_windgen* g) { return g ? g->err.c_str() : ""; }

}  // extern "C"
