// wf_series_abi.hip — the C boundary of the series extension (include/wfseries.h): the window of a series' coming rows, the
// series cursor read and put back, and the enqueue the row extensions' series-ahead mode shares (series/wf_series.h).  It
// works on the handle itself — the series, the start rows and the tick live there (wf_handle.h, wf_wind_abi.hip) — and owns
// no object; what a call needs on the device besides the caller's arrays (a farm list, a host caller's window) is the call's
// own and is released before it returns.  The setters of the series-ahead mode are defined with their objects, in
// lookahead/, plan/ and credit/.
#include "../ext/wf_ext.h"
#include "wf_series.h"

using namespace wfi;

namespace wfi {

series_view handle_series(const wf_handle* h) {
  series_view v;
  v.T = h->series_T; v.t = h->series_t;
  v.start = h->d_series_start; v.ws = h->d_series_ws; v.wd = h->d_series_wd;
  v.row_stride = 1; v.farm_stride = 0;
  return v;
}

int series_available(int T, int t, int first, int H) {
  const long long left = (long long)T - t - first;
  return left <= 0 ? 0 : (left < H ? (int)left : H);
}

hipError_t series_window_enqueue(const series_view& v, hipStream_t s, int first, int H, int n, const int* d_farms, double* d_wind) {
  const long long t0 = (long long)v.t + first;
  WfSeriesWindowArgs a{};
  a.farms = d_farms; a.n = n; a.H = H; a.T = v.T;
  a.tick0 = (int)(t0 < (long long)v.T - 1 ? t0 : (long long)v.T - 1);
  a.start = v.start; a.s_ws = v.ws; a.s_wd = v.wd;
  a.row_stride = v.row_stride; a.farm_stride = v.farm_stride;
  a.wind = d_wind;
  return wfk_launch_series_window(&a, s);
}

// the series a series-ahead run reads: the source's, or the parent's own
static int series_ahead_view(ext_base* x, const wf_windgen* source, series_view* v) {
  const wf_handle* h = x->h;
  if (source) {
    const char* why = "";
    if (!windgen_series(source, h, v, &why)) return ext_fail(x, WF_E_INVALID, std::string("series-ahead mode: ") + why);
    return WF_OK;
  }
  if (h->series_T <= 0) return ext_fail(x, WF_E_INVALID, "series-ahead mode needs a parent in series mode: wf_wind_series comes first");
  *v = handle_series(h);
  return WF_OK;
}

int series_ahead_check(ext_base* x, const wf_windgen* source, bool caller_wind, int H) {
  series_view v;
  const int rc = series_ahead_view(x, source, &v);
  if (rc != WF_OK) return rc;
  if (caller_wind) return ext_fail(x, WF_E_INVALID, "series-ahead mode reads the series' coming rows: pass no wind of your own, or switch the mode off");
  if (series_available(v.T, v.t, 1, H) == 0) return ext_fail(x, WF_E_INVALID, "wind series exhausted: the coming step has no row left");
  return WF_OK;
}

int series_ahead_window(ext_base* x, const wf_windgen* source, dev_buf<double>& buf, int H, int n, const int* d_farms) {
  series_view v;
  int rc = series_ahead_view(x, source, &v);
  if (rc != WF_OK) return rc;
  rc = reserve(x, buf, 2 * (size_t)n * H);
  if (rc != WF_OK) return rc;
  WFX_HIP(x, series_window_enqueue(v, x->h->stream, 1, H, n, d_farms, buf));
  return WF_OK;
}

}  // namespace wfi

namespace {

const char* const kNoSeries = "the handle is not in series mode: wf_wind_series comes first";

// device memory of one call
struct call_buf {
  void* p = nullptr;
  ~call_buf() { hipFree(p); }
};

}  // namespace

extern "C" {

int wf_series_window(wf_handle* h, int first, int H, int n_farms, const int* farms, double* wind, int* available, int on_device) {
  if (!h) return WF_E_INVALID;
  if (h->series_T <= 0 || h->B <= 0) return fail(h, WF_E_INVALID, kNoSeries);
  if (!wind) return fail(h, WF_E_INVALID, "wf_series_window: wind is NULL");
  if (H < 1 || H > WF_LOOKAHEAD_MAX_H) return fail(h, WF_E_INVALID, "the window length H must be in 1..64");
  if (first < 0) return fail(h, WF_E_INVALID, "the window's first tick must be >= 0");
  if (!farms) n_farms = h->B;
  else {
    if (n_farms < 1) return fail(h, WF_E_INVALID, "n_farms must be >= 1");
    for (int k = 0; k < n_farms; ++k)
      if (farms[k] < 0 || farms[k] >= h->B) return fail(h, WF_E_INVALID, "farm index out of range (0 .. env_batch - 1)");
  }
  WF_ON_DEVICE(h);
  call_buf d_farms, d_wind;
  const size_t bytes = sizeof(double) * 2 * (size_t)n_farms * H;
  if (farms) {
    WF_HIP(h, hipMalloc(&d_farms.p, sizeof(int) * (size_t)n_farms));
    WF_HIP(h, hipMemcpyAsync(d_farms.p, farms, sizeof(int) * (size_t)n_farms, hipMemcpyHostToDevice, h->stream));
  }
  if (!on_device) WF_HIP(h, hipMalloc(&d_wind.p, bytes));
  WF_HIP(h, series_window_enqueue(handle_series(h), h->stream, first, H, n_farms, (const int*)d_farms.p, on_device ? wind : (double*)d_wind.p));
  if (!on_device) WF_HIP(h, hipMemcpyAsync(wind, d_wind.p, bytes, hipMemcpyDeviceToHost, h->stream));
  if (!on_device || farms) WF_HIP(h, hipStreamSynchronize(h->stream));  // (before the call's own buffers go)
  if (available) *available = series_available(h->series_T, h->series_t, first, H);
  return WF_OK;
}

int wf_series_get(wf_handle* h, int* T, int* t, int* start, int* prev_pending) {
  if (!h) return WF_E_INVALID;
  if (h->series_T <= 0) return fail(h, WF_E_INVALID, kNoSeries);
  if (T) *T = h->series_T;
  if (t) *t = h->series_t;
  if (prev_pending) *prev_pending = (h->ws_prev_valid && h->d_ws_prev) ? 1 : 0;
  if (start) {
    WF_ON_DEVICE(h);
    WF_HIP(h, hipMemcpyAsync(start, h->d_series_start, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
    WF_HIP(h, hipStreamSynchronize(h->stream));
  }
  return WF_OK;
}

int wf_series_seek(wf_handle* h, int t, int prev_pending) {
  if (!h) return WF_E_INVALID;
  if (h->series_T <= 0 || h->B <= 0) return fail(h, WF_E_INVALID, kNoSeries);
  if (t < 0 || t >= h->series_T) return fail(h, WF_E_INVALID, "wf_series_seek: the tick must be in 0 .. T - 1");
  if (prev_pending && t == 0) return fail(h, WF_E_INVALID, "wf_series_seek: no tick precedes tick 0, so no speed can be pending there");
  WF_ON_DEVICE(h);
  if (prev_pending) {  // the speeds of tick t - 1, as the tick to t would have kept them
    if (!h->d_ws_prev) WF_HIP(h, hipMalloc(&h->d_ws_prev, sizeof(double) * h->B));
    WF_HIP(h, wfk_launch_series_gather(h->B, h->series_T, t - 1, h->d_series_start, h->d_series_ws, h->d_series_wd, h->d_ws, h->d_wd,
                                       h->stream));
    WF_HIP(h, hipMemcpyAsync(h->d_ws_prev, h->d_ws, sizeof(double) * h->B, hipMemcpyDeviceToDevice, h->stream));
  }
  h->ws_prev_valid = prev_pending != 0;
  h->series_t = t;
  WF_HIP(h, wfk_launch_series_gather(h->B, h->series_T, t, h->d_series_start, h->d_series_ws, h->d_series_wd, h->d_ws, h->d_wd,
                                     h->stream));
  h->wind_count = h->B;
  h->shared_dir = false;
  if (h->n_groups > 0) {
    h->group_shift = t;  // (as wf_wind_series_step: geometry and tables are per row)
  } else {
    int rc = run_geometry(h, h->B, h->d_wd, false);
    if (rc != WF_OK) return rc;
    h->pair_dirty = true;
  }
  return WF_OK;
}

int wf_series_kernel_info(wf_handle* h, int* info) {
  if (!h || !info) return fail(h, WF_E_INVALID, "wf_series_kernel_info: NULL argument");
  WF_ON_DEVICE(h);
  hipFuncAttributes a{};
  WF_HIP(h, wfk_series_func_attributes(0, &a));
  info[0] = a.numRegs; info[1] = (int)a.sharedSizeBytes; info[2] = (int)a.localSizeBytes;
  return WF_OK;
}

}  // extern "C"
