// wf_series.h — what the two translation units of the series extension (include/wfseries.h) share, and what the row extensions
// (lookahead/, plan/, credit/, rollout/, retgrad/) call for their series-ahead mode: the arguments of wf_series_window_kernel
// and its launcher (wf_series_kernels.hip), and the host-side enqueue of a window (wf_series_abi.hip).  A window is read from a
// series_view: the handle's shared series (wf_wind_series), or the per-farm series of a wind generator (include/wfwindgen.h,
// windgen/) — the same kernel, the same cursor arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfseries.h"

// (the host side's types, ext/wf_ext.h: the kernels' translation unit does not need them)
struct wf_handle;
struct wf_windgen;
namespace wfi {
struct ext_base;
template <class T>
struct dev_buf;
}  // namespace wfi

struct WfSeriesWindowArgs {
  const int* farms;       // [n] device copy of the caller's list, or null = farm i
  int n, H, T;
  int tick0;              // min(t + first, T - 1): the tick of entry 0
  const int* start;       // [B] start row of every farm, or null: every farm starts at row 0 and no row wraps
  const double *s_ws, *s_wd;  // the series: row r of farm b is element r * row_stride + b * farm_stride
  size_t row_stride, farm_stride;  // a shared series [T]: (1, 0); a series per farm, tick-major [T][B]: (B, 1)
  double* wind;           // [n][H][2] speed, direction
};

extern "C" hipError_t wfk_launch_series_window(const WfSeriesWindowArgs* a, hipStream_t s);
extern "C" hipError_t wfk_series_func_attributes(int kernel, hipFuncAttributes* a);

namespace wfi {

// a series and its cursor, as a window reads them
struct series_view {
  int T = 0, t = 0;
  const int* start = nullptr;
  const double *ws = nullptr, *wd = nullptr;
  size_t row_stride = 1, farm_stride = 0;
};
// the shared series of a handle in series mode
series_view handle_series(const wf_handle* h);
// The series of a generator that is playing on its parent (windgen/wf_windgen_abi.hip).  False, with the reason in *why, when
// it holds no series or the parent's wind was meanwhile set another way.
bool windgen_series(const wf_windgen* g, const wf_handle* parent, series_view* v, const char** why);

// clamp(T - t - first, 0, H)
int series_available(int T, int t, int first, int H);
// One launch on `s`: the window (first, H) of n farms — d_farms a device list or null — into d_wind [n][H][2].  The caller
// has checked the limits.
hipError_t series_window_enqueue(const series_view& v, hipStream_t s, int first, int H, int n, const int* d_farms, double* d_wind);

// The series-ahead mode of a row extension, in two steps of its run_rows policy.  `source` is the generator the object was
// given (wf_*_set_wind_source), or null: the parent handle's own series.
// In `check`: the source plays (or the parent is in series mode), the caller passes no wind of its own, and the coming step exists.
int series_ahead_check(ext_base* x, const wf_windgen* source, bool caller_wind, int H);
// In `reserve` (the farm list is on the device): the window (first = 1, H) of the run's n farms into `buf`, grown as needed —
// [n][H][2], laid out like a caller's wind, so chunks index it the same way.
int series_ahead_window(ext_base* x, const wf_windgen* source, dev_buf<double>& buf, int H, int n, const int* d_farms);

}  // namespace wfi
