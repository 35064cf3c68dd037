// wf_series.h — what the two translation units of the series extension (include/wfseries.h) share, and what the row extensions
// (lookahead/, plan/, credit/) call for their series-ahead mode: the arguments of wf_series_window_kernel and its launcher
// (wf_series_kernels.hip), and the host-side enqueue of a window on a parent handle (wf_series_abi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/wfseries.h"

// (the host side's types, ext/wf_ext.h: the kernels' translation unit does not need them)
struct wf_handle;
namespace wfi {
struct ext_base;
template <class T>
struct dev_buf;
}  // namespace wfi

struct WfSeriesWindowArgs {
  const int* farms;       // [n] device copy of the caller's list, or null = farm i
  int n, H, T;
  int tick0;              // min(t + first, T - 1): the tick of entry 0
  const int* start;       // [B] start row of every farm
  const double *s_ws, *s_wd;  // [T] the series
  double* wind;           // [n][H][2] speed, direction
};

extern "C" hipError_t wfk_launch_series_window(const WfSeriesWindowArgs* a, hipStream_t s);
extern "C" hipError_t wfk_series_func_attributes(int kernel, hipFuncAttributes* a);

namespace wfi {

// clamp(T - t - first, 0, H) of a handle in series mode
int series_available(const wf_handle* h, int first, int H);
// One launch on the handle's stream: the window (first, H) of n farms — d_farms a device list or null — into d_wind
// [n][H][2].  The caller has checked series mode and the limits.
hipError_t series_window_enqueue(wf_handle* h, int first, int H, int n, const int* d_farms, double* d_wind);

// The series-ahead mode of a row extension (lookahead/, plan/, credit/), in two steps of its run_rows policy.
// In `check`: the parent is in series mode, the caller passes no wind of its own, and the coming step exists.
int series_ahead_check(ext_base* x, bool caller_wind, int H);
// In `reserve` (the farm list is on the device): the window (first = 1, H) of the run's n farms into `buf`, grown as needed —
// [n][H][2], laid out like a caller's wind, so chunks index it the same way.
int series_ahead_window(ext_base* x, dev_buf<double>& buf, int H, int n, const int* d_farms);

}  // namespace wfi
