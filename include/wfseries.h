/* wfseries.h — time-series episodes beyond reset / step: a preview of the wind series' coming rows on the device, the series
 * cursor as a checkpoint, and the series-ahead mode of the three row extensions (include/wflookahead.h, include/wfplan.h,
 * include/wfcredit.h) — the series extension of libwfstep.so (include/wfstep.h).
 *
 * A handle in series mode (wf_wind_series) plays T rows (speed, direction), every farm from a start row of its own; the
 * series, the start rows and the tick counter live on the device and in the handle.  This header reads a WINDOW of the coming
 * rows without a host round trip, hands the cursor out and puts it back, and lets lookahead, plan and credit solve their rows
 * under the wind the env is going to see instead of the wind it holds.  These are THE PROJECT'S OWN definitions.
 * PARITY UNPINNED beyond the oracle — except the window itself, which tests/test_series.py pins to the free wind the host
 * env over the oracle observes over its next steps; tests/series_ref.py restates it in NumPy.
 *
 * DEFINITIONS.  The handle is in series mode with T rows; t is the number of ticks (wf_wind_series_step) made since
 * wf_wind_series, so t = 0 right after it; farm b starts at start[b].
 *   The wind of farm b at tick u is series row (start[b] + u) % T, for 0 <= u <= T - 1.  Tick T does not exist:
 *   wf_wind_series_step fails there ("wind series exhausted").
 *   WINDOW (first, H): entry h is the wind at tick min(t + first + h, T - 1), h = 0 .. H - 1.
 *   available = clamp(T - t - first, 0, H) entries are real; the rest hold the last tick's wind.
 *   first = 0 starts at the wind the handle holds; first = 1 starts at the wind of the coming env step, because the env ticks
 *   before it steps.
 * SERIES-AHEAD RUNS (wf_*_set_series below).  Row h of a run on a series parent is solved under window entry h with
 *   first = 1 (the credit extension: H = 1).  wr_0, the speed the reward of h = 0 is normalised by, is the farm's CURRENT
 *   speed: the tick of the coming step leaves exactly that for the step.  A pending speed of an earlier tick (or of
 *   wf_env_set_prev_wind) is NOT used for wr_0: right after a reset it still holds the speed of the tick before the warm-up
 *   solve, which computes no reward and so does not consume it.  available == 0 is WF_E_INVALID "wind series exhausted" — the
 *   coming step itself would fail —; 0 < available < H runs, with the last wind held.
 *
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFSERIES_H
#define WFSERIES_H

#include "wfcredit.h"
#include "wflookahead.h"
#include "wfplan.h"
#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_SERIES_KERNELS 1

/* The window (first, H) of the listed farms.
 *   first       >= 0
 *   H           1 .. WF_LOOKAHEAD_MAX_H
 *   farms       [n_farms] farm indices (always a HOST array, validated), or NULL = all env_batch farms (n_farms ignored)
 *   wind        [n_farms][H][2] double (speed, direction), block i belongs to farms[i]
 *   available   one int (always a HOST int; may be NULL): clamp(T - t - first, 0, H)
 * on_device != 0: wind is a device pointer and the call only enqueues one launch of wf_series_window_kernel on the handle's
 * stream — except that it drains the stream when a `farms` list is given (its device copy is the call's own).  Otherwise wind
 * is a host array and the call synchronises.
 * WF_E_INVALID: the handle is not in series mode, wind == NULL, H or first outside their limits, a farm index out of range. */
int wf_series_window(wf_handle* h, int first, int H, int n_farms, const int* farms, double* wind, int* available, int on_device);

/* The cursor: T rows, t ticks made, start [env_batch] (a HOST array, or NULL) and whether the speed of tick t - 1 waits for the
 * next env step's reward (prev_pending).  Any pointer may be NULL.  Synchronises when start is given.
 * WF_E_INVALID: the handle is not in series mode. */
int wf_series_get(wf_handle* h, int* T, int* t, int* start, int* prev_pending);

/* Puts the handle in the state t ticks after wf_wind_series would have left: the wind of tick t is gathered, the geometry is
 * rebuilt (on the grouped path the groups turn to tick t), the speeds of tick t - 1 wait for the next env step's reward iff
 * prev_pending.  Ticking continues from there and exhausts at the same tick as before.  The series and the start rows stay.
 * WF_E_INVALID: the handle is not in series mode, t outside 0 .. T - 1, prev_pending with t == 0. */
int wf_series_seek(wf_handle* h, int t, int prev_pending);

/* Series-ahead mode of the three row extensions.  ahead != 0: a run with wind == NULL (wf_credit_run takes no wind) enqueues
 * the window (first = 1; H = the run's horizon, 1 for credit) of its farms into a buffer the object owns, solves row h under
 * entry h, and normalises h = 0 by the farm's current speed; no host round trip is added.  Default 0: the run holds the
 * parent's current wind, as before.  With ahead != 0 a run fails with WF_E_INVALID on a parent that is not in series mode, when
 * the caller passes a wind of its own as well, and when the series is exhausted (available == 0). */
int wf_lookahead_set_series(wf_lookahead* l, int ahead);
int wf_plan_set_series(wf_plan* p, int ahead);
int wf_credit_set_series(wf_credit* c, int ahead);

/* Register / LDS footprint of the kernel as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_SERIES_KERNELS][3] ints: row wf_series_window_kernel. */
int wf_series_kernel_info(wf_handle* h, int* info);

#ifdef __cplusplus
}
#endif
#endif /* WFSERIES_H */
