/* wfwindgen.h — synthetic wind episodes: a stochastic wind series PER FARM, generated and played on the device — the wind
 * generator extension of libwfstep.so (include/wfstep.h).
 *
 * A handle in series mode (wf_wind_series) plays ONE series of T rows that every farm enters at a start row of its own: a
 * batch sees at most T distinct winds, all slices of one realisation, and the series comes from a file.  A generator object
 * holds a series of T ticks for EVERY farm of its parent's batch — a mean-reverting speed and direction with an optional
 * direction ramp, drawn from the counter-based Philox of the wind process (csrc/wf_philox.h) — and plays it through the
 * parent's public ABI, exactly as a caller with device arrays would: a tick is wf_set_wind(row t + 1, on_device = 1) followed
 * by wf_env_set_prev_wind(speeds of row t, on_device = 1).  The object stores nothing in the handle, and the handle is NOT
 * in wf_wind_series mode while a generated episode plays.  Window, cursor, seek and the series-ahead mode of the row
 * extensions mean what include/wfseries.h says, with "series row (start[b] + u) % T" replaced by "the farm's own row u".
 * These are THE PROJECT'S OWN definitions.  PARITY UNPINNED beyond the NumPy restatement (tests/windgen_ref.py).
 *
 * DEFINITION.  All arithmetic is float64 and every product and sum below is ONE rounding (the library is built with
 * -ffp-contract=off), so the NumPy restatement reproduces the bits.
 *   Inputs: T >= 1 ticks; a 64-bit seed; a wf_wind_dist for tick 0 (NULL: the default of wf_wind_sample); a process
 *   (ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp) — the reverts in [0, 1], the sigmas (m/s, degrees per tick) and the
 *   ramp (degrees per tick) finite and >= 0 —; optionally host arrays ws0, wd0 of env_batch entries.
 *   TICK 0 of farm b.  Without ws0 / wd0, (S0, D0) is what wf_wind_sample(seed, dist) stores for farm b: the same kernel
 *   writes row 0 of the series, so the bits are wf_wind_sample's by construction.  With ws0 / wd0: S0 = ws0[b] (> 0),
 *   D0 = fmod(wd0[b], 360), + 360 if negative (wd0[b] finite).
 *   THE RAMP of farm b: rate = wd_ramp * (2 * u01(r[0], r[1]) - 1), r = philox(seed, counter b, stream 3), u01 the 53-bit
 *   uniform of csrc/wf_philox.h: a rate in (-wd_ramp, wd_ramp) degrees per tick, fixed for the episode.
 *   DEVIATES: z(b, u, stream) = (the sum of the four words of philox(seed, counter (b << 32) | u, stream) * 2^-32 - 2) * sqrt 3 —
 *   mean 0, variance 1, |z| <= 2 sqrt 3; the planner's deviate (csrc/ext/wf_deviate.h), exact up to the last product.
 *   TICKS u = 1 .. T - 1, with the latent x_0 = S0, y_0 = D0:
 *     x_u = (x_{u-1} + ws_revert * (S0 - x_{u-1})) + ws_sigma * z(b, u, 4)
 *     m_u = D0 + rate * (double)u
 *     y_u = (y_{u-1} + wd_revert * (m_u - y_{u-1})) + wd_sigma * z(b, u, 5)
 *     speed_u     = min(max(x_u, dist.ws_lo), dist.ws_hi)
 *     direction_u = fmod(y_u, 360), + 360 if negative
 *   The latent is neither clipped nor wrapped: a clipped speed leaves the bound as the process would have.  dist.wd_lo and
 *   dist.wd_hi act AT TICK 0 ONLY (they belong to the reset draw): later directions wander over the whole circle.
 *   A farm's series depends on (seed, b, dist, process) — and ws0[b], wd0[b] when given — alone: not on env_batch, not on the
 *   launch shape.
 *   The stationary variance of x is ws_sigma^2 / (1 - (1 - ws_revert)^2) for ws_revert > 0.
 * CURSOR.  t is the number of ticks (wf_windgen_step) made since wf_windgen_generate, so t = 0 right after it: generate puts
 *   tick 0 into the parent and leaves no pending speed.  Tick T does not exist: wf_windgen_step fails there ("wind series
 *   exhausted").  WINDOW (first, H), available, seek and prev_pending: include/wfseries.h.
 * The series is stored tick-major, ws[T][B] and wd[T][B]: row u is a contiguous [B] array that a tick hands to wf_set_wind as
 * it is.  T * env_batch * 16 bytes that the device cannot hold is WF_E_NOMEM.
 *
 * The parent's wind may be set another way while a generator holds a series (wf_set_wind, wf_wind_sample, wf_wind_series):
 * that ends the generated episode.  wf_windgen_step, _seek, _window and the series-ahead runs then refuse where they can tell —
 * the parent is in wf_wind_series mode or holds one wind for the batch —; a caller that set a wind per farm of its own has to
 * call wf_windgen_generate (or wf_windgen_seek) again before it goes on ticking.
 *
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFWINDGEN_H
#define WFWINDGEN_H

#include "wfcredit.h"
#include "wflookahead.h"
#include "wfplan.h"
#include "wfretgrad.h"
#include "wfrollout.h"
#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_WINDGEN_KERNELS 2

typedef struct wf_windgen wf_windgen;

typedef struct wf_wind_process {
  double ws_revert; /* [0, 1]: the share of the speed's distance to S0 that a tick takes back */
  double ws_sigma;  /* >= 0, m/s: the speed's innovation per tick */
  double wd_revert; /* [0, 1]: the same for the direction, towards D0 + rate * u */
  double wd_sigma;  /* >= 0, degrees: the direction's innovation per tick */
  double wd_ramp;   /* >= 0, degrees per tick: every farm draws its ramp rate from (-wd_ramp, wd_ramp) */
} wf_wind_process;

/* An object of handle h (wf_set_layout and wf_set_batch may come later); it goes before its handle. */
int wf_windgen_create(wf_handle* h, wf_windgen** out);
int wf_windgen_destroy(wf_windgen* g);

/* Generates the series of every farm of the parent's batch (one generating launch on the handle's stream, no host traffic without
 * ws0 / wd0), sets the parent's wind to tick 0 and leaves no pending speed; t = 0.  ws0 / wd0: HOST arrays [env_batch], both
 * or neither.  WF_E_INVALID with a message: a NULL g or process, no batch, T < 1, an invalid distribution, a process parameter
 * outside its range or not finite, ws0 without wd0 (or the reverse), a ws0 that is not > 0, a wd0 that is not finite.
 * WF_E_NOMEM: the series does not fit. */
int wf_windgen_generate(wf_windgen* g, int T, unsigned long long seed, const wf_wind_dist* dist, const wf_wind_process* process,
                        const double* ws0, const double* wd0);

/* Which kernel the next wf_windgen_generate launches: -1 the library's choice (the default), 0 wf_windgen_kernel — a thread per
 * farm walks its ticks —, 1 wf_windgen_tiled_kernel — a block draws a tile of (farm, tick) deviates in parallel and a lane per
 * farm walks it.  The two store the same bits; the switch exists for measurements and tests.  WF_E_INVALID: another value. */
int wf_windgen_set_kernel(wf_windgen* g, int kernel);

/* One tick: the parent's wind becomes row t + 1 (wf_set_wind, which clears the pending speed), THEN the speeds of row t wait
 * for the next env step's reward (wf_env_set_prev_wind); t += 1.  Nothing is copied through the host.
 * WF_E_INVALID: no series, t + 1 >= T ("wind series exhausted"), the parent's wind was set another way. */
int wf_windgen_step(wf_windgen* g);

/* The cursor — T, t, prev_pending (the parent holds a pending speed) — and what a checkpoint needs to generate the same
 * series again: seed, dist (the default's values when generate took NULL) and process.  Any pointer may be NULL.
 * ws0 / wd0 are the caller's to keep.  WF_E_INVALID: no series. */
int wf_windgen_get(wf_windgen* g, int* T, int* t, int* prev_pending, unsigned long long* seed, wf_wind_dist* dist,
                   wf_wind_process* process);

/* Puts parent and cursor in the state t ticks after wf_windgen_generate would have left: the wind of row t, the speeds of
 * row t - 1 pending iff prev_pending.  Ticking continues from there and exhausts at the same tick as before.
 * WF_E_INVALID: no series, t outside 0 .. T - 1, prev_pending with t == 0. */
int wf_windgen_seek(wf_windgen* g, int t, int prev_pending);

/* The window (first, H) of the listed farms: the arguments and the behaviour of wf_series_window (include/wfseries.h).
 * WF_E_INVALID: no series, wind == NULL, H outside 1 .. WF_LOOKAHEAD_MAX_H, first < 0, n_farms < 1 with a list, a farm index
 * out of range, the parent's wind was set another way. */
int wf_windgen_window(wf_windgen* g, int first, int H, int n_farms, const int* farms, double* wind, int* available, int on_device);

/* Ticks [tick0, tick0 + n) of the listed farms (a HOST list, or NULL = all env_batch farms) into the HOST array wind
 * [n_farms][n][2] (speed, direction), whatever the cursor and the parent's wind are: for tests and plots.  Synchronises.
 * WF_E_INVALID: no series, wind == NULL, a tick outside 0 .. T - 1 or n < 1, a farm index out of range. */
int wf_windgen_read(wf_windgen* g, int tick0, int n, int n_farms, const int* farms, double* wind);

/* Series-ahead mode of the five row extensions on a generated episode.  With a source set and the object's wf_*_set_series
 * (ahead != 0), a run reads the window of the generator's coming rows instead of the handle's series; everything else about
 * the mode is include/wfseries.h's: step 0 normalised by the current speed, available == 0 refused, no host round trip.
 * g == NULL: the parent handle's own series again.  The generator has to belong to the object's parent and outlive the runs. */
int wf_credit_set_wind_source(wf_credit* c, wf_windgen* g);
int wf_lookahead_set_wind_source(wf_lookahead* l, wf_windgen* g);
int wf_plan_set_wind_source(wf_plan* p, wf_windgen* g);
int wf_rollout_set_wind_source(wf_rollout* r, wf_windgen* g);
int wf_retgrad_set_wind_source(wf_retgrad* r, wf_windgen* g);

/* Register / LDS footprint of the kernel as the runtime reports it (hipFuncGetAttributes): vgprs, static LDS bytes,
 * private-segment bytes.  info [WF_WINDGEN_KERNELS][3] ints: rows wf_windgen_kernel,
 * wf_windgen_tiled_kernel. */
int wf_windgen_kernel_info(wf_windgen* g, int* info);

const char* wf_windgen_last_error(wf_windgen* g);

#ifdef __cplusplus
}
#endif
#endif /* WFWINDGEN_H */
