/* wfprobe.h — flow sampling at arbitrary points: the probe extension of libwfstep.so (include/wfstep.h).
 *
 * FLORIS 3.5 offers `sample_flow_at_points` and `calculate_horizontal_plane` on the object the reference's
 * FlorisInterface wraps (reference wfcrl/interface.py:479, `self.fi`).  A probe is the counterpart here: for any farm of a
 * handle's batch it returns the flow (u, v, w) at caller-chosen points — a virtual met mast, a hub-height wake map, a check
 * of a yaw policy against the flow it produces.
 *
 * What a probe value IS (this project's own definition, the turbine solve extended to points): the value a rotor-grid point
 * of ONE ADDITIONAL turbine placed at (x, y, z) would have after the sequential Gauss-Curl-Hybrid solve, that extra turbine
 * giving no wake and inducing nothing on itself.  In the terms of oracle/floris_gch_numpy.py::farm_step:
 *   Uinit = ws (z / HH)^shear;  every real turbine's deflection [A.3-3] and deficit [A.3-6] evaluated at the point and
 *   combined as wake = hypot(wake, deficit Uinit);  every real turbine's transverse terms [A.3-4] added (ground mirrors, the
 *   dx < 0 mask, the per-source w < 0 clamp);  u = Uinit - wake.
 * The source's Ct, induction, commanded / effective yaw and wake-rotation circulation come from the float64 turbine solve;
 * where that solve reads the source's turbulence intensity "at the target's grid index" the probe reads the source's CENTRE
 * grid column (before the yaw-added mixing for the deflection, after it for the deficit).  No turbulence intensity is
 * returned for a point: the overlap count is defined for a rotor.
 * PARITY UNPINNED: this is NOT FLORIS' own full-flow solver, which may treat the source turbulence differently; like
 * everything beyond the one known-answer vector it rests on the project's restatement (tests/probe_ref.py holds the
 * kernels to it through "ghost" turbines).
 *
 * Everything is float64 on the device (csrc/probe/); outputs are float32.  Coordinates are those of wf_set_layout; z is the
 * height above ground, z > 0.  A probe belongs to a handle, owns its device buffers (per-source state records, points,
 * staging), stores nothing in the handle and must be destroyed BEFORE it.  All work runs on the handle's stream.
 * wfstep.h and WF_ABI_VERSION are not touched by this extension.
 */
#ifndef WFPROBE_H
#define WFPROBE_H

#include "wfstep.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wf_probe wf_probe;

int wf_probe_create(wf_handle* h, wf_probe** out);
int wf_probe_destroy(wf_probe* p);

/* The points to sample: xyz [n_sets][n_points][3] double, caller's frame.
 *   n_sets == 1          one set of n_points for every farm
 *   n_sets == env_batch  a set per farm (indexed by the farm's index in the batch)
 * Host arrays (on_device == 0) are validated (finite, z > 0) and the call returns after the copy (it synchronises); device
 * arrays are copied as they are, asynchronously (a point with z <= 0 samples NaN).  The probe keeps its own copy. */
int wf_probe_set_points(wf_probe* p, int n_points, const double* xyz, int n_sets, int on_device);

/* Solve the listed farms at `yaw` in float64 and sample their flow at the points.
 *   yaw   [env_batch * n_turbines] float, absolute degrees, caller's turbine order — or NULL: the fused env's current yaw
 *         state (wf_env_reset / wf_env_step), which is read, never written
 *   farms [n_farms] farm indices (always a HOST array), or NULL = all env_batch farms (n_farms is then ignored)
 *   uvw   [n_farms][n_points][3] float: u along the wind, v lateral, w vertical, m/s
 * on_device != 0: yaw and uvw are device pointers and the call enqueues its work on the handle's stream without waiting
 * for it — except that it drains the stream first when one of the probe's buffers has to grow (more farms or points than
 * any call before) and when a `farms` list is given (the list is uploaded from a host copy the previous call may still
 * be read from).  A caller that samples every step with farms == NULL and unchanged sizes never waits.
 * Reads the wind (what wf_get_wind reports) and the layout the handle holds at the time of the call.
 * WF_E_INVALID: no wind or no points set.  WF_E_UNSUPPORTED (version 1): a handle with several layouts (wf_set_layouts*) or
 * with turbine definitions (wf_set_turbine_types). */
int wf_probe_sample(wf_probe* p, const float* yaw, int n_farms, const int* farms, float* uvw, int on_device);

/* HIP-event time of the two kernels of the last wf_probe_sample (synchronises): the float64 farm solve that leaves the
 * per-source state records, and the sampler.  Either pointer may be NULL. */
int wf_probe_last_timing(wf_probe* p, float* state_ms, float* sample_ms);

/* Register / LDS footprint of the two kernels as the runtime reports it (hipFuncGetAttributes; recorded next to the timings
 * by tools/probe_timing.py): vgprs, static LDS bytes, private-segment bytes.
 * info [2][3] ints: row 0 wf_probe_state_kernel, row 1 wf_probe_sample_kernel (whose LDS is dynamic on top:
 * 160 bytes per turbine). */
int wf_probe_kernel_info(wf_probe* p, int* info);

const char* wf_probe_last_error(wf_probe* p);

#ifdef __cplusplus
}
#endif
#endif /* WFPROBE_H */
