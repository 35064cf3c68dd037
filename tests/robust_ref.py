"""TEST INFRASTRUCTURE — the reference for expected power under wind-direction uncertainty and the robust yaw search
(include/wfrobust.h): a plain NumPy restatement over the float64 oracle, which it does not modify.  Grids, visit order and
farm power are those of tests/yawopt_ref.py.

The definition, as the header states it:
  members   M offsets delta[m] (degrees, strictly ascending), weights weight[m] >= 0 with a positive sum;
            w[m] = weight[m] / (weight[0] + weight[1] + ...), the sum in index order
  frame     "relative": every member is stepped with the yaw as given; "fixed": member m is stepped with
            float32(float64(yaw) + delta[m]) — the nacelle stays where the nominal direction put it
  expected power  E = sum_m w[m] P_m, P_m the farm power (yawopt_ref.farm_power) at (ws, wd + delta[m]) and the member's
            yaw; the member sum runs in index order, every product and sum rounded on its own
  search    yawopt_ref.optimize with farm power replaced by E: visit order from the NOMINAL direction, bounds on the nominal yaw

`optimize` records the decision margin per farm exactly as yawopt_ref.optimize does (the relative distance between the best
and the second-best distinct candidate, here in E)."""
from statistics import NormalDist

import numpy as np

import yawopt_ref

MEMBERS5 = (np.array([-6.0, -3.0, 0.0, 3.0, 6.0]), np.exp(-np.array([-6.0, -3.0, 0.0, 3.0, 6.0]) ** 2 / 18.0))  # std 3 deg


def members(delta=None, weight=None, std=None, resolution=1.0, cutoff=0.995):
    """(delta, w): the offsets and the NORMALISED weights — from (delta, weight) as they are, or the Gaussian table of
    (std, resolution, cutoff): bound = ceil(inv_cdf(cutoff) std / resolution), 2 bound + 1 members, weights exp(-d^2 / 2 std^2)."""
    if std is not None:
        bound = int(np.ceil(NormalDist().inv_cdf(cutoff) * std / resolution))
        delta = resolution * np.arange(-bound, bound + 1, dtype=np.float64)
        weight = np.exp(-(delta * delta) / (2.0 * std * std))
    delta, weight = np.asarray(delta, np.float64).reshape(-1), np.asarray(weight, np.float64).reshape(-1)
    assert delta.size == weight.size >= 1 and (np.diff(delta) > 0).all() and (weight >= 0).all()
    s = 0.0
    for v in weight:
        s = s + float(v)
    assert s > 0.0
    return delta, weight / s


def member_yaw(yaw, d, frame):
    """The float32 yaw member `d` is stepped with."""
    yaw = np.asarray(yaw, np.float32)
    if frame == "fixed":
        return (yaw.astype(np.float64) + d).astype(np.float32)
    assert frame == "relative"
    return yaw


def expected_power(x, y, ws, wd, yaw, delta, w, frame="fixed", p=None, step=None):
    """ws, wd (B,), yaw (B, N) float32 values, (delta, w) from `members`.  Returns (E (B,), member powers (B, M), per-turbine
    expectation (B, N)), float64."""
    yaw = np.atleast_2d(np.asarray(yaw, np.float32))
    B, N = yaw.shape
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    fn = step or yawopt_ref._c_step
    pm = np.zeros((B, len(delta)))
    E, Et = np.zeros(B), np.zeros((B, N))
    for m, d in enumerate(delta):
        pw = fn(x, y, ws, wd + d, member_yaw(yaw, d, frame).astype(np.float64), p or yawopt_ref.ModelParams())
        s = np.zeros(B)
        for t in range(N):
            s = s + pw[:, t]
        pm[:, m] = s
        E = E + w[m] * s
        Et = Et + w[m] * pw
    return E, pm, Et


def optimize(x, y, ws, wd, delta, w, frame="fixed", yaw0=None, bounds=(-25.0, 25.0), passes=(5, 4), p=None, step=None):
    """The robust search: yawopt_ref.optimize over E.  Returns what it returns (power / power_initial / history are E)."""
    def objective(x, y, ws, wd, yaw, p, step):
        return expected_power(x, y, ws, wd, yaw, delta, w, frame, p, step)[0]

    return yawopt_ref.optimize(x, y, ws, wd, yaw0, bounds, passes, p, step, objective)
