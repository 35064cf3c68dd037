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
    """The robust search.  Returns what yawopt_ref.optimize returns (power / power_initial / history are E)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ws, wd = np.atleast_1d(np.asarray(ws, np.float64)), np.atleast_1d(np.asarray(wd, np.float64))
    B, N = ws.size, x.size
    lo, hi = float(bounds[0]), float(bounds[1])
    best = np.zeros((B, N), np.float32) if yaw0 is None else np.array(yaw0, dtype=np.float32).reshape(B, N)
    order = np.stack([yawopt_ref.visit_order(x, y, wd[b]) for b in range(B)])
    margin = np.full(B, np.inf)
    history = []
    rows = np.arange(B)
    p_init = None
    for pi, (K, h, _) in enumerate(yawopt_ref.pass_steps(lo, hi, passes)):
        for s in range(N):
            t = order[:, s]
            inc = best[rows, t]
            cand = (np.broadcast_to(yawopt_ref.pass0_candidates(lo, hi, K), (B, K)) if pi == 0
                    else yawopt_ref.refine_candidates(inc, h, K, lo, hi))
            vals = np.concatenate([inc[:, None], cand], axis=1)  # index 0: the incumbent
            yaw = np.repeat(best[:, None, :], K + 1, axis=1)
            yaw[rows, :, t] = vals
            pw = expected_power(x, y, np.repeat(ws, K + 1), np.repeat(wd, K + 1), yaw.reshape(B * (K + 1), N), delta, w, frame, p,
                                step)[0].reshape(B, K + 1)
            if p_init is None:
                p_init = pw[:, 0].copy()
                history.append(p_init)
            win = np.argmax(pw, axis=1)  # first maximum: the incumbent, then the lowest index, keep a tie
            pb = pw[rows, win]
            rival = np.where(vals != vals[rows, win][:, None], pw, -np.inf).max(axis=1)
            margin = np.minimum(margin, np.where(np.isfinite(rival), (pb - rival) / pb, np.inf))
            best[rows, t] = vals[rows, win]
            history.append(pb)
    return {"yaw": best, "power": history[-1], "power_initial": p_init, "margin": margin, "history": np.array(history),
            "order": order}
