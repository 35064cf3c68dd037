"""TEST INFRASTRUCTURE — the reference for the rose extension (include/wfrose.h): the yaw-table look-up, the expected-power
reduction over a wind rose and the look-up-table policy restated in plain NumPy, over the float64 oracle, which it does not
modify.

  lookup    the header's definition, step by step, in float64 (np.fmod is C's fmod, every product and sum is one IEEE
            operation — the arithmetic of the device function, so that float32 results can be compared bit for bit)
  evaluate  rows in (case, direction, speed) order through oracle.c_oracle.farm_step_batch; a row's float64 turbine powers
            added in caller order; a condition with ws < cut_in or ws > cut_out counts as zero; the weighted sums run over
            (d, s) in index order
  policy    the target clipped to the env's bounds in float32, then the env's action encoding
"""
import numpy as np

from oracle.floris_gch_numpy import ModelParams

# ---- the row of three the CPU and GPU tests of table building share -------------------------------------------------------
D = 126.0
ROW3 = (np.array([0.0, 5 * D, 10 * D]), np.zeros(3))  # three turbines in a row, 5 D apart
ROW3_WD = np.arange(260.0, 281.0, 5.0)                # along the row and up to 10 deg off it
ROW3_WS = np.array([6.0, 8.0, 10.0])


def bracket(twd, tws, ws, wd):
    """(k, k1, fd, j, j1, fs) of one wind: steps 1-3 of the header."""
    twd, tws = np.asarray(twd, np.float64), np.asarray(tws, np.float64)
    Dt, St = twd.size, tws.size
    w = np.fmod(np.float64(wd), 360.0)
    if w < 0.0:
        w = w + 360.0
    if Dt == 1:
        k, k1, fd = 0, 0, np.float64(0.0)
    else:
        k = int(np.sum(twd <= w)) - 1
        if k < 0:
            w, k = w + 360.0, Dt - 1
        if k == Dt - 1:
            x0, x1, k1 = twd[Dt - 1], twd[0] + 360.0, 0
        else:
            x0, x1, k1 = twd[k], twd[k + 1], k + 1
        fd = (w - x0) / (x1 - x0)
    v = min(max(np.float64(ws), tws[0]), tws[St - 1])
    j = max(int(np.sum(tws <= v)) - 1, 0)
    j1 = min(j + 1, St - 1)
    fs = (v - tws[j]) / (tws[j1] - tws[j]) if j1 > j else np.float64(0.0)
    return k, k1, fd, j, j1, fs


def lookup(table, twd, tws, ws, wd, interp="linear"):
    """table (Dt, St, N); ws, wd scalars or (B,) arrays.  Returns (N,) or (B, N) float32."""
    T = np.asarray(table, np.float32)
    if np.ndim(ws) > 0 or np.ndim(wd) > 0:
        ws, wd = np.broadcast_arrays(np.asarray(ws, np.float64), np.asarray(wd, np.float64))
        return np.stack([lookup(T, twd, tws, a, b, interp) for a, b in zip(ws, wd)])
    k, k1, fd, j, j1, fs = bracket(twd, tws, ws, wd)
    if interp == "nearest":
        return T[k1 if fd > 0.5 else k, j1 if fs > 0.5 else j].copy()
    assert interp == "linear", interp
    t = T.astype(np.float64)
    lo = (1.0 - fs) * t[k, j] + fs * t[k, j1]
    hi = (1.0 - fs) * t[k1, j] + fs * t[k1, j1]
    return ((1.0 - fd) * lo + fd * hi).astype(np.float32)


def case_yaw(case, wd, ws, N, tables):
    """(D, S, N) float32 yaw of one case over the rose.  case: "zero", an (N,) array, or ("table", slot) with
    tables[slot] = (table, twd, tws, interp)."""
    D, S = len(wd), len(ws)
    if isinstance(case, str):
        assert case == "zero"
        return np.zeros((D, S, N), np.float32)
    if isinstance(case, tuple) and case[0] == "table":
        T, twd, tws, interp = tables[case[1]]
        return np.stack([np.stack([lookup(T, twd, tws, ws[s], wd[d], interp) for s in range(S)]) for d in range(D)])
    return np.broadcast_to(np.asarray(case, np.float32), (D, S, N)).copy()


def evaluate(x, y, wd, ws, freq, cases=("zero",), cut_in=0.001, cut_out=None, tables=None, p=None):
    """dict(turbine_power (C, D, S, N) float64 — the oracle's, unmasked —, condition_power (C, D, S) float64 masked,
    weighted_power (C,), weighted_turbine_power (C, N), mask (S,) bool, freq_sum)."""
    from oracle import c_oracle

    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    wd, ws = np.atleast_1d(np.asarray(wd, np.float64)), np.atleast_1d(np.asarray(ws, np.float64))
    freq = np.asarray(freq, np.float64)
    D, S, N, C = wd.size, ws.size, x.size, len(cases)
    assert freq.shape == (D, S)
    yaw = np.stack([case_yaw(c, wd, ws, N, tables) for c in cases]).astype(np.float64)  # (C, D, S, N)
    rws = np.broadcast_to(ws[None, None, :], (C, D, S)).reshape(-1)
    rwd = np.broadcast_to(wd[None, :, None], (C, D, S)).reshape(-1)
    pw = c_oracle.farm_step_batch(x, y, rws, rwd, yaw.reshape(-1, N), p or ModelParams())["power"].reshape(C, D, S, N)
    mask = (ws < cut_in) | ((ws > cut_out) if cut_out is not None and cut_out > 0 else np.zeros(S, bool))
    farm = np.zeros((C, D, S))
    for t in range(N):  # caller order
        farm = farm + pw[..., t]
    farm[:, :, mask] = 0.0
    wp, wtp = np.zeros(C), np.zeros((C, N))
    for d in range(D):  # (d, s) index order
        for s in range(S):
            if not mask[s]:
                wp = wp + freq[d, s] * farm[:, d, s]
                wtp = wtp + freq[d, s] * pw[:, d, s, :]
    return {"turbine_power": pw, "condition_power": farm, "weighted_power": wp, "weighted_turbine_power": wtp, "mask": mask,
            "freq_sum": float(np.sum(freq)), "yaw": yaw.astype(np.float32)}


def policy(table, twd, tws, interp, ws, wd, yaw_now, lo, hi, step, discrete):
    """(target (B, N) float32, action (B, N) float32) of the look-up-table controller."""
    lo, hi, step = np.float32(lo), np.float32(hi), np.float32(step)
    target = np.minimum(np.maximum(lookup(table, twd, tws, ws, wd, interp), lo), hi).astype(np.float32)
    dy = target - np.asarray(yaw_now, np.float32)
    if discrete:
        half = np.float32(0.5) * step
        action = np.where(dy >= half, 2.0, np.where(dy <= -half, 0.0, 1.0)).astype(np.float32)
    else:
        action = np.minimum(np.maximum(dy, -step), step).astype(np.float32)
    return target, action
