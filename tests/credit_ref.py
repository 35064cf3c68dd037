"""TEST INFRASTRUCTURE — the reference for the per-agent counterfactual rewards (include/wfcredit.h): a plain NumPy
restatement over the float64 oracle (oracle.c_oracle.farm_step_batch), which it does not modify.

The definition, as the header states it, for one farm of N turbines with K alternatives per turbine:
  transition  an ACTION becomes a yaw as in the fused env step, in float32: frac = acc / rate / (moves + 1) / dt;
              frac >= budget zeroes the raw action ("down" in the discrete encoding: the reference's quirk);
              discrete: a = (a - 1) step, continuous: a clipped to +-step; y' = clip(y + a, lo, hi)
  rows        R = 1 + N K: row 0 the base yaw, row 1 + i K + k the base with entry i replaced by alternative (i, k)
  row reward  psum = the row's N powers added in caller order, lsum = its 4 N absolute load values added in memory order,
              r = psum / N / 1e6 * 1e3 / wr^3 - load_coef lsum / (4 N), float64, evaluated left to right; load_coef is the
              float32 the env holds
  difference  [N][K] = reward[0] - reward[1 + i K + k]; where the alternative's float32 yaw has the bits of the base entry it
              is exactly 0.0 and the row's reward / farm_power are copies of row 0's
P and the loads are the oracle's float64 values (the device's are the step's float32 outputs: `bound` says how far the two
may be apart)."""
import numpy as np

import parity


def transition(yaw, acc, moves, action, env_params):
    """float32 yaw' of `action` (B, N[, K]) on the state yaw (B, N), acc (B, N), moves (B,) — the counter BEFORE the step.
    env_params: dict(yaw_lo, yaw_hi, yaw_step, actuator_rate, dt, budget, discrete)."""
    f = np.float32
    e = env_params
    a = np.array(action, dtype=f)
    extra = (1,) * (a.ndim - 2)
    y = np.asarray(yaw, f).reshape(a.shape[:2] + extra)
    ac = np.asarray(acc, f).reshape(a.shape[:2] + extra)
    mv = (np.asarray(moves).reshape((-1, 1) + extra) + 1).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = ((ac / f(e["actuator_rate"])) / mv) / f(e["dt"])
    a = np.where(frac >= f(e["budget"]), f(0.0), a).astype(f)
    step = f(e["yaw_step"])
    a = ((a - f(1.0)) * step).astype(f) if e["discrete"] else np.minimum(np.maximum(a, -step), step)
    return np.minimum(np.maximum((y + a).astype(f), f(e["yaw_lo"])), f(e["yaw_hi"])).astype(f)


def rows(base, alt):
    """(B, 1 + N K, N) float32: the evaluator's yaw block of base (B, N) and alt (B, N, K) yaws."""
    base = np.asarray(base, np.float32)
    alt = np.asarray(alt, np.float32)
    B, N, K = alt.shape
    blk = np.repeat(base[:, None, :], 1 + N * K, axis=1)
    for i in range(N):
        for k in range(K):
            blk[:, 1 + i * K + k, i] = alt[:, i, k]
    return blk


def sums(out):
    """(psum, lsum) (rows,) float64 of out["power"] (rows, N) W and out["load"] (rows, N, 4): added in order."""
    pw = np.asarray(out["power"], np.float64)
    ld = np.abs(np.asarray(out["load"], np.float64)).reshape(pw.shape[0], -1)
    psum, lsum = np.zeros(pw.shape[0]), np.zeros(pw.shape[0])
    for t in range(pw.shape[1]):
        psum = psum + pw[:, t]
    for t in range(ld.shape[1]):
        lsum = lsum + ld[:, t]
    return psum, lsum


def reward(out, wr, load_coef):
    """(rows,) float64 row rewards; wr (rows,) the normalising speed."""
    N = np.asarray(out["power"]).shape[1]
    psum, lsum = sums(out)
    wr = np.asarray(wr, np.float64)
    return psum / N / 1.0e6 * 1.0e3 / (wr * wr * wr) - np.float64(np.float32(load_coef)) * lsum / (4.0 * N)


def _std_scale(out):
    """What parity.errors() divides a std error by: max(1, 0.2 x the farm's largest rotor wind speed), per row."""
    ws = np.asarray(out["wind_speed"], np.float64)
    return np.maximum(1.0, 0.2 * ws.reshape(ws.shape[0], -1).max(axis=1))


def _tols(out, tol):
    """(tol_power, tol_ti, tol_std (rows,)) as parity.within() applies `tol` to a farm of this size.  TOL_F64["std"] is
    stated on the 1e-4 scale of TOL["std"] (parity.py: 5e-3 of it, 5e-7 m/s)."""
    N = np.asarray(out["power"]).shape[1]
    f = parity.LARGE_FARM_FACTOR if N > 128 else 1.0
    std = tol["std"] * (parity.TOL["std"] if tol is parity.TOL_F64 else 1.0)
    return tol["power"] * f, tol["ti"], std * f * _std_scale(out)


def power_bound(out, tol):
    """(rows,) what the step's per-turbine power contract allows |farm_power_dev - farm_power_ref| to be."""
    tp, _, _ = _tols(out, tol)
    return (tp * np.maximum(np.asarray(out["power"], np.float64), 1e3)).sum(axis=1)


def bound(out, wr, load_coef, tol):
    """(rows,) the bound on |reward_dev - reward_ref| the step's per-turbine contract implies, carried through the formula:
    (1e-3 / wr^3 / N) sum_j tol_power max(P_j, 1e3) + load_coef / (4 N) sum_j (tol_ti + 3 tol_std_j)."""
    N = np.asarray(out["power"]).shape[1]
    _, tti, tstd = _tols(out, tol)
    wr = np.asarray(wr, np.float64)
    return 1e-3 / wr ** 3 / N * power_bound(out, tol) + float(load_coef) / (4.0 * N) * N * (tti + 3.0 * tstd)


def counterfactual(x, y, ws, wd, base, alt, load_coef, wr=None, p=None):
    """ws, wd (B,) a wind per farm; base (B, N), alt (B, N, K) float32 YAWS; wr (B,) the normalising speed (None: ws).
    Returns dict(reward (B, R), farm_power (B, R), difference (B, N, K), same (B, N, K) bool, out: the oracle's outputs of
    all B R rows, wr_rows (B R,))."""
    from oracle import c_oracle

    base, alt = np.asarray(base, np.float32), np.asarray(alt, np.float32)
    B, N, K = alt.shape
    R = 1 + N * K
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    wr = ws if wr is None else np.broadcast_to(np.asarray(wr, np.float64), (B,))
    blk = rows(base, alt)
    out = c_oracle.farm_step_batch(x, y, np.repeat(ws, R), np.repeat(wd, R), blk.reshape(B * R, N).astype(np.float64), p)
    out = {k: np.asarray(v) for k, v in out.items() if k in ("power", "load", "wind_speed", "wind_direction")}
    wr_rows = np.repeat(wr, R)
    rw = reward(out, wr_rows, load_coef).reshape(B, R)
    fp = sums(out)[0].reshape(B, R)
    same = alt.view(np.uint32) == base.view(np.uint32)[:, :, None]
    srow = same.reshape(B, N * K)
    rw[:, 1:] = np.where(srow, rw[:, :1], rw[:, 1:])
    fp[:, 1:] = np.where(srow, fp[:, :1], fp[:, 1:])
    diff = np.where(same, 0.0, (rw[:, :1] - rw[:, 1:]).reshape(B, N, K))
    return {"reward": rw, "farm_power": fp, "difference": diff, "same": same, "out": out, "wr_rows": wr_rows}
