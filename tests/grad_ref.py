"""TEST INFRASTRUCTURE — the reference for the yaw sensitivities (include/wfgrad.h): a plain NumPy restatement of the
difference quotients over the float64 oracle, which it does not modify.  The step functions are those of tests/yawopt_ref.py.

The definition, as the header states it, for a yaw row y (float32 values), a step h > 0 and bounds lo < hi:
  perturbed yaws  y+_i = float32(min(float64(y_i) + h, hi)),  y-_i = float32(max(float64(y_i) - h, lo))
  divisor         d_i = float64(y+_i) - float64(y-_i); where d_i <= 0 every sensitivity of turbine i is exactly 0
  rows            R = 2 N + 1 per farm: row 0 the yaw as given, row 2 i + 1 with y_i -> y+_i, row 2 i + 2 with y_i -> y-_i
  Jacobian        J[i, j] = (P_j(row 2 i + 1) - P_j(row 2 i + 2)) / d_i
  gradient        G[i] = S_i / d_i,  S_i = sum_j float64(c_j) (P+_j - P-_j) over j in caller order, every product and sum
                  rounded on its own
  power           row 0's per-turbine power
P is the oracle's float64 per-turbine power (the device's is the step's float32 power: the GPU tests bound the difference)."""
import numpy as np

import yawopt_ref


def perturbed(yaw, h=1.0, bounds=(-45.0, 45.0)):
    """(y+, y-, d): float32, float32, float64 arrays of yaw's shape."""
    y = np.asarray(yaw, np.float32).astype(np.float64)
    lo, hi = float(bounds[0]), float(bounds[1])
    yp = np.minimum(y + float(h), hi).astype(np.float32)
    ym = np.maximum(y - float(h), lo).astype(np.float32)
    return yp, ym, yp.astype(np.float64) - ym.astype(np.float64)


def rows(yaw, h=1.0, bounds=(-45.0, 45.0)):
    """(B, 2 N + 1, N) float32: the evaluator's yaw block."""
    yaw = np.atleast_2d(np.asarray(yaw, np.float32))
    B, N = yaw.shape
    yp, ym, _ = perturbed(yaw, h, bounds)
    blk = np.repeat(yaw[:, None, :], 2 * N + 1, axis=1)
    for i in range(N):
        blk[:, 2 * i + 1, i] = yp[:, i]
        blk[:, 2 * i + 2, i] = ym[:, i]
    return blk


def gradient(x, y, ws, wd, yaw, cotangent=None, h=1.0, bounds=(-45.0, 45.0), p=None, step=None):
    """ws, wd (B,) a wind per farm, yaw (B, N) float32 values, cotangent (B, N) float32 values or None = ones.
    Returns dict(power (B, N), jacobian (B, N, N), gradient (B, N), d (B, N), p_plus / p_minus (B, N, N): P_j of rows
    2 i + 1 / 2 i + 2 as [b, i, j]), float64.  step: `yawopt_ref.numpy_step` for the NumPy oracle; default the C restatement."""
    yaw = np.atleast_2d(np.asarray(yaw, np.float32))
    B, N = yaw.shape
    R = 2 * N + 1
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    c = np.ones((B, N)) if cotangent is None else np.asarray(cotangent, np.float32).astype(np.float64).reshape(B, N)
    fn = step or yawopt_ref._c_step
    blk = rows(yaw, h, bounds)
    pw = fn(x, y, np.repeat(ws, R), np.repeat(wd, R), blk.reshape(B * R, N).astype(np.float64), p or yawopt_ref.ModelParams())
    pw = np.asarray(pw, np.float64).reshape(B, R, N)
    d = perturbed(yaw, h, bounds)[2]
    pp, pm = pw[:, 1::2, :].copy(), pw[:, 2::2, :].copy()  # [b, i, j]
    live = d > 0.0
    J = np.where(live[:, :, None], (pp - pm) / np.where(live, d, 1.0)[:, :, None], 0.0)
    return {"power": pw[:, 0, :].copy(), "jacobian": J, "gradient": vjp(pp, pm, d, c), "d": d, "p_plus": pp, "p_minus": pm}


def vjp(p_plus, p_minus, d, cotangent):
    """G (B, N) from the perturbed rows' powers [b, i, j], the divisors (B, N) and the cotangent (B, N) float32 values: the sum
    over j in caller order, every product and sum rounded on its own."""
    c = np.asarray(cotangent, np.float32).astype(np.float64)
    diff = p_plus - p_minus
    S = np.zeros(d.shape)
    for j in range(d.shape[1]):
        S = S + c[:, None, j] * diff[:, :, j]
    live = d > 0.0
    return np.where(live, S / np.where(live, d, 1.0), 0.0)
