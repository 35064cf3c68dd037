"""TEST INFRASTRUCTURE — the reference for flow values at points (include/wfprobe.h), built on the numpy oracle alone.

A probe value is DEFINED as what a rotor-grid point of one additional turbine at that place would see in the sequential
solve, the extra turbine giving no wake to what acts on it and inducing nothing on itself.  So the reference is the oracle
run with one "ghost" turbine appended: zero yaw (no top / bottom vortices) and a huge TSR (no wake-rotation vortex) remove
its self-induced transverse terms; its own deficit reaches only turbines downstream of it, which do not act on it.  The
ghost's 3 x 3 rotor grid gives the flow at nine points per call.
"""
from dataclasses import replace

import numpy as np

from oracle.floris_gch_numpy import ModelParams, farm_step, rotate_layout


def ghost_fields(x, y, ws, wd, yaw, gx, gy, p0=None):
    """The oracle with a ghost turbine at (gx, gy): dict with the ghost's U, V, W (3, 3) [lateral j, vertical k], the real
    turbines' fields `U_real`, `TI_real` (N, 3, 3) in the caller's order, and `sources_ti_uniform`: every real turbine
    upstream of the ghost — the sources that act on it — has one TI for its whole grid, so that "the source's TI at the
    target's grid index" and "the source's centre TI" are the same number.  (The ghost's own wake may well leave a
    turbine DOWNSTREAM of it with a TI per column: that turbine does not act on the ghost.)"""
    p0 = p0 or ModelParams()
    N = len(x)
    p = replace(p0, turbine_defs=[{}, {"TSR": 1e15}], turbine_type_of=[0] * N + [1])
    r = farm_step(np.append(x, gx), np.append(y, gy), ws, wd, np.append(np.asarray(yaw, np.float64), 0.0), p, return_fields=True)
    xr, _ = rotate_layout(np.append(x, gx), np.append(y, gy), wd % 360.0)
    up = xr[:N] <= xr[N]
    uniform = bool(np.ptp(r["TI"][:N].reshape(N, 9)[up], axis=1).max(initial=0.0) == 0.0)
    return {"U": r["U"][N], "V": r["V"][N], "W": r["W"][N], "U_real": r["U"][:N], "TI_real": r["TI"][:N],
            "sources_ti_uniform": uniform}


def ghost_uvw(x, y, ws, wd, yaw, gx, gy, p0=None):
    """The reference flow (3, 3, 3) [j, k, (u, v, w)] at ghost_points(gx, gy, wd), exact under the probe's definition (the
    source's CENTRE TI) whatever the sources' TI grids look like, and whether one ghost was enough.  A ghost's centre column
    always reads the sources' centre TI; its side columns do so only where the sources' TI grids are uniform.  Where they are
    not, each side column is taken as the centre column of a second ghost moved a quarter diameter sideways onto it."""
    p0 = p0 or ModelParams()
    r = ghost_fields(x, y, ws, wd, yaw, gx, gy, p0)
    uvw = np.stack([r["U"], r["V"], r["W"]], axis=-1)
    if not r["sources_ti_uniform"]:
        pts = ghost_points(gx, gy, wd, p0)
        for j in (0, 2):
            s = ghost_fields(x, y, ws, wd, yaw, pts[j, 1, 0], pts[j, 1, 1], p0)
            uvw[j] = np.stack([s["U"][1], s["V"][1], s["W"][1]], axis=-1)
    return uvw, r["sources_ti_uniform"]


def ghost_points(gx, gy, wd, p0=None):
    """Caller-frame coordinates (3, 3, 3) [j, k, xyz] of the ghost's nine rotor-grid points."""
    p0 = p0 or ModelParams()
    dev = np.radians((wd % 360.0 - 270.0) % 360.0)
    o = np.linspace(-p0.D / 4.0, p0.D / 4.0, 3)
    pts = np.empty((3, 3, 3))
    pts[:, :, 0] = (gx + np.sin(dev) * o)[:, None]
    pts[:, :, 1] = (gy + np.cos(dev) * o)[:, None]
    pts[:, :, 2] = (p0.HH + o)[None, :]
    return pts


def wind_frame(x, y, wd):
    """The layout in the wind frame (oracle's rotation about its bounding-box centre) and the map back."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xr, yr = rotate_layout(x, y, wd % 360.0)
    xc, yc = (x.min() + x.max()) / 2.0, (y.min() + y.max()) / 2.0
    dev = np.radians((wd % 360.0 - 270.0) % 360.0)

    def back(xp, yp):
        xo, yo = xp - xc, yp - yc
        return xo * np.cos(dev) + yo * np.sin(dev) + xc, -xo * np.sin(dev) + yo * np.cos(dev) + yc

    return xr, yr, back


def draw_ghosts(rng, x, y, wd, n_down=4, n_up=2, D=126.0):
    """Ghost positions (caller's frame) for one farm: n_down placed 0.5 .. 10 D behind and within 1.5 D beside a random
    turbine (wind frame), n_up upstream of the whole farm; none within 1 m of a turbine's x' (ties, the dx > 0.1 edge).
    Returns (gx, gy, downstream flag)."""
    xr, yr, back = wind_frame(x, y, wd)
    out = []
    while len(out) < n_down + n_up:
        down = len(out) < n_down
        if down:
            t = rng.integers(len(xr))
            xp, yp = xr[t] + rng.uniform(0.5, 10.0) * D, yr[t] + rng.uniform(-1.5, 1.5) * D
        else:
            xp, yp = xr.min() - rng.uniform(0.5, 5.0) * D, rng.uniform(yr.min() - 1.5 * D, yr.max() + 1.5 * D)
        if np.abs(xr - xp).min() < 1.0:
            continue
        gx, gy = back(xp, yp)
        out.append((float(gx), float(gy), down))
    return out
