"""TEST INFRASTRUCTURE — the inputs tests/test_series.py (CPU: the references alone) and tests/test_series_gpu.py (the device
against them) share, and the planner's reference on them, computed once.

  series(T)   T rows; the speed rises by 0.4 m/s every SECOND row (rows 2 j and 2 j + 1 share it), the direction swings around
              270 deg by a few degrees a row, in quarters of a degree (exact through a CSV file and the host env's arithmetic):
              consecutive ticks differ always in direction and every other time in speed — so
              a farm whose pending speed (the tick before) equals its current one exists next to farms where it differs
  plan case   8 farms of a layout on series(12), start rows that cover both kinds and the wrap past T - 1, one tick made
              (t = 1, the speed of tick 0 pending: the state right after a reset), a random env state with open and closed
              gates (test_lookahead._state), K = 8, H = 3, E = 3, the default widths, under test_lookahead.PARAMS,
              load_coef 0.1, gamma 0.9.  The planner's seeds were chosen with the reference ALONE (tests/test_series.py
              asserts it): every farm is safe under the strict bounds, so the GPU test compares bits on all of them."""
import functools

import numpy as np

import plan_ref
import series_ref
import yawopt_ref
from test_lookahead import PARAMS, _state

LAYOUTS = ("Turb3_Row1_", "Turb6_Row2_")
LOAD_COEF, GAMMA = 0.1, 0.9
PLAN = dict(farms=8, T=12, t=1, K=8, H=3, E=3, sigma=(5.0, 2.5, 1.25), rng=17,
            start=(0, 1, 4, 11, 7, 10, 5, 2), seed={"Turb3_Row1_": 5, "Turb6_Row2_": 8})  # (the widest margins of seeds 1..8: 1.1e-3, 8e-4)


def series(T):
    k = np.arange(T)
    s = np.stack([7.0 + 0.4 * (k // 2), np.round((270.0 + 6.0 * np.sin(1.3 * k) + 0.25 * k) * 4.0) / 4.0], axis=1)
    s.setflags(write=False)
    return s


def layout(name):
    lay = yawopt_ref.layouts()[name]
    return np.asarray(lay["xcoords"], np.float64), np.asarray(lay["ycoords"], np.float64)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def plan_case(name):
    """dict(x, y, series, start, t, state, ws, wd — the wind of tick t —, rows (B, H, 2) — the window (1, H) —, and PLAN)."""
    c = PLAN
    x, y = layout(name)
    B, N = c["farms"], len(x)
    s = series(c["T"])
    start = np.asarray(c["start"], np.int32)
    state = _state(np.random.default_rng(c["rng"]), B, N)
    state["moves"] = state["moves"].astype(np.int32)
    cur = series_ref.window(s, start, c["t"], 0, 1)[0][:, 0]
    rows, avail = series_ref.window(s, start, c["t"], 1, c["H"])
    assert avail == c["H"]
    return _freeze(dict(c, x=x, y=y, N=N, series=s, start=start, state=state, ws=cur[:, 0].copy(), wd=cur[:, 1].copy(), rows=rows,
                        seed=c["seed"][name]))


@functools.lru_cache(maxsize=None)
def plan_reference(name):
    """plan_ref.plan of the case under the strict bounds: row h under window entry h, step 0 normalised by the CURRENT speed."""
    c = plan_case(name)
    return _freeze(plan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], c["sigma"], c["seed"],
                                 GAMMA, LOAD_COEF, wind=c["rows"], wr0=c["ws"]))
