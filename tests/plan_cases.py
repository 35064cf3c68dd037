"""TEST INFRASTRUCTURE — the two planner cases tests/test_plan.py (CPU: the reference alone) and tests/test_plan_gpu.py (the
device against it) share, and their references, computed once.

  A  eight farms of the row of three (yawopt_ref.ROW3), a wind and a random env state each (test_lookahead._state: open and
     closed gates), K = 8, H = 3, E = 3, I = 3, the default widths (1, 1/2, 1/4) yaw_step, the wind held, no warm start
  B  16 farms of Ablaincourt, a wind per farm and per step (the speed drifts by 2 % a step, the direction turns by 1.5 deg a
     step), a random env state, a warm start uniform in [-3, 3], K = 16, H = 4, E = 4, I = 2
Both under test_lookahead.PARAMS (+-40 deg, 5 deg a step, 0.3 deg/s, 60 s steps, budget 0.1), load_coef 0.1, gamma 0.9.
The seeds were chosen with the reference ALONE (tests/test_plan.py asserts it): every farm of both cases is safe under the
strict bounds, so the GPU tests compare bits on all of them."""
import functools

import numpy as np

import plan_ref
import yawopt_ref
from test_lookahead import PARAMS, _state

LOAD_COEF, GAMMA = 0.1, 0.9
CASES = {
    "A": dict(layout="row3", farms=8, K=8, H=3, E=3, sigma=(5.0, 2.5, 1.25), seed=5, rng=3, wind_per_step=False, warm=False),
    "B": dict(layout="Ablaincourt_", farms=16, K=16, H=4, E=4, sigma=(5.0, 2.5), seed=5, rng=8, wind_per_step=True, warm=True),
}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x, y, ws, wd (B,), state, wind (B, H, 2) or None, mean0 (B, H, N) or None, and the case's parameters)."""
    c = CASES[name]
    if c["layout"] == "row3":
        x, y = yawopt_ref.ROW3
    else:
        lay = yawopt_ref.layouts()[c["layout"]]
        x, y = np.asarray(lay["xcoords"], np.float64), np.asarray(lay["ycoords"], np.float64)
    B, N, H = c["farms"], len(x), c["H"]
    rng = np.random.default_rng(c["rng"])
    ws, wd = rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B)
    state = _state(rng, B, N)
    state["moves"] = state["moves"].astype(np.int32)
    wind = mean0 = None
    if c["wind_per_step"]:
        h = np.arange(H)
        wind = np.stack([ws[:, None] * (1.0 + 0.02 * h), wd[:, None] + 1.5 * h], axis=2)
    if c["warm"]:
        mean0 = rng.uniform(-3.0, 3.0, (B, H, N)).astype(np.float32)
    return _freeze(dict(c, x=x, y=y, ws=ws, wd=wd, state=state, wind=wind, mean0=mean0, N=N))


@functools.lru_cache(maxsize=None)
def reference(name, seed=None):
    """plan_ref.plan of the case under the strict bounds (parity.TOL_F64); `seed` replaces the case's planner seed."""
    c = case(name)
    return _freeze(plan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], c["sigma"],
                                 c["seed"] if seed is None else seed, GAMMA, LOAD_COEF, wind=c["wind"], mean0=c["mean0"]))
