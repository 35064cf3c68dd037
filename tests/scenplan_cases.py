"""TEST INFRASTRUCTURE — the two scenario-planner cases tests/test_scenplan.py (CPU: the reference alone) and
tests/test_scenplan_gpu.py (the device against it) share, and their references, computed once.

  A  eight farms of the row of three (yawopt_ref.ROW3), a wind and a random env state each (test_lookahead._state: open and
     closed gates), K = 8, M = 4, H = 3, E = 3, I = 3, the default widths (1, 1/2, 1/4) yaw_step, no warm start, no anchor,
     tail 1 (the worst member), half the weight on it
  B  16 farms of Ablaincourt, a wind per farm, a random env state, a warm start uniform in [-3, 3], an anchor per farm (the
     current speed scaled by 0.9 to 1.1, the direction turned by up to 5 degrees), K = 8, M = 4, H = 4, E = 3, I = 2, tail 2,
     risk weight 0 (the expected return)
Both under test_lookahead.PARAMS (+-40 deg, 5 deg a step, 0.3 deg/s, 60 s steps, budget 0.1), load_coef 0.1, gamma 0.9,
scenario_ref's PROCESS and the default speed bounds (3, 28).  The seeds were chosen with the reference ALONE
(first_safe_seed: planner and scenario seed both s = 0, 1, 2, ... — the first for which no farm is unsafe under the strict
bounds; tests/test_scenplan.py asserts what they were chosen for), so the GPU tests compare bits on every farm."""
import functools

import numpy as np

import parity
import scenario_ref
import scenplan_ref
import yawopt_ref
from test_lookahead import PARAMS, _state

LOAD_COEF, GAMMA = 0.1, 0.9
PROCESS = scenario_ref.PROCESS
BOUNDS = (3.0, 28.0)
CASES = {
    "A": dict(layout="row3", farms=8, K=8, M=4, H=3, E=3, sigma=(5.0, 2.5, 1.25), tail=1, lam=0.5, seed=0, scenario_seed=0, rng=3,
              warm=False, anchor=False),
    "B": dict(layout="Ablaincourt_", farms=16, K=8, M=4, H=4, E=3, sigma=(5.0, 2.5), tail=2, lam=0.0, seed=0, scenario_seed=0, rng=8,
              warm=True, anchor=True),
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
    """dict(x, y, ws, wd (B,), state, mean0 (B, H, N) or None, anchor (B, 2) or None, and the case's parameters)."""
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
    mean0 = rng.uniform(-3.0, 3.0, (B, H, N)).astype(np.float32) if c["warm"] else None
    anchor = np.stack([ws * rng.uniform(0.9, 1.1, B), wd + rng.uniform(-5.0, 5.0, B)], axis=1) if c["anchor"] else None
    return _freeze(dict(c, x=x, y=y, ws=ws, wd=wd, state=state, mean0=mean0, anchor=anchor, N=N))


@functools.lru_cache(maxsize=None)
def reference(name, strict=True, seeds=None):
    """scenplan_ref.plan of the case, its bounds and margins under parity.TOL_F64 (strict) or parity.TOL (the default mode);
    `seeds` = (planner seed, scenario seed) replaces the case's."""
    c = case(name)
    seed, scenario_seed = (c["seed"], c["scenario_seed"]) if seeds is None else seeds
    return _freeze(scenplan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], c["sigma"], seed,
                                     GAMMA, LOAD_COEF, c["M"], PROCESS, scenario_seed, c["tail"], c["lam"], c["anchor"], BOUNDS,
                                     c["mean0"], tol=parity.TOL_F64 if strict else parity.TOL))


# The limit shapes: the row of three, 2 farms, I = 2, K M H = 4096 at the extremes of each LDS array — (64, 64, 1): more members
# than a wave, 64 candidates a pass of one; (4, 16, 64): the longest horizon, the even stride; (1024, 1, 4): a slot wider than
# one reward tile, a rank count over 1024 scores.  The path tile's several-tiles branch (M H > 2048) is NOT reachable: K >= 3
# leaves M H <= 1365.  name: (K, M, H, E, tail, lam, the inputs' rng, planner seed, scenario seed) — rng and seeds chosen with the
# reference alone so that both farms are safe with a finite margin (tests/test_scenplan.py asserts it)
# "wide1024" is the slot of many floats instead: Turb16_Row5_ (N = 16), K M H = 512, R N = 8192 — the threshold from which the
# advance kernel runs 1024 threads (at the row limit the rewards leave no room for them: the three shapes above run 256)
LIMITS = {"members64": (64, 64, 1, 8, 7, 0.4, 1001, 0, 0), "steps64": (4, 16, 64, 2, 3, 0.4, 20, 7, 9),
          "candidates1024": (1024, 1, 4, 16, 1, 0.0, 1025, 7, 9), "wide1024": (8, 8, 8, 3, 3, 0.4, 16, 0, 0)}
LIMIT_LAYOUT = {"wide1024": "Turb16_Row5_"}
LIMIT_SIGMA = (5.0, 2.5)


@functools.lru_cache(maxsize=None)
def limit_case(name):
    K, M, H, E, tail, lam, rng, seed, scenario_seed = LIMITS[name]
    x, y = yawopt_ref.ROW3
    if name in LIMIT_LAYOUT:
        lay = yawopt_ref.layouts()[LIMIT_LAYOUT[name]]
        x, y = np.asarray(lay["xcoords"], np.float64), np.asarray(lay["ycoords"], np.float64)
    rng = np.random.default_rng(rng)
    ws, wd = rng.uniform(6.0, 12.0, 2), rng.uniform(255.0, 285.0, 2)
    state = _state(rng, 2, len(x))
    state["moves"] = state["moves"].astype(np.int32)
    return _freeze(dict(K=K, M=M, H=H, E=E, tail=tail, lam=lam, seed=seed, scenario_seed=scenario_seed, x=x, y=y, ws=ws, wd=wd,
                        state=state, N=len(x), farms=2))


@functools.lru_cache(maxsize=None)
def limit_reference(name):
    c = limit_case(name)
    return _freeze(scenplan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], LIMIT_SIGMA, c["seed"],
                                     GAMMA, LOAD_COEF, c["M"], PROCESS, c["scenario_seed"], c["tail"], c["lam"], None, BOUNDS))


def first_safe_seed(name, limit=64):
    """The first s = 0, 1, 2, ... for which the case's reference under seeds (s, s) has no unsafe farm under the strict bounds."""
    for s in range(limit):
        if reference(name, True, (s, s))["safe"].all():
            return s
    raise AssertionError(f"case {name}: no seed below {limit} leaves every farm safe")
