"""TEST INFRASTRUCTURE — the inputs tests/test_retgrad.py (CPU: the reference alone) and tests/test_retgrad_gpu.py (the device
against it) share, and the reference on them, computed once (tests/retgrad_ref.py).

The shapes are the smallest that take each loop of the kernels round at least twice:
  row3   the row of three (N = 3), B = 6, K = 2, H = 5            the base case
  abl    Ablaincourt (N = 7), B = 3, K = 3, H = 4                 a step's rows and a block's sequences beyond one tile / pass
  wide   Ablaincourt, B = 2, K = 40, H = 1                        K N = 280 > 256 threads in the lay-out
  horns  HornsRev1 (N = 80), B = 2, K = 1, H = 2                  turbines beyond one wave; 644 oracle rows
Winds along the rows (speed 7 .. 11 m/s, direction 255 .. 285 deg: waked turbines, where yaw matters), a wind per farm, held
over the horizon.  Env state from default_rng(71): yaw uniform in [4, 30] deg — NOT symmetric about 0: the central difference
at zero yaw on an aligned row is near 0 — with every fifth entry within 3 deg of the upper bound (the state clip takes, the
perturbation is one-sided), acc uniform in [0, 30], moves in 1 .. 5 under dt = 180 s (the gate is closed where
acc >= 5.4 (moves + 1)); actions uniform in [-7, 7] against yaw_step = 5 (the action clip takes on 2 / 7 of them);
load_coef 0.1, gamma 0.9, delta 1."""
import functools

import numpy as np

import retgrad_ref
import yawopt_ref

PARAMS = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=180.0, budget=0.1, discrete=False)
LOAD_COEF, GAMMA, DELTA = 0.1, 0.9, 1.0
CASES = {"row3": ("row3", 6, 2, 5), "abl": ("Ablaincourt_", 3, 3, 4), "wide": ("Ablaincourt_", 2, 40, 1), "horns": ("HornsRev1_", 2, 1, 2)}


def freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            freeze(v)
    return d


def layout(layout_name):
    if layout_name == "row3":
        return yawopt_ref.ROW3
    lay = yawopt_ref.layouts()[layout_name]
    return np.asarray(lay["xcoords"], np.float64), np.asarray(lay["ycoords"], np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x, y, ws, wd (B,), state, actions (B, K, H, N))."""
    layout_name, B, K, H = CASES[name]
    x, y = layout(layout_name)
    N = len(x)
    rng = np.random.default_rng(71)
    yaw = rng.uniform(4.0, 30.0, (B, N))
    near = rng.uniform(37.0, 40.0, (B, N))
    yaw.reshape(-1)[::5] = near.reshape(-1)[::5]
    state = {"yaw": yaw.astype(np.float32), "acc": rng.uniform(0.0, 30.0, (B, N)).astype(np.float32),
             "moves": rng.integers(1, 6, B).astype(np.int32)}
    actions = rng.uniform(-7.0, 7.0, (B, K, H, N)).astype(np.float32)
    return freeze(dict(x=x, y=y, N=N, B=B, K=K, H=H, ws=rng.uniform(7.0, 11.0, B), wd=rng.uniform(255.0, 285.0, B), state=state,
                       actions=actions))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return freeze(retgrad_ref.return_gradient(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["actions"], PARAMS, GAMMA, LOAD_COEF,
                                              delta=DELTA))


def bounds(ref, tol, gamma=GAMMA, load_coef=LOAD_COEF, terminal=None):
    """What the step's per-turbine contract (tests/parity.py, `tol`) allows, carried through the definition: dict(rewards,
    farm_power (B, K, H), returns (B, K), reward_gradient, action_gradient (B, K, H, N), state_gradient (B, K, N),
    rows (B, K, H, W))."""
    import credit_ref
    import lookahead_ref

    B, K, H, N = ref["yaw"].shape
    shape = (B, K, H, 2 * N + 1)
    rb = credit_ref.bound(ref["out"], ref["wr_rows"], load_coef, tol).reshape(shape)
    pb = credit_ref.power_bound(ref["out"], tol).reshape(shape)[..., 0]
    qb = retgrad_ref.quotient_bound(rb, ref["d"])
    agb, sgb = retgrad_ref.sweep_bound(qb, ref["reward_gradient"], ref["pass_mask"], gamma, terminal)
    return {"rewards": rb[..., 0], "farm_power": pb, "returns": (lookahead_ref.discounts(gamma, H) * rb[..., 0]).sum(axis=2),
            "reward_gradient": qb, "action_gradient": agb, "state_gradient": sgb, "rows": rb}
