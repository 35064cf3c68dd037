"""TEST INFRASTRUCTURE — the reference for the scenario rollouts of yaw-table controllers (include/wfrollscen.h).  It COMPOSES
existing references and contains no new physics:

  paths       scenario_ref.paths — the member paths of include/wfscenario.h
  a member    rollout_ref.rollout(..., wind=path_m, wr0=the current speed, filter0=...) — the controller of include/wfrollout.h
              in closed loop under member m's winds, its rows over the float64 oracle, its rewards and its return
  statistics  scenario_ref.statistics of the (B, K, M) member returns
  bounds      credit_ref.bound per row, carried by scenario_ref.carry (parity.TOL / parity.TOL_F64)
It also defines the cases the CPU and GPU tests share (`CASES`, `case`, `reference`) and the condition their seeds were picked
for (`clear`)."""
import functools

import numpy as np

import rollout_ref as rr
import scenario_ref as S
import yawopt_ref

WANT = ("expected_returns", "cvar", "score", "member_returns", "rewards", "wind_paths", "actions", "final_yaw", "gated",
        "first_action", "best")
FREE = ("wind_paths", "actions", "final_yaw", "gated", "first_action")  # what does not depend on the solver
MAX_K, MAX_ROWS, LDS_RECORDS = 64, 4096, 1024


def rollscen(x, y, ws, wd, state, controllers, tables, H, env_params, gamma, load_coef, M, process, seed, tail=None, lam=0.0,
             anchor=None, bounds=(3.0, 28.0), filter0=None, farms=None, p=None):
    """ws, wd (B,) and state of the LISTED farms, whose batch indices are `farms` (None: 0 .. B - 1).  Returns
    dict(expected_returns, cvar, score (B, K), member_returns (B, K, M), rewards (B, K, M, H), wind_paths (B, M, H, 2), actions
    (B, K, M, H, N) float32, final_yaw (B, K, M, N) float32, gated (B, K, M) int32, first_action (B, K, N) float32, best (B,),
    members: rollout_ref.rollout's dict of every member — its oracle outputs and normalising speeds, for scenario_ref.carry)."""
    B = np.asarray(state["yaw"]).shape[0]
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    farms = np.arange(B) if farms is None else np.asarray(farms, np.int64).reshape(-1)
    pt = S.paths(seed, farms, M, H, process, ws, wd, anchor, bounds)
    members = [rr.rollout(x, y, ws, wd, state, controllers, tables, H, env_params, gamma, load_coef, wind=pt["wind"][:, m], wr0=ws,
                          filter0=filter0, p=p) for m in range(M)]
    ret = np.stack([r["returns"] for r in members], axis=2)
    st = S.statistics(ret, M if tail is None else tail, lam)
    return {"expected_returns": st["expected_returns"], "cvar": st["cvar"], "score": st["score"], "best": st["best"],
            "member_returns": ret, "rewards": np.stack([r["rewards"] for r in members], axis=2), "wind_paths": pt["wind"],
            "actions": np.stack([r["actions"] for r in members], axis=2), "final_yaw": np.stack([r["final_yaw"] for r in members], axis=2),
            "gated": np.stack([r["gated_count"] for r in members], axis=2).astype(np.int32),
            "first_action": members[0]["actions"][:, :, 0].copy(), "latent": pt, "members": members}


def clear(ref, load_coef, tol, gamma, lam):
    """(B,) bool: the two best reference scores of the farm are further apart than the sum of their two bounds — where `best`
    must be the reference's.  K = 1: nothing to order."""
    sc = ref["score"]
    if sc.shape[1] < 2:
        return np.ones(sc.shape[0], bool)
    sb = S.carry(ref, load_coef, tol, gamma, lam)["score"]
    rows = np.arange(sc.shape[0])
    order = np.argsort(-sc, axis=1, kind="stable")
    first, second = order[:, 0], order[:, 1]
    return sc[rows, first] - sc[rows, second] > sb[rows, first] + sb[rows, second]


# ---- the cases tests/test_rollscen.py asserts the properties of and tests/test_rollscen_gpu.py compares the device with ------
CONTROLLERS = dict(alpha=[1.0, 0.4, 0.7], deadband=[0.0, 2.0, 0.5], lead=[0, 1, 5], slot=[0, 1, 1])  # lead 5 > H: the clamp min(h + lead, H)
M, H, GAMMA, TAIL, LAM = 5, 4, 0.9, 2, 0.3
COEFS = (0.1, 1.0)
RING = np.arange(5.0, 360.0, 10.0)  # the whole circle, no node at 0: north lies in the table's circular bracket
TWS = np.array([6.0, 8.0, 10.0, 12.0])

# name: layout, farms, the wind process and speed bounds, discrete, the seed of the draws, the controllers, M, H, what it is aimed at.
# The seeds were picked WITH THIS REFERENCE (tests/test_rollscen.py asserts the condition): on every farm of every case, under
# both load coefficients, the two best scores are further apart than the sum of their two default-mode bounds (`clear`).
CASES = {
    # the row of three under its four winds, continuous control: anchors, clipped speeds, a farm at 0 degrees
    "row3": dict(layout="row3", B=4, discrete=False, seed=0),
    # ... under discrete control, where a closed gate moves the yaw "down" and stays closed: a state draw of its own, in which
    # no farm has all three turbines gated from the start (such a farm's controllers tie exactly)
    "row3_discrete": dict(layout="row3", B=4, discrete=True, seed=1, state_seed=62),
    # N = 16, 32 farms under any wind direction: more than one wave of trajectories per (k, m), chunks
    "Turb16_Row5_": dict(layout="Turb16_Row5_", B=32, discrete=False, seed=237),
    # the seam: current winds within 6 degrees of 0 / 360, filter states on the other side of it, paths that cross it: the
    # filter's wrap, the stored direction's wrap and the table's circular bracket
    "seam": dict(layout="row3", B=6, discrete=False, seed=0, M=5, H=6, process=(0.2, 0.8, 0.3, 3.0, 3.0), bounds=(4.0, 9.0)),
    # the limits, K M H = 4096 rows on three farms of the row of three: the brackets go through global memory, 64 members, 64
    # ticks (two lay-out tiles), 64 controllers, the reduce kernel's 1024 threads
    "members64": dict(layout="row3", B=3, discrete=False, seed=0, K=1, M=64, H=64),
    "controllers64": dict(layout="row3", B=3, discrete=False, seed=307, K=64, M=8, H=8),
    "steps64": dict(layout="row3", B=3, discrete=False, seed=0, K=4, M=16, H=64),
    # either side of the switch between brackets in LDS and in global memory: 1024 rows and 1040
    "records1024": dict(layout="row3", B=3, discrete=False, seed=0, K=4, M=16, H=16),
    "records1040": dict(layout="row3", B=3, discrete=False, seed=0, K=5, M=13, H=16),
    # five farms for the chunked run of a farm list
    "chunks": dict(layout="row3", B=5, discrete=False, seed=1),
}
BASE = ("row3", "row3_discrete", "Turb16_Row5_", "seam")
LIMITS = ("members64", "controllers64", "steps64", "records1024", "records1040")


def ring_table(x, shift, seed):
    """rollout_ref.steering_table's sine period of +-45 degrees repeated around the circle (centres shift + 0, 90, 180, 270:
    the four pieces tile it): the winds of the cases come from any direction, and a target that swings by up to 1.7 degrees per
    degree of wind tells controllers with different filters apart."""
    return sum(rr.steering_table(x, RING, TWS, shift + c, 45.0, seed) for c in (0.0, 90.0, 180.0, 270.0))


def grid(K):
    """K controllers over the two table slots: the three of CONTROLLERS first (K >= 3), then a grid of gains, deadbands and
    leads — every one different from the others."""
    base = {k: list(v) for k, v in CONTROLLERS.items()}
    if K <= 3:
        return {k: v[:K] for k, v in base.items()}
    i = np.arange(K - 3)
    base["alpha"] += list(0.15 + 0.8 * ((i * 7) % 16) / 16.0)
    base["deadband"] += list(0.25 * (i % 11))
    base["lead"] += list((i % 4).astype(int))
    base["slot"] += list((i % 2).astype(int))
    return base


def _freeze(obj):
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            _freeze(v)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            _freeze(v)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x, y, ws, wd (B,), state, tables {slot: (T, twd, tws, interp)}, controllers, K, M, H, B, N, env, gamma, tail, lam,
    process, bounds, seed, anchor (B, 2), filter0 (B, K, 2) or None) — read-only.  Layouts and winds are yawopt_ref.gpu_input's,
    the env state is the scenario tests' draw (default_rng(61)) under env_config(dt=180)."""
    c = CASES[name]
    x, y, ws, wd = yawopt_ref.gpu_input(c["layout"])
    B, N = c["B"], len(x)
    rng = np.random.default_rng(c.get("state_seed", 61))
    if name == "seam":
        near = np.where(np.arange(B) % 2 == 0, c["bounds"][0], c["bounds"][1])
        ws = near + rng.uniform(-0.5, 0.5, B)
        wd = np.mod(rng.uniform(-6.0, 6.0, B), 360.0)
    else:
        ws, wd = np.resize(ws, B).astype(np.float64), np.resize(wd, B).astype(np.float64)
        if B > len(yawopt_ref.gpu_input(c["layout"])[2]):  # (the fifth farm of the chunked case: a wind of its own)
            ws[4:], wd[4:] = 8.5, 265.0
    # yaw and move counter as the scenario tests draw them.  The accumulator is drawn RELATIVE to the gate, as rollout_ref.case
    # does: under dt = 180 the gate of step h closes at acc >= 5.4 (moves + 1 + h), and scenario_ref's uniform(0, 30) leaves
    # every farm with moves == 1 gated through the whole horizon — all controllers then hold the same yaw and tie exactly, which
    # no seed can separate.  Up to 1.25 of the first step's threshold: a fifth of the turbines start gated and open again.
    moves = rng.integers(1, 6, B).astype(np.int32)
    state = {"yaw": rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32),
             "acc": (rng.uniform(0.0, 1.25, (B, N)) * 5.4 * (moves[:, None] + 1)).astype(np.float32), "moves": moves}
    K = c.get("K", 3)
    ctl, K = rr.broadcast_controllers(grid(K))
    rng = np.random.default_rng(67)
    anchor = np.stack([ws * rng.uniform(0.9, 1.1, B), wd + rng.uniform(-5.0, 5.0, B)], axis=1)
    filter0 = None
    if name == "seam":  # filter states across the seam from the current direction, not reduced to [0, 360)
        filter0 = np.stack([np.repeat(ws[:, None], K, axis=1) + rng.uniform(-0.5, 0.5, (B, K)),
                            np.where(wd[:, None] < 180.0, 360.0 - rng.uniform(0.0, 8.0, (B, K)), rng.uniform(0.0, 8.0, (B, K)))], axis=2)
    tables = {0: (ring_table(x, 0.0, 1), RING, TWS, "nearest"), 1: (ring_table(x, 20.0, 2), RING, TWS, "linear")}
    out = dict(x=x, y=y, ws=ws, wd=wd, state=state, tables=tables, controllers=ctl, K=K, M=c.get("M", M), H=c.get("H", H), B=B, N=N,
               env=dict(S.PARAMS, discrete=c["discrete"]), gamma=GAMMA, tail=TAIL, lam=LAM, process=c.get("process", S.PROCESS),
               bounds=c.get("bounds", S.BOUNDS), seed=c["seed"], anchor=anchor, filter0=filter0)
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, load_coef=0.1, extra=0):
    """`rollscen` of a case — read-only.  extra: that many further controllers are appended (they must not change the first K's
    outputs)."""
    c = case(name)
    ctl = c["controllers"]
    if extra:
        more = {"alpha": [0.55] * extra, "deadband": [1.25] * extra, "lead": [2] * extra, "slot": [1] * extra}
        ctl = {k: np.concatenate([ctl[k], np.asarray(more[k], ctl[k].dtype)]) for k in ctl}
    r = rollscen(c["x"], c["y"], c["ws"], c["wd"], c["state"], ctl, c["tables"], c["H"], c["env"], c["gamma"], load_coef, c["M"],
                 c["process"], c["seed"], c["tail"], c["lam"], c["anchor"], c["bounds"], c["filter0"])
    _freeze(r)
    return r
