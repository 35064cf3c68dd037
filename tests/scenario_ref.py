"""TEST INFRASTRUCTURE — the reference for the scenario look-ahead (include/wfscenario.h): the member paths, the rows, the
member returns, the statistics and the float64 bound carry restated in NumPy over lookahead_ref (trajectories, rewards and
returns of one wind per step, over the float64 oracle), credit_ref (the row bound), plan_ref (Philox, the deviate) and
wind_ref (u01).  float64 throughout; every product and sum is one rounding, in the header's order.

  ramp        rate_m = wd_ramp (2 u01(r[0], r[1]) - 1), r = philox(seed, counter (b << 32) | m, stream 16)
  deviate     z(b, m, u, stream) = plan_ref.deviate(seed, farm b, index m 64 + u - 1, stream), streams 17 (speed), 18 (direction)
  tick u      x_u = (x_{u-1} + ws_revert (S_a - x_{u-1})) + ws_sigma z(17),  x_0 = S_c
              y_u = (y_{u-1} + wd_revert ((D_a + rate_m u) - y_{u-1})) + wd_sigma z(18),  y_0 = D_c
              speed_u = clip(x_u, ws_lo, ws_hi);  direction_u = fmod(y_u, 360), + 360 if negative
  rows        step h of sequence k under member m's wind of tick h + 1; step 0 normalised by S_c, step h by speed_h
  statistics  mean = (sum_m ret, ascending m) / M; rank_m = #{j: (ret_j, j) < (ret_m, m)}; cvar = (sum of ranks 0 .. q - 1,
              ascending rank) / q; score = ((1 - lam) mean) + (lam cvar); best = the first maximum of the score
b is the farm's index in the parent's batch: `farms` names it for a sub-list."""
import functools

import numpy as np

import credit_ref
import lookahead_ref
import plan_ref
import wind_ref
from windgen_ref import process_of, wrap360

STREAM_RATE, STREAM_WS, STREAM_WD = 16, 17, 18
MAX_MEMBERS, MAX_ROWS = 64, 4096


def ramp_rates(seed, farms, M, wd_ramp):
    """(n, M) float64 ramp rates of members 0 .. M - 1 of the farms with batch indices `farms`."""
    b = np.asarray(farms, np.uint64).reshape(-1, 1)
    ctr = (b << np.uint64(32)) | np.arange(M, dtype=np.uint64).reshape(1, M)
    r = plan_ref.philox4x32_10(seed, ctr, STREAM_RATE)
    return float(wd_ramp) * (2.0 * wind_ref.u01(r[..., 0], r[..., 1]) - 1.0)


def paths(seed, farms, M, H, process, ws, wd, anchor=None, bounds=(3.0, 28.0)):
    """The member paths of the farms with batch indices `farms` (n,) under current winds ws, wd (n,): dict(wind (n, M, H, 2) —
    what the kernel stores, (speed, direction) of tick h + 1 —, x, y (n, M, H) the latents, rate (n, M)).  anchor (n, 2) or
    None = the current wind."""
    p = process_of(process)
    farms = np.asarray(farms, np.int64).reshape(-1)
    n = farms.size
    Sc = np.broadcast_to(np.asarray(ws, np.float64), (n,)).reshape(n, 1)
    Dc = np.broadcast_to(np.asarray(wd, np.float64), (n,)).reshape(n, 1)
    if anchor is None:
        Sa, Da = Sc, Dc
    else:
        anchor = np.asarray(anchor, np.float64).reshape(n, 2)
        Sa, Da = anchor[:, :1], anchor[:, 1:]
    rate = ramp_rates(seed, farms, M, p["wd_ramp"])
    b = farms.astype(np.uint64).reshape(n, 1)
    m = np.arange(M, dtype=np.uint64).reshape(1, M)
    x, y = np.empty((n, M, H)), np.empty((n, M, H))
    xu, yu = np.repeat(Sc, M, axis=1), np.repeat(Dc, M, axis=1)
    for u in range(1, H + 1):
        idx = m * np.uint64(64) + np.uint64(u - 1)
        zs = plan_ref.deviate(seed, b, idx, STREAM_WS)
        zd = plan_ref.deviate(seed, b, idx, STREAM_WD)
        xu = (xu + p["ws_revert"] * (Sa - xu)) + p["ws_sigma"] * zs
        mu = Da + rate * float(u)
        yu = (yu + p["wd_revert"] * (mu - yu)) + p["wd_sigma"] * zd
        x[:, :, u - 1], y[:, :, u - 1] = xu, yu
    lo, hi = (float(v) for v in bounds)
    wind = np.stack([np.minimum(np.maximum(x, lo), hi), wrap360(y)], axis=-1)
    return {"wind": wind, "x": x, "y": y, "rate": rate}


def ranks(ret):
    """rank_m = #{j: ret_j < ret_m or (ret_j == ret_m and j < m)} along the last axis: (return, m) ascending, a count."""
    M = ret.shape[-1]
    j, m = np.arange(M)[:, None], np.arange(M)[None, :]
    rj, rm = ret[..., :, None], ret[..., None, :]
    return ((rj < rm) | ((rj == rm) & (j < m))).sum(axis=-2)


def statistics(member_returns, tail, lam):
    """dict(expected_returns, cvar, score (..., ) float64, best (...,) over the second-last axis' sequences, ranks) of member
    returns (..., K, M), with the header's summation orders."""
    r = np.asarray(member_returns, np.float64)
    M, q = r.shape[-1], int(tail)
    assert 1 <= q <= M
    total = np.zeros(r.shape[:-1])
    for m in range(M):
        total = total + r[..., m]
    mean = total / np.float64(M)
    rk = ranks(r)
    srt = np.empty_like(r)
    np.put_along_axis(srt, rk, r, axis=-1)
    t = np.zeros(r.shape[:-1])
    for j in range(q):
        t = t + srt[..., j]
    cvar = t / np.float64(q)
    lam = np.float64(lam)
    score = ((np.float64(1.0) - lam) * mean) + (lam * cvar)
    return {"expected_returns": mean, "cvar": cvar, "score": score, "best": np.argmax(score, axis=-1), "ranks": rk, "sorted": srt}


def scenario(x, y, ws, wd, state, actions, env_params, gamma, load_coef, M, process, seed, tail=None, lam=0.0, anchor=None,
             bounds=(3.0, 28.0), farms=None, p=None):
    """ws, wd (B,), state and actions (B, K, H, N) of the LISTED farms, whose batch indices are `farms` (None: 0 .. B - 1).
    Returns dict(expected_returns, cvar, score (B, K), member_returns (B, K, M), rewards (B, K, M, H), wind_paths (B, M, H, 2),
    final_yaw (B, K, N) float32, best (B,), members: lookahead_ref.lookahead's dict of every member — its oracle outputs and
    normalising speeds, for `carry`)."""
    actions = np.asarray(actions, np.float32)
    B, K, H, N = actions.shape
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    farms = np.arange(B) if farms is None else np.asarray(farms, np.int64).reshape(-1)
    pt = paths(seed, farms, M, H, process, ws, wd, anchor, bounds)
    members = [lookahead_ref.lookahead(x, y, ws, wd, state, actions, env_params, gamma, load_coef, wind=pt["wind"][:, m], wr0=ws, p=p)
               for m in range(M)]
    rewards = np.stack([r["rewards"] for r in members], axis=2)  # (B, K, M, H)
    ret = np.stack([r["returns"] for r in members], axis=2)      # (B, K, M)
    st = statistics(ret, M if tail is None else tail, lam)
    return {"expected_returns": st["expected_returns"], "cvar": st["cvar"], "score": st["score"], "best": st["best"],
            "member_returns": ret, "rewards": rewards, "wind_paths": pt["wind"], "final_yaw": members[0]["final_yaw"],
            "latent": pt, "members": members}


def carry(ref, load_coef, tol, gamma, lam):
    """The step's per-turbine contract carried through the definition: dict(rewards (B, K, M, H) = credit_ref.bound per row,
    member_returns (B, K, M) = sum_h g_h bound_h, expected_returns (B, K) = mean_m, cvar (B, K) = max_m — the tail mean is
    1-Lipschitz in the sup norm of the member returns, whatever the ranks do —, score = (1 - lam) mean + lam cvar)."""
    shape = ref["members"][0]["rewards"].shape  # (B, K, H)
    b = np.stack([credit_ref.bound(r["out"], r["wr_rows"], load_coef, tol).reshape(shape) for r in ref["members"]], axis=2)
    rb = (lookahead_ref.discounts(gamma, shape[2]) * b).sum(axis=3)
    mean, worst = rb.mean(axis=2), rb.max(axis=2)
    return {"rewards": b, "member_returns": rb, "expected_returns": mean, "cvar": worst, "score": (1.0 - lam) * mean + lam * worst}


# ---- the cases tests/test_scenario.py asserts the properties of and tests/test_scenario_gpu.py compares the device with ----
NAMES = ("row3", "Ablaincourt_", "Turb6_Row2_", "Turb16_Row5_")  # yawopt_ref.gpu_input: N = 3 to 16, 4 or 32 farms
K, M, H, GAMMA, TAIL, LAM = 4, 5, 3, 0.9, 2, 0.3
PROCESS = (0.1, 0.5, 0.05, 2.0, 0.5)
BOUNDS = (6.5, 11.5)  # inside the cases' 6 to 12 m/s: current speeds near and beyond either bound, so stored speeds are clipped
SEED = 11             # picked on the CPU with the oracle: test_scenario.py and test_scenario_gpu.py assert what it was picked for
PARAMS = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=180.0, budget=0.1)  # tests/test_lookahead_gpu.py's


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """(x, y, ws, wd, state, actions, anchor): the look-ahead GPU tests' layout, winds and env state (the same draws of
    default_rng(61)), K sequences of H continuous actions, sequence 0 all-hold, and an anchor per farm: the current speed
    scaled by 0.9 to 1.1, the current direction turned by up to 5 degrees."""
    import yawopt_ref

    x, y, ws, wd = yawopt_ref.gpu_input(name)
    B, N = len(ws), len(x)
    rng = np.random.default_rng(61)
    state = {"yaw": rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32), "acc": rng.uniform(0.0, 30.0, (B, N)).astype(np.float32),
             "moves": rng.integers(1, 6, B).astype(np.int32)}
    rng = np.random.default_rng(67)
    actions = rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
    actions[:, 0] = 0.0
    anchor = np.stack([ws * rng.uniform(0.9, 1.1, B), wd + rng.uniform(-5.0, 5.0, B)], axis=1)
    for a in (*state.values(), actions, anchor):
        a.setflags(write=False)
    return x, y, ws, wd, state, actions, anchor


@functools.lru_cache(maxsize=None)
def gpu_ref(name, load_coef, seed=SEED):
    x, y, ws, wd, state, actions, anchor = gpu_case(name)
    return scenario(x, y, ws, wd, state, actions, dict(PARAMS, discrete=False), GAMMA, load_coef, M, PROCESS, seed, TAIL, LAM,
                    anchor, BOUNDS)


# paths alone, where the rules bite: 70 farms whose current wind and anchor lie at the circle's seam and at the speed bounds,
# 64 members of 64 ticks (two lay-out tiles), a ramp of up to 3 degrees per tick
EDGE = dict(B=70, M=64, H=64, process=(0.2, 0.8, 0.3, 3.0, 3.0), bounds=(4.0, 9.0), seed=2024)


@functools.lru_cache(maxsize=None)
def edge_case():
    """(ws, wd, anchor, paths): current directions within 6 degrees of 0 / 360, current speeds within 0.5 m/s of a bound;
    anchors within 8 degrees of the current direction — an anchor is not wrapped: 363 means 3 degrees approached across the
    seam, -2 means 358 — and within 0.3 m/s of the same bound."""
    e = EDGE
    rng = np.random.default_rng(71)
    B = e["B"]
    near = np.where(np.arange(B) % 2 == 0, e["bounds"][0], e["bounds"][1])
    ws = near + rng.uniform(-0.5, 0.5, B)
    wd = np.mod(rng.uniform(-6.0, 6.0, B), 360.0)
    anchor = np.stack([near + rng.uniform(-0.3, 0.3, B), wd + rng.uniform(-8.0, 8.0, B)], axis=1)
    pt = paths(e["seed"], np.arange(B), e["M"], e["H"], e["process"], ws, wd, anchor, e["bounds"])
    return ws, wd, anchor, pt
