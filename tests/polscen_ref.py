"""TEST INFRASTRUCTURE — the reference for policy rollouts over a wind ensemble (include/wfpolscen.h).  It COMPOSES and restates
nothing: scenario_ref.paths (the member paths and their Philox keying), per member policy_ref.rollout(..., wind=paths[:, m],
wr0=the current speed) (the closed loop, over the float64 oracle), and scenario_ref.statistics (mean, ranks by count, tail mean,
score, choice)."""
import functools

import numpy as np

import policy_ref
import scenario_ref

M, TAIL, LAM = 3, 2, 0.5               # odd and no power of two; the two lowest of three
PROCESS = (0.1, 0.5, 0.05, 2.0, 0.5)   # ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp: every term of the recursion is live
STILL = (0.0, 0.0, 0.0, 0.0, 0.0)      # every member path is the current wind held
SEED = 29

# name: (policy_ref case, members, tail); K, H, the network and the env state are the policy case's
CASES = {
    "row3_central": ("row3_central", M, TAIL),
    "row3_shared": ("row3_shared", M, TAIL),
    "row3_discrete": ("row3_discrete", M, TAIL),
    "abl_central": ("abl_central", M, TAIL),
    "horns_central": ("horns_central", M, TAIL),
    "edge": ("abl_shared", 1, 1),        # K = 1, M = 1, H = 1
    "ragged": ("abl_central", 5, 2),     # 7 farms, K = 3, M = 5: chunks of 2 farms under max_eval_farms = 32, the last of 1
}
NAMES = tuple(CASES)


def rollouts(c, ws, wd, M, tail, lam, process, seed, anchor=None, bounds=(3.0, 28.0), farms=None, gamma=None):
    """The composition, for the policy case `c` under current winds ws, wd (B,): dict(wind_paths (B, M, H, 2), member_returns
    (B, K, M), rewards, farm_power (B, K, M, H), actions (B, K, M, H, N), observations, final_yaw (B, K, M, N), gated (B, K, M),
    first_action (B, K, N), expected_returns, cvar, score (B, K), best (B,), latent: scenario_ref.paths' dict)."""
    B, H = len(ws), c["H"]
    farms = np.arange(B) if farms is None else np.asarray(farms)
    pt = scenario_ref.paths(seed, farms, M, H, process, ws, wd, anchor, bounds)
    gamma = c["gamma"] if gamma is None else gamma
    mem = [policy_ref.rollout(c["x"], c["y"], ws, wd, c["state"], c["params"], c["spec"], H, c["env"], gamma, policy_ref.LOAD_COEF,
                              wind=pt["wind"][:, m], wr0=ws) for m in range(M)]
    out = {k: np.stack([r[k] for r in mem], axis=2) for k in ("rewards", "farm_power", "actions", "observations", "final_yaw", "gated")}
    out["member_returns"] = np.stack([r["returns"] for r in mem], axis=2)
    st = scenario_ref.statistics(out["member_returns"], tail, lam)
    out.update({k: st[k] for k in ("expected_returns", "cvar", "score", "best")})
    out["first_action"] = mem[0]["actions"][:, :, 0]
    out["wind_paths"], out["latent"] = pt["wind"], pt
    return out


def build(name, c, members, tail, process=PROCESS):
    """The inputs of an ensemble case over the policy case `c` (policy_ref.build's dict: layout, env state, K parameter vectors,
    spec, H), and the ensemble's: the current wind — the policy case's, with the last two farms turned to 359.5 and 0.5 degrees,
    so that their paths cross 0 / 360 —, bounds whose lower one lies 0.05 m/s below the slowest farm's current speed, so that a
    stored speed of it is clipped, and an anchor per farm for the runs that take one."""
    ws, wd = np.array(c["ws"]), np.array(c["wd"])
    wd[-2:] = (359.5, 0.5)
    bounds = (float(ws.min()) - 0.05, 28.0)
    rng = np.random.default_rng(97)
    anchor = np.stack([ws * rng.uniform(0.9, 1.1, ws.size), wd + rng.uniform(-5.0, 5.0, ws.size)], axis=1)
    for a in (ws, wd, anchor):
        a.setflags(write=False)
    return dict(name=name, c=c, ws=ws, wd=wd, M=members, tail=tail, lam=LAM, process=process, seed=SEED, bounds=bounds, anchor=anchor,
                B=c["B"], N=c["N"], K=c["K"], H=c["H"])


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case of CASES: `build` over its policy_ref case."""
    base, members, tail = CASES[name]
    return build(name, policy_ref.case(base), members, tail)


def reference_of(s):
    """The reference of a case `build` made, frozen."""
    return policy_ref._freeze(rollouts(s["c"], s["ws"], s["wd"], s["M"], s["tail"], s["lam"], s["process"], s["seed"], None, s["bounds"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(case(name))
