"""GPU: scenario look-ahead on the device (include/wfscenario.h) against tests/scenario_ref.py — the same member paths, rows,
rewards, member returns and statistics in NumPy over the float64 oracle.

The paths are compared BIT FOR BIT.  The bounds of everything that passes through the step need no measured number: the
step's contract is per turbine (tests/parity.py), carried through the reward's formula by credit_ref.bound per ROW — TOL_F64
when every row is solved in float64 (strict), TOL in the handle's default mode —; a member return is held to
sum_h g_h bound_h, the mean to the mean of its members' bounds, the tail mean to the largest of them (it is 1-Lipschitz in the
sup norm of the member returns, whatever the ranks do), the score to (1 - lam) and lam times those (scenario_ref.carry), on
EVERY entry; nothing is exempted.  The statistics themselves are checked without any tolerance: they are scenario_ref's
statistics of the device's OWN member returns, bit for bit.

Inputs (scenario_ref.gpu_case, asserted on the CPU in tests/test_scenario.py): the look-ahead GPU tests' layouts, winds and
env state under env_config(dt=180); K = 4 sequences of H = 3 steps, sequence 0 all-hold, M = 5 members (not a power of two),
gamma 0.9, load_coef 0.1 and 1.0, process (0.1, 0.5, 0.05, 2.0, 0.5), tail 2, risk weight 0.3, an anchor per farm and speed
bounds inside the winds' range, so that clipped speeds occur; and the edge case: paths alone at the circle's seam and at the
speed bounds.

Bit identity across chunk sizes and farm lists is asserted in STRICT mode, where every row is solved by the float64 kernel,
whose bits do not depend on the batch; in the default mode only two runs on the same evaluator are compared."""
import functools

import numpy as np
import pytest

import lookahead_ref
import parity
import scenario_ref as S
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

COEFS = (0.1, 1.0)
WANT = ("expected_returns", "cvar", "score", "member_returns", "rewards", "wind_paths", "final_yaw", "best")
STATS = ("expected_returns", "cvar", "score")
PROC = S.process_of(S.PROCESS)
BASE = dict(members=S.M, process=PROC, seed=S.SEED, gamma=S.GAMMA, tail=S.TAIL, risk_weight=S.LAM, bounds=S.BOUNDS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    """Two env states (nested dicts of arrays, numbers and None) compare equal."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(np.asarray(a), np.asarray(b)))


def _handle(name, lc, state=True):
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, st = S.gpu_case(name)[:5]
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    w.env_config(load_coef=lc, discrete=False, dt=S.PARAMS["dt"])
    if state:
        w.env_reset()
        w.env_set_state(st)
    return w


@functools.lru_cache(maxsize=None)
def _device(name, strict, lc):
    w = _handle(name, lc)
    actions, anchor = S.gpu_case(name)[5:]
    r = w.scenario_returns(actions, anchor=anchor, strict=strict, want=WANT, **BASE)
    w.close()
    for v in r.values():
        v.setflags(write=False)
    return r


def _own_statistics(got, tail, lam, gamma):
    """The device's statistics are scenario_ref's of its OWN member returns, and those the discounted sums of its own rewards."""
    assert np.array_equal(_bits(got["member_returns"]), _bits(lookahead_ref.discounted(got["rewards"], gamma)))
    st = S.statistics(got["member_returns"], tail, lam)
    for k in STATS:
        assert np.array_equal(_bits(got[k]), _bits(st[k])), k
    assert np.array_equal(got["best"], st["best"])


def _against_reference(ref, got, lc, tol, gamma, lam, label):
    c = S.carry(ref, lc, tol, gamma, lam)
    worst = {}
    for k in ("rewards", "member_returns") + STATS:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64, k
        err = np.abs(got[k] - ref[k])
        worst[k] = float((err / c[k]).max())
    print(f"{label}: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (label, k, v)
    return c


def _check(name, strict, tol):
    for lc in COEFS:
        ref, got = S.gpu_ref(name, lc), _device(name, strict, lc)
        B, N = ref["final_yaw"].shape[0], ref["final_yaw"].shape[2]
        assert got["wind_paths"].shape == (B, S.M, S.H, 2) and got["wind_paths"].dtype == np.float64
        assert got["final_yaw"].shape == (B, S.K, N) and got["final_yaw"].dtype == np.float32
        assert got["best"].shape == (B,) and got["best"].dtype == np.int32
        assert got["rewards"].shape == (B, S.K, S.M, S.H) and got["member_returns"].shape == (B, S.K, S.M)
        label = f"{name} {'strict' if strict else 'default mode'} load_coef {lc}"
        c = _against_reference(ref, got, lc, tol, S.GAMMA, S.LAM, label)
        spread = np.median(ref["score"].max(axis=1) - ref["score"].min(axis=1))
        assert spread >= 50.0 * np.median(c["score"]), label  # (what is checked is far larger than what is allowed)
        assert np.array_equal(_bits(got["final_yaw"]), _bits(ref["final_yaw"]))


def test_wind_paths_have_the_bits_of_the_reference():
    """Every stored (speed, direction) of every member and tick, on the base cases — with anchors, clipped speeds and, on the
    row of three, wrapped directions — and on the edge case: 70 farms at the circle's seam and at the speed bounds, 64 members
    of 64 ticks (two lay-out tiles, five chunks), where about half the speeds are clipped and half the directions wrapped."""
    from wfcrl_env_amd.backend import WfStep

    for name in S.NAMES:
        ref, got = S.gpu_ref(name, 0.1), _device(name, False, 0.1)
        assert np.array_equal(_bits(got["wind_paths"]), _bits(ref["wind_paths"])), name
        assert np.array_equal(_bits(_device(name, True, 1.0)["wind_paths"]), _bits(ref["wind_paths"])), name
    ws, wd, anchor, pt = S.edge_case()
    e = S.EDGE
    x, y = ROW3
    w = WfStep(x, y, env_batch=e["B"])
    w.set_wind(ws, wd)
    w.env_config()
    w.env_reset()
    held = w.get_wind()
    got = w.scenario_returns(np.zeros((e["B"], 1, e["H"], 3), np.float32), e["M"], S.process_of(e["process"]), seed=e["seed"],
                             anchor=anchor, bounds=e["bounds"], want=("wind_paths", "best"))
    w.close()
    assert np.array_equal(_bits(np.asarray(held[0], np.float64)), _bits(ws)) and np.array_equal(_bits(np.asarray(held[1], np.float64)), _bits(wd))
    assert got["wind_paths"].shape == (e["B"], e["M"], e["H"], 2)
    clipped, wrapped = pt["x"] != pt["wind"][..., 0], pt["y"] != pt["wind"][..., 1]
    assert clipped.mean() > 0.25 and wrapped.mean() > 0.25
    same = _bits(got["wind_paths"]) == _bits(pt["wind"])
    assert same[..., 0][clipped].all() and same[..., 1][wrapped].all()
    assert same.all(), np.argwhere(~same)[:5]
    assert (got["best"] == 0).all()  # K = 1


@pytest.mark.parametrize("name", S.NAMES)
def test_strict_against_the_reference(name):
    """Every row solved in float64: every reward, member return, mean, tail mean and score inside the bounds that follow
    from TOL_F64, with both load coefficients; final_yaw has the reference's bits."""
    _check(name, True, parity.TOL_F64)


@pytest.mark.parametrize("name", S.NAMES)
def test_default_mode_against_the_reference(name):
    """The handle's own resolve mode: the same inequalities from TOL.  Nothing is exempted."""
    _check(name, False, parity.TOL)


@pytest.mark.parametrize("strict", [True, False])
def test_statistics_are_those_of_the_devices_own_member_returns(strict):
    for name in S.NAMES:
        for lc in COEFS:
            _own_statistics(_device(name, strict, lc), S.TAIL, S.LAM, S.GAMMA)


def test_degenerate_ends():
    """Zero sigmas and zero ramp (strict): all members of a sequence have the same bits, those of lookahead_returns under
    the held wind.  M = 1: expected == cvar == member.  tail = 1: the exact minimum.  tail = M: cvar and expected agree to the
    rounding of two summation orders of the same M numbers — each sum is within (M - 1) 2^-53 sum|ret| of the exact one and
    each division adds 2^-53 of the quotient: |cvar - expected| <= 2 M 2^-53 mean|ret|.  risk_weight = 0: score has the bits
    of expected_returns.  A duplicated sequence: equal members, equal scores, and best is never the later copy."""
    name, lc = "Ablaincourt_", 0.1
    actions = S.gpu_case(name)[5]
    B = actions.shape[0]
    w = _handle(name, lc)
    kw = dict(gamma=S.GAMMA, strict=True, want=WANT)
    still = w.scenario_returns(actions, 2, dict(ws_revert=0.3, wd_revert=0.7), seed=3, tail=2, risk_weight=0.5, **kw)
    held = w.lookahead_returns(actions, gamma=S.GAMMA, strict=True, want=("returns", "rewards", "best", "final_yaw"))
    one = w.scenario_returns(actions, 1, PROC, seed=S.SEED, **kw)
    low = w.scenario_returns(actions, S.M, PROC, seed=S.SEED, tail=1, risk_weight=1.0, **kw)
    full = w.scenario_returns(actions, S.M, PROC, seed=S.SEED, tail=None, risk_weight=0.0, **kw)
    top = actions[np.arange(B), full["best"]]
    three = np.stack([actions[:, 0], top, top], axis=1)
    dup = w.scenario_returns(three, S.M, PROC, seed=S.SEED, tail=2, risk_weight=0.3, **kw)
    w.close()
    for m in range(2):
        assert np.array_equal(_bits(still["member_returns"][:, :, m]), _bits(held["returns"])), m
        assert np.array_equal(_bits(still["rewards"][:, :, m]), _bits(held["rewards"])), m
    for k in STATS:
        assert np.array_equal(_bits(still[k]), _bits(held["returns"])), k  # (two equal terms: r + r, / 2 and 0.5 r + 0.5 r are exact)
    assert np.array_equal(still["best"], held["best"]) and np.array_equal(_bits(still["final_yaw"]), _bits(held["final_yaw"]))
    for k in ("expected_returns", "cvar"):
        assert np.array_equal(_bits(one[k]), _bits(one["member_returns"][:, :, 0])), k
    assert np.array_equal(_bits(low["cvar"]), _bits(low["member_returns"].min(axis=2)))
    assert np.array_equal(_bits(low["score"]), _bits(low["cvar"]))  # (weight 1: (0 mean) + (1 cvar))
    assert np.array_equal(_bits(full["score"]), _bits(full["expected_returns"]))
    allow = 2.0 * S.M * 2.0 ** -53 * np.abs(full["member_returns"]).mean(axis=2)
    assert (np.abs(full["cvar"] - full["expected_returns"]) <= allow).all()
    assert np.array_equal(_bits(low["member_returns"]), _bits(full["member_returns"]))  # (tail and weight do not reach the rows)
    _own_statistics(one, 1, 0.0, S.GAMMA); _own_statistics(low, 1, 1.0, S.GAMMA); _own_statistics(full, S.M, 0.0, S.GAMMA)
    assert np.array_equal(_bits(dup["member_returns"][:, 1]), _bits(dup["member_returns"][:, 2]))
    assert np.array_equal(_bits(dup["score"][:, 1]), _bits(dup["score"][:, 2])) and (dup["best"] != 2).all()
    assert (dup["best"] == 1).any()
    _own_statistics(dup, 2, 0.3, S.GAMMA)


@pytest.mark.parametrize("strict", [True, False])
def test_best(strict):
    """best is the first maximum of the device's own score; the reference score of the device's choice is no lower than the
    reference maximum minus the two sequences' score bounds, on every farm; in strict mode it IS the reference's best on every
    farm whose top two reference scores are further apart than their two bounds — at least three quarters of the farms
    (asserted on the reference alone; what scenario_ref.SEED was picked for)."""
    tol = parity.TOL_F64 if strict else parity.TOL
    for name in S.NAMES:
        for lc in COEFS:
            ref, got = S.gpu_ref(name, lc), _device(name, strict, lc)
            sb = S.carry(ref, lc, tol, S.GAMMA, S.LAM)["score"]
            rows = np.arange(sb.shape[0])
            best, top, sc = got["best"], ref["best"], ref["score"]
            assert ((best >= 0) & (best < S.K)).all()
            assert np.array_equal(best, np.argmax(got["score"], axis=1))
            assert (sc[rows, best] >= sc[rows, top] - (sb[rows, best] + sb[rows, top])).all(), (name, lc)
            if strict:
                order = np.argsort(-sc, axis=1, kind="stable")
                first, second = order[:, 0], order[:, 1]
                clear = sc[rows, first] - sc[rows, second] > sb[rows, first] + sb[rows, second]
                assert clear.mean() >= 0.75, (name, lc)  # (the reference alone)
                assert np.array_equal(best[clear], top[clear]), (name, lc)


def test_same_bits():
    """Strict: max_eval_farms = R + 1 (a farm per chunk) and 3 R + 1 (32 farms in chunks of 3 and a ragged 2), a shuffled
    sub-list of farms — whose paths are those of the farms' indices in the batch — and torch tensors in and out give all the
    bits of the whole NumPy run.  Two default-mode runs on one evaluator agree bit for bit."""
    import torch

    name, lc = "Ablaincourt_", 0.1
    actions, anchor = S.gpu_case(name)[5:]
    B, R = actions.shape[0], S.K * S.M * S.H
    whole = _device(name, True, lc)
    kw = dict(anchor=anchor, strict=True, want=WANT, **BASE)
    w = _handle(name, lc)
    again = w.scenario_returns(actions, **kw)
    chunks = w.scenario_returns(actions, max_eval_farms=3 * R + 1, **kw)
    single = w.scenario_returns(actions, max_eval_farms=R + 1, **kw)
    farms = np.random.default_rng(5).permutation(B)[:13]
    sub = w.scenario_returns(actions[farms], farms=farms, **dict(kw, anchor=anchor[farms]))
    t = w.scenario_returns(torch.from_numpy(actions.copy()).cuda(), **dict(kw, anchor=torch.from_numpy(anchor.copy()).cuda()))
    out = {"score": torch.empty((B, S.K), dtype=torch.float64, device="cuda")}
    t0 = w.scenario_returns(torch.from_numpy(actions.copy()).cuda(), **dict(kw, want="score", out=out))
    dkw = dict(kw, strict=False)
    d1, d2 = w.scenario_returns(actions, **dkw), w.scenario_returns(actions, **dkw)
    timing = w.scenario_timing()
    w.close()
    assert all(v.is_cuda for v in t.values()) and t0["score"] is out["score"] and set(t0) == {"score"}
    assert t["best"].dtype == torch.int32 and t["final_yaw"].dtype == torch.float32 and t["wind_paths"].dtype == torch.float64
    for k in WANT:
        assert np.array_equal(_bits(again[k]), _bits(whole[k])), k
        assert np.array_equal(_bits(chunks[k]), _bits(whole[k])), k
        assert np.array_equal(_bits(single[k]), _bits(whole[k])), k
        assert np.array_equal(_bits(sub[k]), _bits(whole[k][farms])), k
        assert np.array_equal(_bits(t[k].cpu().numpy()), _bits(whole[k])), k
        assert np.array_equal(_bits(d1[k]), _bits(d2[k])), k
    assert np.array_equal(_bits(t0["score"].cpu().numpy()), _bits(whole["score"]))
    assert timing["total_ms"] > 0.0


SHAPES = {  # layout, K, M, H, tail — the row of three under its four winds unless stated
    "pairs300": ("row3", 60, 5, 2, 2),    # 300 (sequence, member) pairs: more than 256 threads
    "rows4096": ("row3", 128, 8, 4, 3),   # the row limit: every sequence holds; R N = 12 288, the reduce kernel's 1024 threads
    "members64": ("row3", 1, 64, 3, 7),
    "steps1": ("row3", 7, 6, 1, 6),
    "steps64": ("row3", 1, 1, 64, 1),     # one sequence under one member
    "wide": ("Turb16_Row5_", 8, 8, 8, 3),  # N = 16, R N = 8192: the threshold of the reduce kernel's 1024 threads, four farms
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_past_one_unit(shape):
    """Strict, N = 3 (N = 16 for the wide slot): the paths' bits, every reward, member return and statistic inside the strict bounds, the statistics of
    the device's own member returns, final_yaw's bits.  At the row limit every sequence holds: best == 0 and equal scores."""
    from wfcrl_env_amd.backend import WfStep

    import yawopt_ref

    layout, Kc, Mc, Hc, tail = SHAPES[shape]
    x, y, ws, wd = yawopt_ref.gpu_input(layout)
    ws, wd = ws[:4], wd[:4]  # (the row's four winds; four farms of a 32-farm input)
    B, N, lc, lam, gamma, seed = len(ws), len(x), 0.1, 0.4, 0.95, 77
    rng = np.random.default_rng(Kc * 1000 + Mc)
    state = {"yaw": rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32), "acc": rng.uniform(0.0, 30.0, (B, N)).astype(np.float32),
             "moves": rng.integers(1, 6, B).astype(np.int32)}
    holds = Kc * Mc * Hc == S.MAX_ROWS
    actions = np.zeros((B, Kc, Hc, N), np.float32) if holds else rng.uniform(-5.0, 5.0, (B, Kc, Hc, N)).astype(np.float32)
    bounds = (6.0, 11.0)
    ref = S.scenario(x, y, ws, wd, state, actions, dict(S.PARAMS, discrete=False), gamma, lc, Mc, S.PROCESS, seed, tail, lam, None, bounds)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    w.env_config(load_coef=lc, dt=S.PARAMS["dt"])
    w.env_reset()
    w.env_set_state(state)
    got = w.scenario_returns(actions, Mc, PROC, seed=seed, gamma=gamma, tail=tail, risk_weight=lam, bounds=bounds, strict=True, want=WANT)
    w.close()
    assert np.array_equal(_bits(got["wind_paths"]), _bits(ref["wind_paths"]))
    assert np.array_equal(_bits(got["final_yaw"]), _bits(ref["final_yaw"]))
    _against_reference(ref, got, lc, parity.TOL_F64, gamma, lam, shape)
    _own_statistics(got, tail, lam, gamma)
    if holds:
        assert (got["best"] == 0).all() and (_bits(got["score"]) == _bits(got["score"][:, :1])).all()
        assert (_bits(got["member_returns"]) == _bits(got["member_returns"][:, :1])).all()


def test_state_and_pending_speed_are_left_alone():
    """env_get_state before and after compare equal.  A speed left by env_set_prev_wind is neither used — the rewards have the
    bits of a run without it (strict) — nor consumed: the next env_step pays the reward of a handle that never ran a scenario."""
    name, lc = "Turb6_Row2_", 0.1
    x, y, ws, wd, state, actions, anchor = S.gpu_case(name)
    kw = dict(anchor=anchor, strict=True, want=("rewards", "score"), **BASE)
    w, plain = _handle(name, lc), _handle(name, lc)
    free = w.scenario_returns(actions, **kw)
    w.env_set_prev_wind(ws * 1.1)
    plain.env_set_prev_wind(ws * 1.1)
    before = w.env_get_state()
    got = w.scenario_returns(actions, **kw)
    after = w.env_get_state()
    a = actions[:, 1, 0].copy()
    paid, want = w.env_step(a, want=("reward",))["reward"], plain.env_step(a, want=("reward",))["reward"]
    unpaid = _handle(name, lc)
    other = unpaid.env_step(a, want=("reward",))["reward"]
    w.close(); plain.close(); unpaid.close()
    for k in before:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], np.asarray(state[k]).reshape(before[k].shape)), k
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(free[k])), k
    assert np.array_equal(_bits(paid), _bits(want)) and (paid != other).all()  # (the pending speed was still there, and counts)


def test_vec_env_method():
    """VecWindFarmEnv.scenario_returns on a wind_process env: process=None takes the env's process and its distribution's
    speed bounds, and agrees with WfStep.scenario_returns on the same state, on a farm list too; the env is left as it was;
    an env without a process refuses with a clear message and serves when given one."""
    import torch
    from wfcrl_env_amd import environments as envs

    B, Kv, Hv, Mv = 6, 3, 2, 4
    dist = dict(ws_lo=5.0, ws_hi=9.0)
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20, wind_process=dict(PROC, dist=dist))
    N = env.num_turbines
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    env.step({"yaw": (torch.rand((B, N), generator=gen) * 10.0 - 5.0).cuda()})
    seqs = (torch.rand((B, Kv, Hv, N), generator=gen) * 10.0 - 5.0).cuda()
    before = env.get_state()
    want = ("expected_returns", "cvar", "score", "best", "wind_paths")
    r = env.scenario_returns({"yaw": seqs}, members=Mv, seed=9, gamma=0.95, tail=2, risk_weight=0.5, want=want)
    assert set(r) == set(want) and all(v.is_cuda for v in r.values())
    assert tuple(r["score"].shape) == (B, Kv) and r["score"].dtype == torch.float64 and r["best"].dtype == torch.int32
    assert tuple(r["wind_paths"].shape) == (B, Mv, Hv, 2)
    direct = env.fi.scenario_returns(seqs, Mv, PROC, seed=9, gamma=0.95, tail=2, risk_weight=0.5, bounds=(5.0, 9.0), want=want)
    for k in r:
        assert torch.equal(r[k], direct[k]), k
    assert float(r["wind_paths"][..., 0].min()) >= 5.0 and float(r["wind_paths"][..., 0].max()) <= 9.0
    assert torch.equal(r["best"].long(), r["score"].argmax(dim=1))
    strict = env.scenario_returns(seqs, members=Mv, seed=9, strict=True)
    sub = env.scenario_returns(seqs, members=Mv, seed=9, farms=[5, 2], strict=True)
    for k in sub:
        assert torch.equal(sub[k], strict[k][[5, 2]]), k
    after = env.get_state()
    assert _same(before, after)
    with pytest.raises(ValueError, match=r"\(num_envs, K, H, num_turbines\)"):
        env.scenario_returns(seqs[:, 0])
    env.close()
    plain = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    plain.reset(seed=0)
    with pytest.raises(ValueError, match="needs a wind process.*built without wind_process"):
        plain.scenario_returns(seqs)
    given = plain.scenario_returns(seqs, members=Mv, process=PROC)  # (a held-wind episode: only the current wind is read)
    assert tuple(given["score"].shape) == (B, Kv) and bool(torch.isfinite(given["score"]).all())
    plain.close()


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    N = 3
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.scenario_returns(np.zeros((2, 2, 2, N), np.float32), 2, PROC)
    w.close()
    w = WfStep(x, y, env_batch=2)
    zero = np.zeros((2, 2, 2, N), np.float32)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.scenario_returns(zero, 2, PROC)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.scenario_returns(zero, 2, PROC)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
        w.scenario_returns(np.zeros((2, 1, 65, N), np.float32), 1, PROC)
    for members in (0, 65, -3):
        with pytest.raises(ValueError, match="WF_E_INVALID.*M must be in 1..64"):
            w.scenario_returns(zero, members, PROC)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K M H <= 4096"):
        w.scenario_returns(np.zeros((2, 4097, 1, N), np.float32), 1, PROC)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K M H <= 4096"):
        w.scenario_returns(np.zeros((2, 241, 1, N), np.float32), 17, PROC)  # 4097 rows
    for tail in (0, 3, -1):
        with pytest.raises(ValueError, match="WF_E_INVALID.*tail must be in 1..M"):
            w.scenario_returns(zero, 2, PROC, tail=tail)
    for v in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.scenario_returns(zero, 2, PROC, gamma=v)
        with pytest.raises(ValueError, match="WF_E_INVALID.*risk_weight"):
            w.scenario_returns(zero, 2, PROC, risk_weight=v)
    for bad in (dict(ws_revert=1.5), dict(wd_revert=-0.1), dict(ws_revert=float("nan"))):
        with pytest.raises(ValueError, match="WF_E_INVALID.*ws_revert and wd_revert must be in"):
            w.scenario_returns(zero, 2, dict(PROC, **bad))
    for bad in (dict(ws_sigma=-1.0), dict(wd_sigma=float("inf")), dict(wd_ramp=-0.5)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*ws_sigma, wd_sigma and wd_ramp"):
            w.scenario_returns(zero, 2, dict(PROC, **bad))
    with pytest.raises(ValueError, match="unknown wind process parameter"):
        w.scenario_returns(zero, 2, dict(PROC, sigma=1.0))
    with pytest.raises(ValueError, match="needs a wind process"):
        w.scenario_returns(zero, 2, None)
    for bounds in ((9.0, 9.0), (10.0, 4.0), (0.0, 9.0), (3.0, float("inf")), (float("nan"), 9.0)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*speed bounds"):
            w.scenario_returns(zero, 2, PROC, bounds=bounds)
    for anchor in ([[8.0, 270.0], [0.0, 270.0]], [[-1.0, 270.0], [8.0, 270.0]], [[8.0, float("nan")], [8.0, 270.0]]):
        with pytest.raises(ValueError, match="WF_E_INVALID.*anchor's speed must be > 0"):
            w.scenario_returns(zero, 2, PROC, anchor=anchor)
    with pytest.raises(ValueError, match=r"anchor must be \(n_farms, 2\)"):
        w.scenario_returns(zero, 2, PROC, anchor=[8.0, 270.0])
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.scenario_returns(zero, 2, PROC, max_eval_farms=7)  # K M H = 8
    with pytest.raises(ValueError, match="farm index out of range"):
        w.scenario_returns(zero, 2, PROC, farms=[0, 2])
    with pytest.raises(ValueError, match=r"\(n_farms, K, H, num_turbines\)"):
        w.scenario_returns(zero[:1], 2, PROC)
    with pytest.raises(ValueError, match=r"\(n_farms, K, H, num_turbines\)"):
        w.scenario_returns(zero[:, :, :, :2], 2, PROC)
    with pytest.raises(ValueError, match="want must name"):
        w.scenario_returns(zero, 2, PROC, want=("returns",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.scenario_timing()
    up = zero.copy()
    up[:, 1] = 5.0
    r = w.scenario_returns(up[:1], 2, PROC, farms=[1], max_eval_farms=8, want=WANT)  # (the handle still serves)
    assert r["score"].shape == (1, 2) and np.isfinite(r["score"]).all() and r["best"].tolist() in ([0], [1])
    assert r["member_returns"].shape == (1, 2, 2) and r["wind_paths"].shape == (1, 2, 2, 2)
    # from the reset state: the first 5 deg pass, and fill the budget (5 / 0.3 / 2 / 60 = 0.14 >= 0.1): the second step is gated
    assert r["final_yaw"][0, 0].tolist() == [0.0] * N and r["final_yaw"][0, 1].tolist() == [5.0] * N
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_kernel_info_shows_no_scratch():
    w = _handle("row3", 0.1, state=False)
    info = w.scenario_kernel_info()
    w.close()
    assert set(info) == {"layout", "reduce"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
