"""GPU: time-series episodes beyond reset / step (include/wfseries.h) — the preview of the series' coming rows against
tests/series_ref.py, the series-ahead mode of lookahead, plan and credit against the same runs given the rows by the caller,
against their NumPy references over the float64 oracle and against what the env then pays, the end of the series, and the
checkpoint of a time-series episode.

The bounds need no measured number: they are the ones tests/test_lookahead_gpu.py, test_plan_gpu.py and test_credit_gpu.py
use — the step's per-turbine contract (tests/parity.py) carried through the reward's formula per row (credit_ref.bound), TOL_F64
for rows solved in float64 (strict), TOL for the env's own default-mode step, plus the rounding of the env's float32 reward.
Bit identity between runs is asserted in strict mode, where every row is solved by the float64 kernel, whose bits do not
depend on the batch.

Inputs (tests/series_cases.py): series(T) — the speed changes every second row, the direction every row —, so a batch holds
farms whose pending speed equals the current one next to farms where it differs; start rows are set through the env's own
set_state, which this file tests as well."""
import numpy as np
import pytest

import credit_ref
import lookahead_ref
import parity
import series_cases
import series_ref
from series_cases import GAMMA, LAYOUTS, LOAD_COEF
from test_credit_gpu import _env_params
from test_lookahead import PARAMS
from test_lookahead_gpu import _bounds

pytestmark = pytest.mark.gpu

WANT = ("returns", "rewards", "farm_power", "final_yaw", "best")
PLAN_WANT = ("plan", "plan_return", "hold_return", "first_action", "final_yaw", "mean")


def _csv(tmp_path, s):
    p = tmp_path / "wind.csv"
    p.write_text("ws,wd\n" + "\n".join(f"{float(a)!r},{float(b)!r}" for a, b in s) + "\n")
    return str(p)


def _env(env_id, B, T, tmp_path, **kw):
    from wfcrl_env_amd import environments as envs

    kw.setdefault("return_torch", False)
    return envs.make(env_id, env_batch=B, max_num_steps=50, wind_time_series=_csv(tmp_path, series_cases.series(T)),
                     load_coef=LOAD_COEF, **kw)


def _restart(env, start):
    """The env's state with start rows of the test's choice (the env's own draw them from the reset seed)."""
    state = env.get_state()
    state["series_start"] = np.asarray(start, np.int32)
    env.set_state(state)


def _handle(name, B, T, start, **config):
    """A WfStep in the state VecWindFarmEnv.reset leaves: series set, env state zeroed, one tick, the warm-up solve."""
    from wfcrl_env_amd.backend import WfStep

    x, y = series_cases.layout(name)
    w = WfStep(x, y, env_batch=B)
    w.env_config(load_coef=LOAD_COEF, **config)
    w.set_wind_series(series_cases.series(T), start=np.asarray(start, np.int32))
    w.env_reset()
    w.wind_series_step()
    w.env_step(None, want=("yaw",))
    return w


def _tick_and_step(w, rng):
    w.wind_series_step()
    a = rng.uniform(-5.0, 5.0, (w.env_batch, w.num_turbines)).astype(np.float32)
    return w.env_step(a, want=("reward",))["reward"]


# ---- 1. the preview ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_preview_has_the_bits_of_the_reference(name):
    """T = 7, 300 farms (the second thread block takes 44 of them), start rows that include T - 1, so the modulo wraps: the
    window equals tests/series_ref.py's at t = 0, 3 and T - 1, for H = 1, 3, 5 and first = 0, 1, with a farm list from both
    blocks, NumPy and torch, with the right `available`; the window (0, 1) is get_wind()."""
    import torch
    from wfcrl_env_amd.backend import WfStep

    T, B = 7, 300
    s = series_cases.series(T)
    start = np.random.default_rng(7).integers(0, T, B).astype(np.int32)
    start[[0, 1, 2, 255, 256, 299]] = [T - 1, 0, T - 1, 3, T - 1, T - 1]
    x, y = series_cases.layout(name)
    w = WfStep(x, y, env_batch=B)
    w.set_wind_series(s, start=start)
    farms = [299, 0, 256]
    seen = {}
    for t in range(T):
        if t:
            w.wind_series_step()
        if t not in (0, 3, T - 1):
            continue
        cur = w.series_state()
        assert (cur["T"], cur["t"], cur["prev_pending"]) == (T, t, t > 0) and np.array_equal(cur["start"], start)
        for H in (1, 3, 5):
            for first in (0, 1):
                want, avail = series_ref.window(s, start, t, first, H)
                got, a = w.wind_preview(H, first=first)
                assert got.shape == (B, H, 2) and got.dtype == np.float64 and a == avail, (t, H, first)
                assert np.array_equal(got, want), (t, H, first)
                sub, a = w.wind_preview(H, first=first, farms=farms)
                assert a == avail and np.array_equal(sub, want[farms]), (t, H, first)
                dev, a = w.wind_preview(H, first=first, as_torch=True)
                assert dev.is_cuda and dev.dtype == torch.float64 and a == avail and np.array_equal(dev.cpu().numpy(), want)
                out = torch.full((3, H, 2), -1.0, dtype=torch.float64, device="cuda")
                dsub, a = w.wind_preview(H, first=first, farms=farms, out=out)
                assert dsub is out and np.array_equal(out.cpu().numpy(), want[farms])
                seen[(t, H, first)] = avail
        ws, wd = w.get_wind()
        now = w.wind_preview(1, first=0)[0]
        assert np.array_equal(now[:, 0, 0], ws) and np.array_equal(now[:, 0, 1], wd)
    assert seen[(0, 5, 1)] == 5 and seen[(3, 5, 1)] == 3 and seen[(T - 1, 3, 1)] == 0 and seen[(T - 1, 3, 0)] == 1
    last = series_ref.window(s, start, T - 1, 0, 1)[0]
    assert np.array_equal(w.wind_preview(5)[0], np.repeat(last, 5, axis=1))  # (nothing is left: the last wind held)
    # refusals: nothing is launched, the handle still serves
    for kw in (dict(H=0), dict(H=65), dict(H=2, first=-1), dict(H=2, farms=[0, B]), dict(H=2, farms=[-1])):
        with pytest.raises(ValueError, match="WF_E_INVALID"):
            w.wind_preview(**kw)
    info = w.series_kernel_info()
    assert set(info) == {"window"} and info["window"]["vgprs"] > 0 and info["window"]["scratch_bytes"] == 0
    w.set_wind(8.0, 270.0)  # not in series mode any more
    for call in (lambda: w.wind_preview(2), w.series_state, lambda: w.series_seek(0)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*not in series mode"):
            call()
    assert w.step(np.zeros((B, len(x)), np.float32))["power"].shape == (B, len(x))
    w.close()


def test_env_preview_is_what_the_env_then_observes(tmp_path):
    """VecWindFarmEnv.wind_preview(H) on a torch env: a CUDA tensor whose entry h is the free wind the env observes after
    step h + 1; an env without a series refuses."""
    import torch
    from wfcrl_env_amd import environments as envs

    B, T, H = 6, 9, 4
    env = _env("Turb6_Row2_Floris", B, T, tmp_path, return_torch=True)
    env.reset(seed=5)
    env.step({"yaw": torch.zeros((B, 6), device="cuda")})
    p, avail = env.wind_preview(H)
    assert p.is_cuda and p.dtype == torch.float64 and tuple(p.shape) == (B, H, 2) and avail == H
    for h in range(H):
        obs = env.step({"yaw": torch.zeros((B, 6), device="cuda")})[0]
        assert torch.equal(obs["freewind_measurements"], p[:, h]), h
    assert env.wind_preview(H)[1] == T - 1 - env.fi.series_state()["t"] == 2
    env.close()
    env = envs.make("Turb6_Row2_Floris", env_batch=2, max_num_steps=5, return_torch=False)
    env.reset(seed=0)
    with pytest.raises(ValueError, match="time-series episode"):
        env.wind_preview(2)
    for call in (lambda: env.lookahead_returns(np.zeros((2, 1, 1, 6), np.float32), wind="series"),
                 lambda: env.counterfactual_rewards(np.zeros((2, 6), np.float32), wind="series"),
                 lambda: env.plan_actions(2, candidates=3, elites=1, wind="series")):
        with pytest.raises(ValueError, match="needs a time-series episode"):
            call()
    env.close()


# ---- 2. lookahead --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_lookahead_under_the_coming_rows(name, tmp_path):
    """B = 5, K = 3, H = 3, T = 12, strict; right after reset (t = 1: the speed of tick 0 is still pending, the warm-up solve
    did not consume it) and again after two steps (nothing pending).  wind="series"
      - has the bits of wind=<the rows of tests/series_ref.py> in every output that does not see the pending speed
        (farm_power, final_yaw, rewards of h >= 1) on every farm, and in ALL outputs on the farms whose pending speed equals
        the current one — after two steps: on every farm; where the two speeds differ, step 0's rewards differ;
      - is inside the bounds of lookahead_ref.lookahead(wind=rows, wr0=current speed) in rewards, farm power and returns;
      - rewards[:, 0, :] is what the env then pays along sequence 0 (state taken before, put back after), within the row's
        strict bound plus the env step's default-mode bound plus the rounding of its float32 reward;
      - a farm per chunk (max_eval_farms = K H) and a farm list give the bits of the whole run."""
    B, K, H, T = 5, 3, 3, 12
    s = series_cases.series(T)
    x, y = series_cases.layout(name)
    N = len(x)
    env = _env(name + "Floris", B, T, tmp_path)
    env.reset(seed=1)
    _restart(env, [0, 1, 4, 11, 7])  # pending speed == current speed on farms 0 and 2 (even start rows at t = 1)
    params = _env_params(env)
    rng = np.random.default_rng(23)
    kw = dict(gamma=GAMMA, strict=True, want=WANT)
    for phase in ("after reset", "after two steps"):
        if phase == "after two steps":
            for _ in range(2):
                env.step({"yaw": rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)})
        cur = env.fi.series_state()
        t, start = cur["t"], cur["start"]
        assert t == (1 if phase == "after reset" else 3) and cur["prev_pending"] == (phase == "after reset")
        rows, avail = series_ref.window(s, start, t, 1, H)
        assert avail == H
        ws, wd = env.fi.get_wind()
        assert np.array_equal(np.stack([ws, wd], axis=1), series_ref.window(s, start, t, 0, 1)[0][:, 0])
        state = env.fi.env_get_state()
        act = rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
        got = env.fi.lookahead_returns(act, wind="series", **kw)
        by_rows = env.fi.lookahead_returns(act, wind=rows, **kw)
        pending = series_ref.window(s, start, t - 1, 0, 1)[0][:, 0, 0]
        same = (pending == ws) if cur["prev_pending"] else np.ones(B, bool)
        for k in ("farm_power", "final_yaw"):
            assert np.array_equal(got[k], by_rows[k]), (phase, k)
        assert np.array_equal(got["rewards"][:, :, 1:], by_rows["rewards"][:, :, 1:]), phase
        for k in WANT:
            assert np.array_equal(got[k][same], by_rows[k][same]), (phase, k)
        if phase == "after reset":
            assert same.tolist() == [True, False, True, False, False]
            assert (got["rewards"][~same][:, :, 0] != by_rows["rewards"][~same][:, :, 0]).all()
        else:
            assert same.all()
        ref = lookahead_ref.lookahead(x, y, ws, wd, state, act, params, GAMMA, LOAD_COEF, wind=rows, wr0=ws)
        b, pb, rb = _bounds(ref, LOAD_COEF, parity.TOL_F64)
        er, ep, et = (np.abs(got[k] - ref[k]) for k in ("rewards", "farm_power", "returns"))
        print(f"{name} {phase}: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}, "
              f"return {(et / rb).max():.3f}")
        assert (er <= b).all() and (ep <= pb).all() and (et <= rb).all(), phase
        assert np.array_equal(got["final_yaw"].view(np.uint32), ref["final_yaw"].view(np.uint32))
        # the env's method, a farm per chunk, a farm list
        via_env = env.lookahead_returns({"yaw": act}, gamma=GAMMA, strict=True, wind="series")
        single = env.fi.lookahead_returns(act, wind="series", max_eval_farms=K * H, **kw)
        farms = [3, 0, 4]
        sub = env.fi.lookahead_returns(act[farms], wind="series", farms=farms, max_eval_farms=K * H, **kw)
        for k in WANT:
            assert np.array_equal(single[k], got[k]), (phase, k)
            assert np.array_equal(sub[k], got[k][farms]), (phase, k)
            assert k == "farm_power" or np.array_equal(via_env[k], got[k]), (phase, k)
        # the truth: what the env pays along sequence 0
        saved = env.get_state()
        paid = np.stack([env.step({"yaw": act[:, 0, h].copy()})[1] for h in range(H)], axis=1).astype(np.float64)
        end = env.fi.env_get_state()
        env.set_state(saved)
        back = env.get_state()
        for k in saved:
            assert (saved[k] is None and back[k] is None) or np.array_equal(np.asarray(saved[k]), np.asarray(back[k])), (phase, k)
        assert np.array_equal(got["final_yaw"][:, 0].view(np.uint32), end["yaw"].view(np.uint32))
        b32 = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, parity.TOL).reshape(B, K, H)
        err = np.abs(got["rewards"][:, 0] - paid)
        allow = b[:, 0] + b32[:, 0] + np.abs(paid) * 2.0 ** -23
        print(f"{name} {phase}: largest |look-ahead reward - env reward| / allowed: {(err / allow).max():.3f}")
        assert (err <= allow).all(), phase
    # the default call still refuses, a caller's wind next to the mode is refused by name
    with pytest.raises(NotImplementedError, match="time-series"):
        env.lookahead_returns({"yaw": act})
    with pytest.raises(ValueError, match='None or "series"'):
        env.lookahead_returns({"yaw": act}, wind=rows)
    env.close()


# ---- 3. plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_plan_under_the_coming_rows(name):
    """The planner case of tests/series_cases.py (8 farms, every one safe under the reference's margin: asserted here and, with
    the reference alone, in tests/test_series.py; the cap is 0 skipped farms).  Right after the reset's tick, with the speed of
    tick 0 pending: plan_actions(wind="series") has the BITS of plan_ref.plan(wind=rows, wr0=current speed) in plan, mean,
    first_action and final_yaw, and its returns are inside their bounds.  After a step: the bits of plan_actions(wind=rows)
    in every output, also for a farm list run a farm per chunk."""
    c, ref = series_cases.plan_case(name), series_cases.plan_reference(name)
    B, H, K = c["farms"], c["H"], c["K"]
    w = _handle(name, B, c["T"], c["start"], dt=PARAMS["dt"])
    w.env_set_state(c["state"])
    cur = w.series_state()
    assert cur["t"] == c["t"] == 1 and cur["prev_pending"]
    kw = dict(candidates=K, elites=c["E"], sigma=c["sigma"], seed=c["seed"], gamma=GAMMA, strict=True, want=PLAN_WANT)
    got = w.plan_actions(H, wind="series", **kw)
    assert ref["safe"].all()
    for k in ("plan", "mean", "first_action", "final_yaw"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    eh, ep = np.abs(got["hold_return"] - ref["hold_return"]), np.abs(got["plan_return"] - ref["plan_return"])
    print(f"{name}: largest error / bound: hold_return {(eh / ref['hold_bound']).max():.3f}, plan_return {(ep / ref['plan_bound']).max():.3f}")
    assert (eh <= ref["hold_bound"]).all() and (ep <= ref["plan_bound"]).all()
    assert (got["plan"] != 0.0).any() and (got["plan_return"] > got["hold_return"]).any()  # (the search moved)
    rng = np.random.default_rng(3)
    _tick_and_step(w, rng)
    cur = w.series_state()
    assert cur["t"] == 2 and not cur["prev_pending"]
    rows, avail = series_ref.window(c["series"], c["start"], 2, 1, H)
    assert avail == H
    ahead = w.plan_actions(H, wind="series", **kw)
    by_rows = w.plan_actions(H, wind=rows, **kw)
    farms = [5, 2, 7]
    sub = w.plan_actions(H, wind="series", farms=farms, max_eval_farms=K * H, **kw)
    held = w.plan_actions(H, **kw)
    for k in PLAN_WANT:
        assert np.array_equal(ahead[k], by_rows[k]), k
        assert np.array_equal(sub[k], ahead[k][farms]), k
    assert (held["plan_return"] != ahead["plan_return"]).all()  # (the mode is off again: the current wind held)
    w.close()


# ---- 4. credit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_credit_under_the_coming_row(name, tmp_path):
    """counterfactual_rewards(a, wind="series") BEFORE step(a), right after reset (a stale pending speed) and after two steps:
    every row within the reference's bounds (the transition restated in credit_ref, the oracle under the series' coming row,
    normalised by the current speed; default mode: TOL), and the reward step(a) then pays within the base row's bound of
    reward_base, as tests/test_credit_gpu.py holds it.  The default call on the same env still raises."""
    B, T = 5, 12
    s = series_cases.series(T)
    x, y = series_cases.layout(name)
    N = len(x)
    env = _env(name + "Floris", B, T, tmp_path)
    env.reset(seed=2)
    _restart(env, [0, 1, 4, 11, 7])
    params = _env_params(env)
    rng = np.random.default_rng(31)
    for phase in ("after reset", "after two steps"):
        if phase == "after two steps":
            env.step({"yaw": rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)})
        cur = env.fi.series_state()
        nxt = series_ref.window(s, cur["start"], cur["t"], 1, 1)[0][:, 0]
        ws = env.fi.get_wind()[0]
        st = env.fi.env_get_state()
        a = rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)
        base_yaw = credit_ref.transition(st["yaw"], st["acc"], st["moves"], a, params)
        alt_yaw = credit_ref.transition(st["yaw"], st["acc"], st["moves"], np.zeros((B, N, 1), np.float32), params)
        ref = credit_ref.counterfactual(x, y, nxt[:, 0], nxt[:, 1], base_yaw, alt_yaw, LOAD_COEF, wr=ws)
        b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, parity.TOL).reshape(B, 1 + N)
        with pytest.raises(NotImplementedError, match="time-series"):
            env.counterfactual_rewards(a)
        cf = env.counterfactual_rewards(a, wind="series")
        assert cf["reward_base"].shape == (B,) and cf["reward_alt"].shape == (B, N, 1) and cf["difference"].shape == (B, N, 1)
        e0 = np.abs(cf["reward_base"] - ref["reward"][:, 0])
        ea = np.abs(cf["reward_alt"][:, :, 0] - ref["reward"][:, 1:])
        sub = env.counterfactual_rewards(a, wind="series", farms=[4, 1], strict=True)
        whole = env.counterfactual_rewards(a, wind="series", strict=True)
        for k in sub:
            assert np.array_equal(sub[k], whole[k][[4, 1]]), (phase, k)
        reward = env.step({"yaw": a.copy()})[1].astype(np.float64)
        ep = np.abs(reward - cf["reward_base"])
        print(f"{name} {phase}: largest error / bound: base {(e0 / b[:, 0]).max():.3f}, alternatives {(ea / b[:, 1:]).max():.3f}, "
              f"step reward - reward_base {(ep / b[:, 0]).max():.3f}")
        assert (e0 <= b[:, 0]).all() and (ea <= b[:, 1:]).all(), phase
        assert (ep <= b[:, 0]).all(), phase
        held = env.fi.get_wind()  # (after the step the env holds the row the counterfactual was solved under)
        assert np.array_equal(held[0], nxt[:, 0]) and np.array_equal(held[1], nxt[:, 1])
    env.close()


# ---- 5. the end of the series --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_end_of_the_series(name):
    """T = 7.  At t = T - 3 with H = 5 the three runs run: two entries are real, rows 2 .. 4 hold the last wind — the bits of the
    same runs given those rows.  At t = T - 1 the coming step does not exist: the three runs fail with "exhausted", as the tick
    does, and the handle still serves."""
    T, B, K, H = 7, 4, 3, 5
    s = series_cases.series(T)
    start = np.int32([0, 6, 3, 5])
    w = _handle(name, B, T, start)
    N = w.num_turbines
    rng = np.random.default_rng(11)
    while w.series_state()["t"] < T - 3:
        _tick_and_step(w, rng)
    rows, avail = w.wind_preview(H)
    assert avail == 2 and np.array_equal(rows, series_ref.window(s, start, T - 3, 1, H)[0])
    assert np.array_equal(rows[:, 2:], np.repeat(rows[:, 1:2], 3, axis=1)) and (rows[:, 0] != rows[:, 1]).any()
    act = rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
    kw = dict(gamma=GAMMA, strict=True, want=WANT)
    la, la_rows = w.lookahead_returns(act, wind="series", **kw), w.lookahead_returns(act, wind=rows, **kw)
    pkw = dict(candidates=4, elites=2, seed=1, gamma=GAMMA, strict=True, want=PLAN_WANT)
    pl, pl_rows = w.plan_actions(H, wind="series", **pkw), w.plan_actions(H, wind=rows, **pkw)
    for k in WANT:
        assert np.array_equal(la[k], la_rows[k]), k
    for k in PLAN_WANT:
        assert np.array_equal(pl[k], pl_rows[k]), k
    cf = w.counterfactual_rewards(act[:, 0, 0], base_kind="action", alt_kind="action", wind="series", strict=True)
    one = w.lookahead_returns(act[:, :1, :1], wind="series", strict=True, want=("rewards",))
    assert np.isfinite(cf["reward"]).all() and np.allclose(cf["reward"][:, 0], one["rewards"][:, 0, 0], rtol=1e-12, atol=0.0)
    while w.series_state()["t"] < T - 1:
        _tick_and_step(w, rng)
    assert w.wind_preview(H)[1] == 0
    for call in (lambda: w.lookahead_returns(act, wind="series", **kw), lambda: w.plan_actions(H, wind="series", **pkw),
                 lambda: w.counterfactual_rewards(act[:, 0, 0], base_kind="action", alt_kind="action", wind="series"),
                 w.wind_series_step):
        with pytest.raises(ValueError, match="exhausted"):
            call()
    # the C boundary: a caller's wind next to the mode is refused (the Python keyword cannot express it)
    raw = w._lookahead()
    raw._call("set_series", 1)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind of your own"):
        raw._call("run", act.ctypes.data, K, H, rows.ctypes.data, GAMMA, B, None, None, None, None, None, None, 0)
    held = w.lookahead_returns(act, **kw)  # (the handle still serves; the mode is off again: the wind it holds, held)
    last = np.repeat(w.wind_preview(1, first=0)[0], H, axis=1)
    by_rows = w.lookahead_returns(act, wind=last, **kw)
    for k in WANT:
        assert np.isfinite(held[k]).all() and np.array_equal(held[k], by_rows[k]), k
    assert w.step(np.zeros((B, N), np.float32))["power"].shape == (B, N)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*parent in series mode"):
        w.lookahead_returns(act, wind="series", **kw)
    w.close()


# ---- 6. the checkpoint ---------------------------------------------------------------------------------------------------
def _run(env, acts):
    out = []
    for a in acts:
        obs, r, term, trunc, info = env.step({"yaw": a})
        out.append(({k: np.array(v) for k, v in obs.items()}, np.array(r), np.array(trunc), {k: np.array(v) for k, v in info.items()}))
    return out


def _same_runs(a, b, what):
    assert len(a) == len(b)
    for i, ((o1, r1, t1, i1), (o2, r2, t2, i2)) in enumerate(zip(a, b)):
        for k in o1:
            assert np.array_equal(o1[k], o2[k]), (what, i, k)
        assert np.array_equal(r1, r2) and np.array_equal(t1, t2), (what, i)
        for k in i1:
            assert np.array_equal(i1[k], i2[k]), (what, i, k)


@pytest.mark.parametrize("env_id,B,groups", [("HornsRev1_Floris", 700, 8), ("Turb6_Row2_Floris", 6, 0), ("Turb3_Row1_Floris", 6, 0)])
def test_checkpoint_of_a_series_episode(env_id, B, groups, tmp_path):
    """T = 8: the state right after reset (t = 1, a speed pending) and after 3 steps; 3 more steps, which reach the series'
    last row.  set_state on the same env and on a fresh one, then the same steps again: observations, rewards, truncation
    and info have the same bits, and the step after them fails with "exhausted" as it did.  Once on the grouped path
    (HornsRev1 x 700, sized as tests/test_hip_parity.py sizes it: one geometry and pair table per series row, the groups
    turned by the tick) and on the path with a geometry per farm (direction_groups == 0) — the value is asserted."""
    T = 8
    env = _env(env_id, B, T, tmp_path)
    N = env.num_turbines
    acts = np.random.default_rng(6).uniform(-5.0, 5.0, (6, B, N)).astype(np.float32)
    obs0 = env.reset(seed=4)
    assert env.fi.kernel_info()["direction_groups"] == groups
    at_reset = env.get_state()
    assert at_reset["series_t"] == 1 and at_reset["series_prev_pending"] is True and at_reset["series_start"].shape == (B,)
    assert len(set(at_reset["series_start"].tolist())) > 1
    run1 = _run(env, acts[:3])
    after3 = env.get_state()
    assert after3["series_t"] == 4 and after3["series_prev_pending"] is False and after3["num_iter"] == at_reset["num_iter"] + 3
    run2 = _run(env, acts[3:])
    assert env.fi.series_state()["t"] == T - 1
    with pytest.raises(ValueError, match="exhausted"):
        env.step({"yaw": acts[0]})
    for k in ("wind_speed", "wind_direction"):  # (the run moved through different winds: the cursor matters)
        assert (run1[0][0][k] != run2[2][0][k]).any()

    def replay(e, what):
        e.set_state(after3)
        assert e.fi.kernel_info()["direction_groups"] == groups
        assert np.array_equal(e.get_state()["wind_direction"], after3["wind_direction"])
        _same_runs(_run(e, acts[3:]), run2, what + ", from step 3")
        with pytest.raises(ValueError, match="exhausted"):
            e.step({"yaw": acts[0]})
        e.set_state(at_reset)
        back = e.get_state()
        for k in at_reset:
            assert (at_reset[k] is None and back[k] is None) or np.array_equal(np.asarray(at_reset[k]), np.asarray(back[k])), (what, k)
        _same_runs(_run(e, acts[:3]), run1, what + ", from reset")
        _same_runs(_run(e, acts[3:]), run2, what + ", from reset on")
        with pytest.raises(ValueError, match="exhausted"):
            e.step({"yaw": acts[0]})

    replay(env, "the same env")
    fresh = _env(env_id, B, T, tmp_path)
    replay(fresh, "a fresh env")
    # a series state on an env without a series, and the reverse
    from wfcrl_env_amd import environments as envs

    plain = envs.make(env_id, env_batch=B, max_num_steps=50, return_torch=False)
    plain.reset(seed=0)
    with pytest.raises(ValueError, match="time-series episode"):
        plain.set_state(at_reset)
    with pytest.raises(ValueError, match="no series cursor"):
        fresh.set_state(plain.get_state())
    with pytest.raises(ValueError, match="WF_E_INVALID"):
        fresh.fi.series_seek(T, False)
    with pytest.raises(ValueError, match="WF_E_INVALID.*tick 0"):
        fresh.fi.series_seek(0, True)
    assert obs0["yaw"].shape == (B, N)
    env.close(); fresh.close(); plain.close()
