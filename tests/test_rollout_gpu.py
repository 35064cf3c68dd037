"""GPU: closed-loop rollouts of yaw-table controllers on the device (include/wfrollout.h) against tests/rollout_ref.py — the
same filters, look-ups, trajectories, rows, rewards and returns in NumPy over the float64 oracle.

BITS.  actions, final_yaw, gated and filter_final do not see the solver: they have the reference's bits on every case, in
every mode, with no tolerance and no exempted farm.
BOUNDS need no measured number.  The step's contract is per turbine (tests/parity.py), carried through the reward's formula
by credit_ref.bound / power_bound per ROW — TOL_F64 when every row is solved in float64 (strict), TOL in the handle's default
mode; a return is held to sum_h g_h bound_h, on EVERY entry.  The measured fraction of the bound is printed.
BEST equals the reference's in both modes: tests/test_rollout.py asserts, on the reference alone, that on every farm of every
case the controllers' returns are pairwise further apart than the sum of their two default-mode bounds.

Cases (tests/rollout_ref.py, the smallest shapes at which the kernels can go wrong): the row of three with K = 5, H = 7 in
both encodings; Ablaincourt_ (N = 7, five farms: farm lists, ragged chunks, winds around north); HornsRev1_ (N = 80, K = 4,
H = 70: 320 trajectories per block of 256 threads, 280 rows past one LDS tile, H past lookahead's 64); a series that ends
inside the horizon.  Bit identity across chunk sizes and farm lists is asserted in STRICT mode, where every row is solved by the
float64 kernel, whose bits do not depend on the batch (tests/test_lookahead_gpu.py); the trajectory outputs in every mode."""
import functools

import numpy as np
import pytest

import credit_ref
import parity
import rollout_ref as rr
from rollout_ref import LOAD_COEF
from test_credit_gpu import _env_params

pytestmark = pytest.mark.gpu

NAMES = ("row3", "row3_discrete", "Ablaincourt_", "HornsRev1_")
WANT = ("returns", "rewards", "farm_power", "actions", "final_yaw", "gated", "filter_final", "best")
TRAJECTORY = ("actions", "final_yaw", "gated", "filter_final")
LA_WANT = ("returns", "rewards", "farm_power", "final_yaw", "best")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _set_tables(w, tables):
    for slot, (T, twd, tws, interp) in tables.items():
        w.set_yaw_table(T, twd, tws, interp=interp, slot=slot)


def _handle(c, state=True, tables=True):
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.set_wind(c["ws"], c["wd"])
    w.env_config(load_coef=LOAD_COEF, discrete=c["env"]["discrete"])
    if state:
        w.env_reset()
        w.env_set_state(c["state"])
    if tables:
        _set_tables(w, c["tables"])
    return w


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    c = rr.case(name)
    w = _handle(c)
    r = w.controller_returns(c["controllers"], c["H"], gamma=c["gamma"], wind=c["wind"], strict=strict, want=WANT)
    w.close()
    return _freeze(r)


def _assert_trajectory_bits(got, ref, label):
    assert got["actions"].dtype == np.float32 and got["final_yaw"].dtype == np.float32 and got["gated"].dtype == np.int32
    assert got["filter_final"].dtype == np.float64
    assert _same(got["actions"], ref["actions"]), label
    assert _same(got["final_yaw"], ref["final_yaw"]), label
    assert np.array_equal(got["gated"], ref["gated_count"]), label
    assert _same(got["filter_final"], ref["filter_final"]), label


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_has_the_bits_of_the_reference(name):
    """actions, final_yaw, gated and filter_final: the reference's bits, in strict and in default mode — the filter's
    float64 recurrence, the look-up, the deadband, the gate, the accumulator and the counter are visible here without any
    tolerance."""
    ref = rr.reference(name)
    for strict in (True, False):
        _assert_trajectory_bits(_device(name, strict), ref, (name, strict))
    assert ref["gated_count"].sum() > 0


def _check(name, strict, tol):
    c, ref, got = rr.case(name), rr.reference(name), _device(name, strict)
    B, K, H, N = c["B"], c["K"], c["H"], c["N"]
    assert got["returns"].shape == (B, K) and got["returns"].dtype == np.float64
    assert got["rewards"].shape == (B, K, H) and got["rewards"].dtype == np.float64
    assert got["farm_power"].shape == (B, K, H) and got["farm_power"].dtype == np.float64
    assert got["actions"].shape == (B, K, H, N) and got["final_yaw"].shape == (B, K, N)
    assert got["gated"].shape == (B, K) and got["filter_final"].shape == (B, K, 2)
    assert got["best"].shape == (B,) and got["best"].dtype == np.int32
    b, pb, rb = rr.bounds(ref, LOAD_COEF, tol, c["gamma"])
    er, ep, et = (np.abs(got[k] - ref[k]) for k in ("rewards", "farm_power", "returns"))
    print(f"{name} {'strict' if strict else 'default mode'}: largest error / bound: reward {(er / b).max():.3f}, farm power "
          f"{(ep / pb).max():.3f}, return {(et / rb).max():.3f}")
    assert (er <= b).all(), (name, (er / b).max())
    assert (ep <= pb).all(), (name, (ep / pb).max())
    assert (et <= rb).all(), (name, (et / rb).max())
    # the return is the discounted sum of the device's OWN rewards, bit for bit; best is the argmax of its own returns
    import lookahead_ref

    assert np.array_equal(got["returns"], lookahead_ref.discounted(got["rewards"], c["gamma"]))
    assert np.array_equal(got["best"], np.argmax(got["returns"], axis=1))
    # ... and the reference's: the returns are further apart than their bounds (tests/test_rollout.py), so is their order
    assert np.array_equal(got["best"], ref["best"]), name
    assert np.array_equal(np.argsort(-got["returns"], axis=1, kind="stable"), np.argsort(-ref["returns"], axis=1, kind="stable")), name


@pytest.mark.parametrize("name", NAMES)
def test_strict_against_the_reference(name):
    """Every row solved in float64: every row's reward and farm power and every return inside the bounds that follow from
    TOL_F64; `best` and the order of the returns are the reference's.  Nothing is exempted."""
    _check(name, True, parity.TOL_F64)


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_against_the_reference(name):
    """The handle's own resolve mode: the same from TOL."""
    _check(name, False, parity.TOL)


@pytest.mark.parametrize("name", ["row3", "row3_discrete", "Ablaincourt_"])
@pytest.mark.parametrize("strict", [True, False])
def test_lookahead_of_the_actions_gives_the_same_bits(name, strict):
    """Oracle-free, H <= 64: lookahead_returns fed with the rollout's `actions` under the same winds, in the same mode, returns
    the same bits of rewards, returns, final_yaw (and farm_power, best): the rollout is the look-ahead of what the controller
    issues, row for row."""
    c = rr.case(name)
    w = _handle(c)
    got = w.controller_returns(c["controllers"], c["H"], gamma=c["gamma"], wind=c["wind"], strict=strict, want=WANT)
    la = w.lookahead_returns(got["actions"], gamma=c["gamma"], wind=c["wind"], strict=strict, want=LA_WANT)
    w.close()
    for k in LA_WANT:
        assert _same(got[k], la[k]), (name, strict, k)


def _make_env(env_id, B, tmp_path=None, series=None, **kw):
    from wfcrl_env_amd import environments as envs

    kw.setdefault("return_torch", False)
    if series is not None:
        p = tmp_path / "wind.csv"
        p.write_text("ws,wd\n" + "\n".join(f"{float(a)!r},{float(b)!r}" for a, b in series) + "\n")
        kw["wind_time_series"] = str(p)
    return envs.make(env_id, env_batch=B, max_num_steps=50, load_coef=LOAD_COEF, **kw)


def _state_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _replay(env, got, k, H):
    """(rewards (B, H), yaw state after the last step) of stepping the env with controller k's actions; the env is put back."""
    saved = env.get_state()
    paid = np.stack([env.step({"yaw": got["actions"][:, k, h].copy()})[1] for h in range(H)], axis=1).astype(np.float64)
    end = env.fi.env_get_state()
    env.set_state(saved)
    _state_equal(saved, env.get_state())
    return paid, end


@pytest.mark.parametrize("series", [False, True])
def test_against_the_env_itself(series, tmp_path):
    """VecWindFarmEnv.controller_returns BEFORE step, on an env after two random steps — a plain episode (the wind is held)
    and a time-series episode (wind="series").  The call leaves the env as it was: env state, wind, series cursor and the rose
    tables (lut_target_yaw before and after), bit for bit.  Replaying controller k's actions[:, k, h] through env.step: the
    yaw state after H steps has final_yaw's bits for every k; the rewards the env pays are within the sum of the two step
    tolerances (the row's and the env step's, credit_ref.bound under TOL, plus the rounding of the env's float32 reward) of
    `rewards`.  For alpha 1, deadband 0, lead 0 a second walk that asks `lut_action()` at every step ends on the same yaw
    bits: the rollout of the untuned controller IS what stepping with lut_action does."""
    import series_cases

    B, H, T = 4, 5, 12
    s = series_cases.series(T) if series else None
    env = _make_env("Turb3_Row1_Floris", B, tmp_path, s)
    N = env.num_turbines
    x, y = series_cases.layout("Turb3_Row1_")
    env.reset(seed=3)
    near, tws = np.arange(240.0, 300.1, 2.5), np.array([6.0, 8.0, 10.0, 12.0])
    tables = {0: (rr.steering_table(x, near, tws, 270.0, 20.0, 1), near, tws, "nearest"),
              1: (rr.steering_table(x, near, tws, 270.0, 20.0, 2), near, tws, "linear")}
    _set_tables(env.fi, tables)
    rng = np.random.default_rng(5)
    for _ in range(2):
        env.step({"yaw": rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)})
    ctl = dict(alpha=[1.0, 0.5, 1.0], deadband=[0.0, 1.5, 3.0], lead=[0, 0, 1], slot=[0, 1, 1])
    K = 3
    params = _env_params(env)
    wind_kw = "series" if series else None
    before, target_before = env.get_state(), env.lut_target_yaw(1).copy()
    cursor = env.fi.series_state() if series else None
    got = env.controller_returns(ctl, H, gamma=0.9, wind=wind_kw, want=WANT)
    _state_equal(before, env.get_state())
    assert np.array_equal(target_before, env.lut_target_yaw(1))
    if series:
        after = env.fi.series_state()
        assert (cursor["T"], cursor["t"], cursor["prev_pending"]) == (after["T"], after["t"], after["prev_pending"])
        assert np.array_equal(cursor["start"], after["start"]) and not cursor["prev_pending"]
    # the reference under the env's own parameters, state and winds
    ws, wd = env.fi.get_wind()
    state = env.fi.env_get_state()
    rows = None
    if series:
        import series_ref

        rows, avail = series_ref.window(s, cursor["start"], cursor["t"], 1, H)
        assert avail == H
    ref = rr.rollout(x, y, ws, wd, state, ctl, tables, H, params, 0.9, LOAD_COEF, wind=rows, wr0=ws)
    _assert_trajectory_bits(got, ref, series)
    b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, parity.TOL).reshape(B, K, H)
    assert (np.abs(got["rewards"] - ref["rewards"]) <= b).all()
    assert (got["actions"] != 0.0).any() and got["gated"].sum() > 0
    for k in range(K):
        paid, end = _replay(env, got, k, H)
        assert _same(end["yaw"], got["final_yaw"][:, k]), k
        err = np.abs(got["rewards"][:, k] - paid)
        allow = 2.0 * b[:, k] + np.abs(paid) * 2.0 ** -23
        print(f"series={series} controller {k}: largest |rollout reward - env reward| / allowed: {(err / allow).max():.3f}")
        assert (err <= allow).all(), k
    saved = env.get_state()
    for h in range(H):
        a = env.lut_action(0)
        assert _same(a["yaw"], got["actions"][:, 0, h]), h  # what the untuned controller issues, step by step
        env.step(a)
    assert _same(env.fi.env_get_state()["yaw"], got["final_yaw"][:, 0])
    env.set_state(saved)
    # the refusals of plan_actions
    if series:
        with pytest.raises(NotImplementedError, match="time-series"):
            env.controller_returns(ctl, H)
        by_rows = env.controller_returns(ctl, H, gamma=0.9, wind=rows, want=WANT)
        for k in WANT:
            assert _same(by_rows[k], got[k]), k
    else:
        with pytest.raises(ValueError, match="needs a time-series episode"):
            env.controller_returns(ctl, H, wind="series")
    env.close()


def test_a_reward_shaper_is_refused_and_torch_envs_return_tensors():
    import torch
    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd.rewards import StepPercentage

    env = envs.make("Turb3_Row1_Floris", env_batch=2, max_num_steps=20, reward_shaper=StepPercentage())
    env.reset(seed=0)
    with pytest.raises(ValueError, match="plain reward"):
        env.controller_returns({"alpha": 1.0}, 3)
    env.close()
    c = rr.case("row3")
    env = envs.make("Turb3_Row1_Floris", env_batch=2, max_num_steps=20)
    env.reset(seed=0)
    _set_tables(env.fi, c["tables"])
    r = env.controller_returns(c["controllers"], 4, want=("returns", "actions", "best", "gated"))
    assert all(v.is_cuda for v in r.values()) and tuple(r["actions"].shape) == (2, c["K"], 4, 3) and r["gated"].dtype == torch.int32
    host = env.fi.controller_returns(c["controllers"], 4, want=("returns", "actions", "best", "gated"))
    for k in r:
        assert _same(r[k].cpu().numpy(), host[k]), k
    env.close()


def test_same_bits():
    """Ablaincourt_, five farms.  Strict: two runs, max_eval_farms = 2 K H + 1 (chunks of two slots, the last one ragged),
    a farm per chunk, a shuffled farm list, and torch tensors in and out give all the bits of the whole NumPy run.  Default
    mode: two runs on one evaluator agree bit for bit, and the trajectory outputs agree with the strict run's."""
    import torch

    name = "Ablaincourt_"
    c = rr.case(name)
    B, K, H = c["B"], c["K"], c["H"]
    whole = _device(name, True)
    kw = dict(gamma=c["gamma"], strict=True, want=WANT)
    w = _handle(c)
    again = w.controller_returns(c["controllers"], H, wind=c["wind"], **kw)
    chunks = w.controller_returns(c["controllers"], H, wind=c["wind"], max_eval_farms=2 * K * H + 1, **kw)
    single = w.controller_returns(c["controllers"], H, wind=c["wind"], max_eval_farms=K * H, **kw)
    farms = np.array([3, 0, 4, 1, 2])
    f0 = np.stack([c["ws"], c["wd"]], axis=1)[:, None, :].repeat(K, axis=1)
    sub = w.controller_returns(c["controllers"], H, wind=c["wind"][farms], filter0=f0[farms], farms=farms, max_eval_farms=2 * K * H + 1, **kw)
    t = w.controller_returns(c["controllers"], H, wind=torch.from_numpy(c["wind"].copy()).cuda(), **kw)
    d1 = w.controller_returns(c["controllers"], H, gamma=c["gamma"], wind=c["wind"], want=WANT)
    d2 = w.controller_returns(c["controllers"], H, gamma=c["gamma"], wind=c["wind"], want=WANT)
    timing = w.rollout_timing()
    w.close()
    assert all(v.is_cuda for v in t.values()) and t["best"].dtype == torch.int32 and t["gated"].dtype == torch.int32
    for k in WANT:
        assert _same(again[k], whole[k]), k
        assert _same(chunks[k], whole[k]), k
        assert _same(single[k], whole[k]), k
        assert _same(sub[k], whole[k][farms]), k  # (filter0 = the current wind is what None means)
        assert _same(t[k].cpu().numpy(), whole[k]), k
        assert _same(d1[k], d2[k]), k
    for k in TRAJECTORY:
        assert _same(d1[k], whole[k]), k
    assert timing["total_ms"] > 0.0


def test_the_handle_is_read_only():
    """Env state, wind, the pending speed's effect and the rose tables are unchanged by a call, bit for bit: env_get_state
    and get_wind before and after; lut_policy of every slot before and after; and the pending speed is still there — the
    env step that follows pays what it pays without the call in between."""
    c = rr.case("row3")
    w = _handle(c)
    w.env_set_prev_wind(c["ws"] * 1.1)
    st0, wind0 = w.env_get_state(), w.get_wind()
    pol0 = [w.lut_policy(s) for s in (0, 1)]
    got = w.controller_returns(c["controllers"], c["H"], gamma=c["gamma"], wind=c["wind"], want=WANT)
    st1, wind1 = w.env_get_state(), w.get_wind()
    pol1 = [w.lut_policy(s) for s in (0, 1)]
    paid = w.env_step(got["actions"][:, 0, 0].copy(), want=("reward",))["reward"]
    w.close()
    for k in st0:
        assert np.array_equal(st0[k], st1[k]) and np.array_equal(st0[k], np.asarray(c["state"][k]).reshape(st0[k].shape)), k
    assert np.array_equal(wind0[0], wind1[0]) and np.array_equal(wind0[1], wind1[1])
    for a, b in zip(pol0, pol1):
        assert _same(a["target_yaw"], b["target_yaw"]) and _same(a["action"], b["action"])
    w = _handle(c)  # the same step without the call in between
    w.env_set_prev_wind(c["ws"] * 1.1)
    alone = w.env_step(got["actions"][:, 0, 0].copy(), want=("reward",))["reward"]
    w.close()
    assert _same(paid, alone)


def _series_handle(c):
    """A WfStep at tick t of the series case, as VecWindFarmEnv would have left it: series set, t ticks each followed by a
    (holding) step, which consumes the pending speed, then the case's env state."""
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.env_config(load_coef=LOAD_COEF)
    w.set_wind_series(c["series"], start=c["start"])
    w.env_reset()
    for _ in range(c["t"]):
        w.wind_series_step()
        w.env_step(np.zeros((c["B"], c["N"]), np.float32), want=("reward",))
    w.env_set_state(c["state"])
    _set_tables(w, c["tables"])
    return w


def test_series_ahead():
    """The series case (4 rows left of a horizon of 6: the last row is held).  wind="series" equals the run given the same
    window as wind= — the rows gathered on the host from series_state() — bit for bit in every output (strict), with a farm
    list and a farm per chunk too; the trajectory has the reference's bits and the rewards are inside its bounds, step 0
    normalised by the current speed.  Two half-horizon calls chained through filter_final -> filter0, the env stepped in between
    with the first half's actions, reproduce the trajectory bits of the one full call.  The cursor is where it was."""
    import series_ref

    c, ref = rr.series_case(), rr.series_reference()
    B, K, H = c["B"], c["K"], c["H"]
    w = _series_handle(c)
    cur = w.series_state()
    assert cur["t"] == c["t"] and np.array_equal(cur["start"], c["start"]) and not cur["prev_pending"]
    rows, avail = series_ref.window(c["series"], cur["start"], cur["t"], 1, H)
    assert avail == c["available"] and np.array_equal(rows, c["rows"])
    ws, wd = w.get_wind()
    assert np.array_equal(ws, c["ws"]) and np.array_equal(wd, c["wd"])
    kw = dict(gamma=c["gamma"], strict=True, want=WANT)
    got = w.controller_returns(c["controllers"], H, wind="series", **kw)
    by_rows = w.controller_returns(c["controllers"], H, wind=rows, **kw)
    farms = [2, 0, 3]
    sub = w.controller_returns(c["controllers"], H, wind="series", farms=farms, max_eval_farms=K * H, **kw)
    after = w.series_state()
    assert (after["t"], after["prev_pending"]) == (cur["t"], cur["prev_pending"]) and np.array_equal(after["start"], cur["start"])
    for k in WANT:
        assert _same(got[k], by_rows[k]), k
        assert _same(sub[k], got[k][farms]), k
    _assert_trajectory_bits(got, ref, "series")
    b, pb, rb = rr.bounds(ref, LOAD_COEF, parity.TOL_F64, c["gamma"])
    er, ep, et = (np.abs(got[k] - ref[k]) for k in ("rewards", "farm_power", "returns"))
    print(f"series: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}, return {(et / rb).max():.3f}")
    assert (er <= b).all() and (ep <= pb).all() and (et <= rb).all()
    # two halves, chained: every controller on an env stepped with ITS first half
    h1 = H // 2
    first = w.controller_returns(c["controllers"], h1, wind="series", **kw)
    assert _same(first["actions"], got["actions"][:, :, :h1])
    ctl = c["controllers"]
    for k in range(K):
        w.series_seek(c["t"])
        w.env_set_state(c["state"])
        for h in range(h1):
            w.wind_series_step()
            w.env_step(first["actions"][:, k, h].copy(), want=("reward",))
        assert _same(w.env_get_state()["yaw"], first["final_yaw"][:, k])
        one = {f: ctl[f][k:k + 1] for f in ctl}
        second = w.controller_returns(one, H - h1, wind="series", filter0=first["filter_final"][:, k:k + 1], **kw)
        assert _same(second["actions"][:, 0], got["actions"][:, k, h1:]), k
        assert _same(second["final_yaw"][:, 0], got["final_yaw"][:, k]), k
        assert _same(second["filter_final"][:, 0], got["filter_final"][:, k]), k
        assert np.array_equal(first["gated"][:, k] + second["gated"][:, 0], got["gated"][:, k]), k
    # the end of the series: no row left for the coming step
    while w.series_state()["t"] < c["T"] - 1:
        w.wind_series_step()
        w.env_step(None, want=("yaw",))
    with pytest.raises(ValueError, match="WF_E_INVALID.*exhausted"):
        w.controller_returns(c["controllers"], H, wind="series")
    w.close()


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    c = rr.case("row3")
    x, y = c["x"], c["y"]
    N = 3
    one = {"alpha": 1.0}
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.controller_returns(one, 2)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.controller_returns(one, 2)
    w.set_wind(8.0, 270.0)
    T, twd, tws, interp = c["tables"][0]
    w.set_yaw_table(T, twd, tws, interp=interp, slot=0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.controller_returns(one, 2)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*no yaw table in that slot"):
        w.controller_returns({"slot": [0, 1]}, 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*slot out of range"):
        w.controller_returns({"slot": 4}, 2)
    for alpha in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*alpha must be in"):
            w.controller_returns({"alpha": [1.0, alpha]}, 2)
    for band in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*deadband must be finite and >= 0"):
            w.controller_returns({"deadband": band}, 2)
    for lead in (-1, 17):
        with pytest.raises(ValueError, match="WF_E_INVALID.*lead must be in 0..16"):
            w.controller_returns({"lead": lead}, 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K must be in 1..64"):
        w.controller_returns({"alpha": np.full(65, 0.5)}, 2)
    for H in (0, 1025):
        with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..1024"):
            w.controller_returns(one, H)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K H <= 4096"):
        w.controller_returns({"alpha": np.full(5, 0.5)}, 820)  # 4100 rows
    for gamma in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.controller_returns(one, 2, gamma=gamma)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.controller_returns({"alpha": [1.0, 0.5]}, 2, max_eval_farms=3)
    with pytest.raises(ValueError, match="farm index out of range"):
        w.controller_returns(one, 2, farms=[0, 2])
    with pytest.raises(ValueError, match="WF_E_INVALID.*needs a parent in series mode"):
        w.controller_returns(one, 2, wind="series")
    with pytest.raises(ValueError, match=r"\(n_farms, H, 2\)"):
        w.controller_returns(one, 2, wind=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match=r"\(n_farms, K, 2\)"):
        w.controller_returns(one, 2, filter0=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="common length K"):
        w.controller_returns({"alpha": [1.0, 0.5], "lead": [0, 1, 2]}, 2)
    with pytest.raises(ValueError, match="controllers must be a dict"):
        w.controller_returns({"gain": 1.0}, 2)
    with pytest.raises(ValueError, match="want must name"):
        w.controller_returns(one, 2, want=("reward",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.rollout_timing()
    # series-ahead together with a wind of the caller's own is refused by the library
    w.set_wind_series(np.array([[8.0, 270.0], [8.5, 272.0], [9.0, 268.0]]), start=np.zeros(2, np.int32))
    w.wind_series_step()
    ro = w._rollout()
    ro._call("set_series", 1)
    with pytest.raises(ValueError, match="WF_E_INVALID.*pass no wind of your own"):
        wind = np.zeros((2, 2, 2))
        k = np.zeros(1, np.int32), np.ones(1), np.zeros(1, np.float32), np.zeros(1, np.int32)
        ro._call("run", 1, k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data, k[3].ctypes.data, 2, wind.ctypes.data, None, 1.0, 2, None,
                 None, None, None, None, None, None, None, None, 0)
    r = w.controller_returns(one, 2, wind="series", farms=[1], max_eval_farms=2, want=WANT)  # (the handle still serves)
    assert r["returns"].shape == (1, 1) and np.isfinite(r["returns"]).all() and r["best"].tolist() == [0]
    full = w.controller_returns({"alpha": np.linspace(0.1, 1.0, 4)}, 1024, strict=True, want=("best", "returns", "gated"))  # the longest horizon
    assert full["returns"].shape == (2, 4) and np.isfinite(full["returns"]).all()
    wide = w.controller_returns({"deadband": np.arange(64) * 0.25}, 64, want=("best", "returns"))  # the most controllers, 4096 rows
    assert wide["returns"].shape == (2, 64) and np.isfinite(wide["returns"]).all() and ((wide["best"] >= 0) & (wide["best"] < 64)).all()
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_turbine_definitions_are_refused():
    from wfcrl_env_amd.backend import WfStep

    c = rr.case("row3")
    w = WfStep(c["x"], c["y"], env_batch=2)
    w.set_wind(8.0, 270.0)
    w.set_turbine_types([{}, {"gen_eff": 0.9}], [0, 1, 0])
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.controller_returns({"alpha": 1.0}, 2)
    w.close()


def test_kernel_info_shows_no_scratch():
    w = _handle(rr.case("row3"), state=False, tables=False)
    info = w.rollout_kernel_info()
    w.close()
    assert set(info) == {"layout", "reduce"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
