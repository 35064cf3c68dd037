"""GPU: scenario rollouts of yaw-table controllers on the device (include/wfrollscen.h) against tests/rollscen_ref.py — scenario_ref's
member paths and statistics around rollout_ref's closed loop, in NumPy over the float64 oracle.

BITS.  wind_paths, actions, final_yaw, gated and first_action do not see the solver: they have the reference's bits on every
case, in both modes, with no tolerance and no exempted entry; wind_paths also has the bits of scenario_returns' on the device.
BOUNDS need no measured number.  The step's contract is per turbine (tests/parity.py), carried through the reward's formula by
credit_ref.bound per ROW — TOL_F64 when every row is solved in float64 (strict), TOL in the handle's default mode —; a member
return is held to sum_h g_h bound_h, the mean to the mean of its members' bounds, the tail mean to the largest of them
(scenario_ref.carry), on EVERY entry.  The statistics are scenario_ref's of the device's OWN member returns, bit for bit.  The
measured fraction of the bound is printed.
BEST equals the reference's on EVERY farm of every case in both modes: tests/test_rollscen.py asserts, on the reference alone,
that the two best scores of every farm are further apart than the sum of their two bounds.

Cases (tests/rollscen_ref.py, the smallest shapes at which each branch can go wrong): the row of three (4 farms) in both
encodings and Turb16_Row5_ (32 farms) with K = 3, M = 5, H = 4, an anchor per farm, clipped speeds, load_coef 0.1 and 1.0; the
seam; the limits (1, 64, 64), (64, 8, 8), (4, 16, 64) and 1024 / 1040 rows — either side of the switch between brackets in LDS
and in global memory; a chunked run of a farm list.  Bit identity across chunk sizes and farm lists is asserted in STRICT mode,
where every row is solved by the float64 kernel, whose bits do not depend on the batch."""
import functools

import numpy as np
import pytest

import lookahead_ref
import parity
import rollscen_ref as R
import scenario_ref as S
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

STATS = ("expected_returns", "cvar", "score")
SOLVED = ("rewards", "member_returns") + STATS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _set_tables(w, tables):
    for slot, (T, twd, tws, interp) in tables.items():
        w.set_yaw_table(T, twd, tws, interp=interp, slot=slot)


def _handle(c, lc=0.1, state=True, tables=True):
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.set_wind(c["ws"], c["wd"])
    w.env_config(load_coef=lc, discrete=c["env"]["discrete"], dt=c["env"]["dt"])
    if state:
        w.env_reset()
        w.env_set_state(c["state"])
    if tables:
        _set_tables(w, c["tables"])
    return w


def _kw(c, **over):
    kw = dict(seed=c["seed"], gamma=c["gamma"], tail=c["tail"], risk_weight=c["lam"], anchor=c["anchor"], bounds=c["bounds"],
              filter0=c["filter0"], want=R.WANT)
    kw.update(over)
    return kw


def _run(w, c, controllers=None, **over):
    return w.controller_scenarios(c["controllers"] if controllers is None else controllers, c["H"], c["M"], S.process_of(c["process"]),
                                  **_kw(c, **over))


@functools.lru_cache(maxsize=None)
def _device(name, strict, lc=0.1):
    c = R.case(name)
    w = _handle(c, lc)
    r = _run(w, c, strict=strict)
    w.close()
    for v in r.values():
        v.setflags(write=False)
    return r


def _assert_free_bits(got, ref, label):
    """The solver-independent outputs: shapes, dtypes and the reference's bits."""
    for k, dtype in (("wind_paths", np.float64), ("actions", np.float32), ("final_yaw", np.float32), ("gated", np.int32),
                     ("first_action", np.float32)):
        assert got[k].dtype == dtype and got[k].shape == ref[k].shape, (label, k)
    for k in ("wind_paths", "actions", "final_yaw", "first_action"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (label, k, np.argwhere(_bits(got[k]) != _bits(ref[k]))[:5])
    assert np.array_equal(got["gated"], ref["gated"]), label


def _assert_solved(name, got, ref, lc, tol, label):
    """Every reward, member return and statistic inside its bound; the statistics those of the device's own member returns;
    best the reference's on every farm."""
    c = R.case(name)
    carry = S.carry(ref, lc, tol, c["gamma"], c["lam"])
    worst = {}
    for k in SOLVED:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64, (label, k)
        worst[k] = float((np.abs(got[k] - ref[k]) / carry[k]).max())
    print(f"{label}: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (label, k, v)
    assert np.array_equal(_bits(got["member_returns"]), _bits(lookahead_ref.discounted(got["rewards"], c["gamma"]))), label
    st = S.statistics(got["member_returns"], c["tail"], c["lam"])
    for k in STATS:
        assert np.array_equal(_bits(got[k]), _bits(st[k])), (label, k)
    assert got["best"].dtype == np.int32 and np.array_equal(got["best"], st["best"]), label
    assert R.clear(ref, lc, tol, c["gamma"], c["lam"]).all(), label  # (the reference alone: no farm is left out)
    assert np.array_equal(got["best"], ref["best"]), (label, got["best"], ref["best"])


@pytest.mark.parametrize("name", R.BASE)
def test_solver_independent_outputs_have_the_bits_of_the_reference(name):
    """wind_paths, actions, final_yaw, gated and first_action: the reference's bits, in strict and in default mode, under both
    load coefficients — the paths' draws and walk, the filter's float64 recurrence and its wrap, the look-up, the deadband, the
    gate, the accumulator and the counter are visible here without any tolerance.  wind_paths also equals what
    scenario_returns draws on the device for the same arguments."""
    c = R.case(name)
    for strict in (True, False):
        for lc in R.COEFS:
            _assert_free_bits(_device(name, strict, lc), R.reference(name, lc), (name, strict, lc))
    w = _handle(c)
    hold = np.full((c["B"], 1, c["H"], c["N"]), 1.0 if c["env"]["discrete"] else 0.0, np.float32)
    sc = w.scenario_returns(hold, c["M"], S.process_of(c["process"]), seed=c["seed"], anchor=c["anchor"], bounds=c["bounds"],
                            want=("wind_paths",))
    w.close()
    assert _same(sc["wind_paths"], _device(name, False)["wind_paths"])


@pytest.mark.parametrize("name", R.BASE)
def test_strict_against_the_reference(name):
    """Every row solved in float64: every reward, member return, mean, tail mean and score inside the bounds that follow from
    TOL_F64, with both load coefficients; the statistics of the device's own member returns; best on every farm."""
    for lc in R.COEFS:
        _assert_solved(name, _device(name, True, lc), R.reference(name, lc), lc, parity.TOL_F64, f"{name} strict load_coef {lc}")


@pytest.mark.parametrize("name", R.BASE)
def test_default_mode_against_the_reference(name):
    """The handle's own resolve mode: the same from TOL.  Nothing is exempted."""
    for lc in R.COEFS:
        _assert_solved(name, _device(name, False, lc), R.reference(name, lc), lc, parity.TOL, f"{name} default mode load_coef {lc}")


@pytest.mark.parametrize("name", R.LIMITS)
def test_limits_and_both_sides_of_the_bracket_switch(name):
    """(K, M, H) = (1, 64, 64), (64, 8, 8), (4, 16, 64): 4096 rows, the brackets in global memory, two lay-out tiles, the reduce
    kernel's wide block; 1024 rows (the most brackets LDS takes) and 1040 (the fewest that go through global memory).  The
    solver-independent bits in both modes, every bound, the statistics and best in both modes."""
    ref = R.reference(name)
    for strict, tol in ((True, parity.TOL_F64), (False, parity.TOL)):
        got = _device(name, strict)
        label = f"{name} {'strict' if strict else 'default mode'}"
        _assert_free_bits(got, ref, label)
        _assert_solved(name, got, ref, 0.1, tol, label)


def test_chunked_farm_list_gives_the_bits_of_the_whole_run():
    """Five farms, farms = [4, 0, 3], max_eval_farms = 2 K M H (a chunk of two slots and a ragged one), strict: the bits of the
    same farms unchunked and of the whole batch's entries — a farm's paths are those of its index in the batch."""
    c = R.case("chunks")
    farms = [4, 0, 3]
    rows = c["K"] * c["M"] * c["H"]
    whole = _device("chunks", True)
    w = _handle(c)
    over = dict(anchor=c["anchor"][farms], strict=True, farms=farms)
    listed = _run(w, c, **over)
    chunked = _run(w, c, max_eval_farms=2 * rows, **over)
    single = _run(w, c, max_eval_farms=rows, **over)
    w.close()
    ref = R.reference("chunks")
    for k in R.WANT:
        assert _same(chunked[k], listed[k]), k
        assert _same(single[k], listed[k]), k
        assert _same(listed[k], whole[k][farms]), k
    _assert_free_bits({k: chunked[k] for k in R.FREE}, {k: ref[k][farms] for k in R.FREE}, "chunks")
    _assert_solved("chunks", whole, ref, 0.1, parity.TOL_F64, "chunks strict")


@pytest.mark.parametrize("name", ["row3", "row3_discrete"])
def test_lookahead_of_the_actions_under_the_paths_gives_the_same_rewards(name):
    """Oracle-free, strict, no pending prev-wind: lookahead_returns fed with the actions of member m under member m's path
    returns rewards[:, :, m] bit for bit (and the member returns, and final_yaw): the scenario rollout is the look-ahead of what
    each controller issues under each member, row for row."""
    c = R.case(name)
    got = _device(name, True)
    w = _handle(c)
    for m in range(c["M"]):
        la = w.lookahead_returns(np.ascontiguousarray(got["actions"][:, :, m]), gamma=c["gamma"], wind=np.ascontiguousarray(got["wind_paths"][:, m]),
                                 strict=True, want=("returns", "rewards", "final_yaw"))
        assert _same(la["rewards"], np.ascontiguousarray(got["rewards"][:, :, m])), (name, m)
        assert _same(la["returns"], np.ascontiguousarray(got["member_returns"][:, :, m])), (name, m)
        assert _same(la["final_yaw"], np.ascontiguousarray(got["final_yaw"][:, :, m])), (name, m)
    w.close()


def test_one_still_member_is_controller_returns_under_the_held_wind():
    """M = 1 and a process of all zeros, strict: returns, actions and final_yaw are controller_returns(wind=None)'s, bit for bit,
    and the three statistics are that return."""
    c = R.case("row3")
    w = _handle(c)
    still = w.controller_scenarios(c["controllers"], c["H"], 1, dict(ws_revert=0.0), seed=3, gamma=c["gamma"], strict=True, want=R.WANT)
    held = w.controller_returns(c["controllers"], c["H"], gamma=c["gamma"], strict=True, want=("returns", "rewards", "actions", "final_yaw", "gated", "best"))
    w.close()
    for k in STATS:
        assert _same(still[k], held["returns"]), k
    assert _same(still["member_returns"][:, :, 0], held["returns"]) and _same(still["rewards"][:, :, 0], held["rewards"])
    assert _same(still["actions"][:, :, 0], held["actions"]) and _same(still["final_yaw"][:, :, 0], held["final_yaw"])
    assert _same(still["gated"][:, :, 0], held["gated"]) and _same(still["best"], held["best"])
    assert _same(still["first_action"], np.ascontiguousarray(held["actions"][:, :, 0]))


def test_determinism_and_independence():
    """Two default-mode runs on one evaluator agree bit for bit; a fourth controller changes nothing of the first three's
    outputs (strict); torch tensors in and out give the NumPy run's bits; the env state is unchanged and a pending prev-wind
    speed is neither used — the outputs have the bits of a run without it — nor consumed: the next env_step pays what it pays
    without the call in between."""
    import torch

    name = "row3"
    c = R.case(name)
    K = c["K"]
    whole = _device(name, True)
    w, plain = _handle(c), _handle(c)
    d1, d2 = _run(w, c), _run(w, c)
    more = {f: np.concatenate([c["controllers"][f], np.asarray([v], c["controllers"][f].dtype)])
            for f, v in (("alpha", 0.55), ("deadband", 1.25), ("lead", 2), ("slot", 1))}
    four = _run(w, c, controllers=more, strict=True)
    t = _run(w, c, strict=True, anchor=torch.from_numpy(c["anchor"].copy()).cuda())
    w.env_set_prev_wind(c["ws"] * 1.1)
    plain.env_set_prev_wind(c["ws"] * 1.1)
    before = w.env_get_state()
    pending = _run(w, c, strict=True)
    after = w.env_get_state()
    a = np.ascontiguousarray(whole["first_action"][:, 0])
    paid, want = w.env_step(a, want=("reward",))["reward"], plain.env_step(a, want=("reward",))["reward"]
    timing = w.controller_scenarios_timing()
    w.close(); plain.close()
    unpaid = _handle(c)
    other = unpaid.env_step(a, want=("reward",))["reward"]
    unpaid.close()
    assert all(v.is_cuda for v in t.values()) and t["best"].dtype == torch.int32 and t["gated"].dtype == torch.int32
    for k in R.WANT:
        assert _same(d1[k], d2[k]), k
        assert _same(t[k].cpu().numpy(), whole[k]), k
        assert _same(pending[k], whole[k]), k
        if k not in ("wind_paths", "best"):
            assert _same(np.ascontiguousarray(four[k][:, :K]), whole[k]), k
    assert _same(four["wind_paths"], whole["wind_paths"])
    for k in R.FREE:
        assert _same(d1[k], whole[k]), k
    for k in before:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], np.asarray(c["state"][k]).reshape(before[k].shape)), k
    assert np.array_equal(_bits(paid), _bits(want)) and (paid != other).all()  # (the pending speed was still there, and counts)
    assert timing["total_ms"] > 0.0


def test_vec_env_method():
    """VecWindFarmEnv.controller_scenarios on a wind_process env: process=None takes the env's process and its distribution's
    speed bounds, and agrees with WfStep.controller_scenarios on the same state, on a farm list too; controller_grid's dict is
    taken unchanged; the env is left as it was; an env without a process refuses with a clear message and serves when given
    one."""
    import torch
    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd.backend import WfStep

    B, Hv, Mv = 6, 3, 4
    proc = S.process_of(S.PROCESS)
    env = envs.make("Turb3_Row1_Floris", env_batch=B, max_num_steps=20, wind_process=dict(proc, dist=dict(ws_lo=5.0, ws_hi=9.0)))
    N = env.num_turbines
    c = R.case("row3")
    env.reset(seed=0)
    _set_tables(env.fi, c["tables"])
    gen = torch.Generator().manual_seed(0)
    env.step({"yaw": (torch.rand((B, N), generator=gen) * 10.0 - 5.0).cuda()})
    ctl, params = WfStep.controller_grid([1.0, 0.5], [0.0, 2.0], [0, 1], slot=1)
    Kv = len(params)
    before = env.get_state()
    want = ("expected_returns", "cvar", "score", "best", "wind_paths", "first_action", "gated")
    r = env.controller_scenarios(ctl, Hv, members=Mv, seed=9, gamma=0.95, tail=2, risk_weight=0.5, want=want)
    assert set(r) == set(want) and all(v.is_cuda for v in r.values())
    assert tuple(r["score"].shape) == (B, Kv) and r["score"].dtype == torch.float64 and r["best"].dtype == torch.int32
    assert tuple(r["wind_paths"].shape) == (B, Mv, Hv, 2) and tuple(r["first_action"].shape) == (B, Kv, N)
    assert tuple(r["gated"].shape) == (B, Kv, Mv) and r["gated"].dtype == torch.int32
    direct = env.fi.controller_scenarios(ctl, Hv, Mv, proc, seed=9, gamma=0.95, tail=2, risk_weight=0.5, bounds=(5.0, 9.0), want=want)
    for k in r:
        assert np.array_equal(_bits(r[k].cpu().numpy()), _bits(direct[k])), k
    assert float(r["wind_paths"][..., 0].min()) >= 5.0 and float(r["wind_paths"][..., 0].max()) <= 9.0
    assert torch.equal(r["best"].long(), r["score"].argmax(dim=1))
    strict = env.controller_scenarios(ctl, Hv, members=Mv, seed=9, strict=True)
    sub = env.controller_scenarios(ctl, Hv, members=Mv, seed=9, farms=[5, 2], strict=True)
    for k in sub:
        assert torch.equal(sub[k], strict[k][[5, 2]]), k
    after = env.get_state()
    assert set(before) == set(after)
    for k in before:
        assert (before[k] is None and after[k] is None) or np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    env.close()
    plain = envs.make("Turb3_Row1_Floris", env_batch=B, max_num_steps=20)
    plain.reset(seed=0)
    _set_tables(plain.fi, c["tables"])
    with pytest.raises(ValueError, match="needs a wind process.*built without wind_process"):
        plain.controller_scenarios(ctl, Hv)
    given = plain.controller_scenarios(ctl, Hv, members=Mv, process=proc)  # (a held-wind episode: only the current wind is read)
    assert tuple(given["score"].shape) == (B, Kv) and bool(torch.isfinite(given["score"]).all())
    plain.close()


def test_refusals_name_their_cause():
    """Each refusal — the union of controller_returns' and scenario_returns' — carries its code and a message, and nothing is
    launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    c = R.case("row3")
    x, y = ROW3
    N = 3
    proc = S.process_of(S.PROCESS)
    one = {"alpha": 1.0}
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.controller_scenarios(one, 2, 2, proc)
    w.close()
    w = WfStep(x, y, env_batch=2)
    w.set_wind(8.0, 270.0)
    w.set_turbine_types([{}, {"gen_eff": 0.9}], [0, 1, 0])
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.controller_scenarios(one, 2, 2, proc)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.controller_scenarios(one, 2, 2, proc)
    w.set_wind(8.0, 270.0)
    T, twd, tws, interp = c["tables"][0]
    w.set_yaw_table(T, twd, tws, interp=interp, slot=0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.controller_scenarios(one, 2, 2, proc)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*no yaw table in that slot"):  # an empty slot
        w.controller_scenarios({"slot": [0, 1]}, 2, 2, proc)
    with pytest.raises(ValueError, match="WF_E_INVALID.*slot out of range"):
        w.controller_scenarios({"slot": 4}, 2, 2, proc)
    for alpha in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*alpha must be in"):
            w.controller_scenarios({"alpha": [1.0, alpha]}, 2, 2, proc)
    for band in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*deadband must be finite and >= 0"):
            w.controller_scenarios({"deadband": band}, 2, 2, proc)
    for lead in (-1, 17):
        with pytest.raises(ValueError, match="WF_E_INVALID.*lead must be in 0..16"):
            w.controller_scenarios({"lead": lead}, 2, 2, proc)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K must be in 1..64"):
        w.controller_scenarios({"alpha": np.full(65, 0.5)}, 1, 1, proc)
    for H in (0, 65):
        with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
            w.controller_scenarios(one, H, 1, proc)
    for members in (0, 65, -3):
        with pytest.raises(ValueError, match="WF_E_INVALID.*M must be in 1..64"):
            w.controller_scenarios(one, 2, members, proc)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K M H <= 4096"):
        w.controller_scenarios({"alpha": np.full(2, 0.5)}, 64, 33, proc)  # 4224 rows
    with pytest.raises(ValueError, match="WF_E_INVALID.*K M H <= 4096"):
        w.controller_scenarios({"alpha": np.full(64, 0.5)}, 13, 5, proc)  # 4160 rows
    for tail in (0, 3, -1):
        with pytest.raises(ValueError, match="WF_E_INVALID.*tail must be in 1..M"):
            w.controller_scenarios(one, 2, 2, proc, tail=tail)
    for v in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.controller_scenarios(one, 2, 2, proc, gamma=v)
        with pytest.raises(ValueError, match="WF_E_INVALID.*risk_weight"):
            w.controller_scenarios(one, 2, 2, proc, risk_weight=v)
    for bad in (dict(ws_revert=1.5), dict(wd_revert=-0.1), dict(ws_revert=float("nan"))):
        with pytest.raises(ValueError, match="WF_E_INVALID.*ws_revert and wd_revert must be in"):
            w.controller_scenarios(one, 2, 2, dict(proc, **bad))
    for bad in (dict(ws_sigma=-1.0), dict(wd_sigma=float("inf")), dict(wd_ramp=-0.5)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*ws_sigma, wd_sigma and wd_ramp"):
            w.controller_scenarios(one, 2, 2, dict(proc, **bad))
    with pytest.raises(ValueError, match="unknown wind process parameter"):
        w.controller_scenarios(one, 2, 2, dict(proc, sigma=1.0))
    with pytest.raises(ValueError, match="needs a wind process"):
        w.controller_scenarios(one, 2, 2, None)
    for bounds in ((9.0, 9.0), (10.0, 4.0), (0.0, 9.0), (3.0, float("inf")), (float("nan"), 9.0)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*speed bounds"):
            w.controller_scenarios(one, 2, 2, proc, bounds=bounds)
    for anchor in ([[8.0, 270.0], [0.0, 270.0]], [[-1.0, 270.0], [8.0, 270.0]], [[8.0, float("nan")], [8.0, 270.0]]):
        with pytest.raises(ValueError, match="WF_E_INVALID.*anchor's speed must be > 0"):
            w.controller_scenarios(one, 2, 2, proc, anchor=anchor)
    with pytest.raises(ValueError, match=r"anchor must be \(n_farms, 2\)"):
        w.controller_scenarios(one, 2, 2, proc, anchor=[8.0, 270.0])
    with pytest.raises(ValueError, match=r"filter0 must be \(n_farms, K, 2\)"):
        w.controller_scenarios(one, 2, 2, proc, filter0=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.controller_scenarios({"alpha": [1.0, 0.5]}, 2, 2, proc, max_eval_farms=7)  # K M H = 8
    with pytest.raises(ValueError, match="farm index out of range"):
        w.controller_scenarios(one, 2, 2, proc, farms=[0, 2])
    with pytest.raises(ValueError, match="common length K"):
        w.controller_scenarios({"alpha": [1.0, 0.5], "lead": [0, 1, 2]}, 2, 2, proc)
    with pytest.raises(ValueError, match="controllers must be a dict"):
        w.controller_scenarios({"gain": 1.0}, 2, 2, proc)
    with pytest.raises(ValueError, match="want must name"):
        w.controller_scenarios(one, 2, 2, proc, want=("returns",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.controller_scenarios_timing()
    r = w.controller_scenarios({"alpha": [1.0, 0.5]}, 2, 2, proc, farms=[1], max_eval_farms=8, want=R.WANT)  # (the handle still serves)
    assert r["score"].shape == (1, 2) and np.isfinite(r["score"]).all() and r["best"].tolist() in ([0], [1])
    assert r["member_returns"].shape == (1, 2, 2) and r["wind_paths"].shape == (1, 2, 2, 2) and r["actions"].shape == (1, 2, 2, 2, N)
    assert r["final_yaw"].shape == (1, 2, 2, N) and r["gated"].shape == (1, 2, 2) and r["first_action"].shape == (1, 2, N)
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_kernel_info_shows_no_scratch():
    """The runtime's report of the three kernels: no private segment — at N = 3 here, and at any N: a thread holds one turbine."""
    w = _handle(R.case("row3"), state=False, tables=False)
    info = w.controller_scenarios_kernel_info()
    w.close()
    assert set(info) == {"layout", "layout_spill", "reduce"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
