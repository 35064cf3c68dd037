"""GPU: the receding-horizon planner on the device (include/wfplan.h) against tests/plan_ref.py — the same draws, candidates,
trajectories, returns, ranks, elite means and winners in NumPy over the float64 oracle.

No measured number enters.  An order of two returns is the same on the device and in the reference when they are further
apart than the sum of their return bounds (tests/test_lookahead_gpu.py: sum_h g_h credit_ref.bound_h, TOL_F64 in strict
mode); plan_ref records per farm the smallest such margin over every decision of every iteration, and on a SAFE farm — a
positive margin — the device's plan, mean, first action and final yaw are held to the reference's BITS: they are float32
values that went through no solve.  plan_return and hold_return are held to their own return bounds on every farm.  The
cases (tests/plan_cases.py: A, the row of three with open and closed gates; B, Ablaincourt with a wind per step and a warm
start) have no unsafe farm — tests/test_plan.py checks that with the reference alone; the cap is 10 %.

Bit identity across chunk sizes and farm lists is asserted in STRICT mode, where every row is solved by the float64 kernel,
whose bits do not depend on the batch; in the default mode two runs on one evaluator are compared."""
import functools

import numpy as np
import pytest

import credit_ref
import lookahead_ref
import parity
import plan_cases
from plan_cases import GAMMA, LOAD_COEF
from test_lookahead import PARAMS
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

WANT = ("plan", "plan_return", "hold_return", "first_action", "final_yaw", "mean")
BITS = ("plan", "mean", "first_action", "final_yaw")


def _handle(name, discrete=False, state=True):
    from wfcrl_env_amd.backend import WfStep

    c = plan_cases.case(name)
    w = WfStep(c["x"], c["y"], env_batch=c["farms"])
    w.set_wind(c["ws"], c["wd"])
    w.env_config(load_coef=LOAD_COEF, discrete=discrete, dt=PARAMS["dt"])
    if state:
        w.env_reset()
        w.env_set_state(c["state"])
    return w


def _kw(name, **over):
    c = plan_cases.case(name)
    kw = dict(candidates=c["K"], elites=c["E"], sigma=c["sigma"], seed=c["seed"], gamma=GAMMA, wind=c["wind"], mean=c["mean0"], want=WANT)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    w = _handle(name)
    r = w.plan_actions(plan_cases.case(name)["H"], strict=strict, **_kw(name))
    w.close()
    for v in r.values():
        v.setflags(write=False)
    return r


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                                        b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("name", ["A", "B"])
def test_strict_against_the_reference(name):
    """Every row solved in float64: on safe farms plan, mean, first_action and final_yaw have the reference's bits; on
    every farm plan_return and hold_return are inside their return bounds; at most 10 % of the farms are unsafe."""
    c, ref, got = plan_cases.case(name), plan_cases.reference(name), _device(name, True)
    B, H, N = c["farms"], c["H"], c["N"]
    shapes = {"plan": (B, H, N), "mean": (B, H, N), "first_action": (B, N), "final_yaw": (B, N), "plan_return": (B,), "hold_return": (B,)}
    for k, s in shapes.items():
        assert got[k].shape == s and got[k].dtype == (np.float64 if k.endswith("return") else np.float32), k
    safe = ref["safe"]
    eh, ep = np.abs(got["hold_return"] - ref["hold_return"]), np.abs(got["plan_return"] - ref["plan_return"])
    print(f"case {name}: {int((~safe).sum())} of {B} farms unsafe (smallest margin {ref['margin'].min():.2e}); largest error / bound: "
          f"hold_return {(eh / ref['hold_bound']).max():.3f}, plan_return {(ep / ref['plan_bound']).max():.3f}")
    assert (~safe).sum() <= 0.1 * B
    for k in BITS:
        assert _same(got[k][safe], ref[k][safe]), k
    assert (eh <= ref["hold_bound"]).all() and (ep <= ref["plan_bound"]).all()
    assert np.array_equal(got["first_action"], got["plan"][:, 0])
    assert (got["plan"] != 0.0).any() and (got["plan_return"] > got["hold_return"]).any()  # (the search moved)


@pytest.mark.parametrize("name", ["A", "B"])
def test_default_mode(name):
    """The handle's own resolve mode: the plan is never worse than the hold, exactly; its return is what lookahead_returns
    pays for it, within the sum of the two default-mode bounds (equal bits are not required: another batch may run on
    another kernel family); final_yaw is that call's, bit for bit."""
    c = plan_cases.case(name)
    w = _handle(name)
    got = w.plan_actions(c["H"], **_kw(name))
    again = w.plan_actions(c["H"], **_kw(name))
    la = w.lookahead_returns(got["plan"][:, None].copy(), gamma=GAMMA, wind=c["wind"], want=("returns", "final_yaw"))
    w.close()
    for k in WANT:
        assert _same(got[k], again[k]), k
    assert (got["plan_return"] >= got["hold_return"]).all()
    ref = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], got["plan"][:, None], dict(PARAMS, discrete=False), GAMMA,
                                  LOAD_COEF, wind=c["wind"])
    b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, parity.TOL).reshape(c["farms"], c["H"])
    rb = (lookahead_ref.discounts(GAMMA, c["H"]) * b).sum(axis=1)
    err = np.abs(got["plan_return"] - la["returns"][:, 0])
    print(f"case {name}, default mode: largest |plan_return - lookahead return| / (2 bounds) {(err / (2.0 * rb)).max():.3f}; "
          f"median gain over the hold {np.median(got['plan_return'] - got['hold_return']):.3f}")
    assert (err <= 2.0 * rb).all()
    assert (np.abs(got["plan_return"] - ref["returns"][:, 0]) <= rb).all()  # (and the oracle's return of that plan)
    assert _same(got["final_yaw"], np.ascontiguousarray(la["final_yaw"][:, 0]))
    assert _same(got["final_yaw"], ref["final_yaw"][:, 0])


@pytest.mark.parametrize("name", ["A", "B"])
def test_same_bits(name):
    """Strict: a second run, chunks of three farms (A: 3, 3 and a ragged 2), a farm per chunk, a shuffled sub-list of farms
    and torch tensors in and out give the bits of the whole NumPy run; another seed gives another plan."""
    import torch

    c = plan_cases.case(name)
    B, H, R = c["farms"], c["H"], c["K"] * c["H"]
    whole = _device(name, True)
    w = _handle(name)
    again = w.plan_actions(H, strict=True, **_kw(name))
    chunks = w.plan_actions(H, strict=True, max_eval_farms=3 * R + 1, **_kw(name))
    single = w.plan_actions(H, strict=True, max_eval_farms=R, **_kw(name))
    farms = np.random.default_rng(5).permutation(B)[:5]
    sub = w.plan_actions(H, strict=True, farms=farms, **_kw(name, wind=None if c["wind"] is None else c["wind"][farms],
                                                           mean=None if c["mean0"] is None else c["mean0"][farms]))
    other = w.plan_actions(H, strict=True, **_kw(name, seed=c["seed"] + 1))
    out = {k: torch.empty(whole[k].shape, dtype=torch.float32 if whole[k].dtype == np.float32 else torch.float64, device="cuda") for k in WANT}
    tw = None if c["wind"] is None else torch.from_numpy(c["wind"].copy()).cuda()
    tm = None if c["mean0"] is None else torch.from_numpy(c["mean0"].copy()).cuda()
    t = w.plan_actions(H, strict=True, out=out, **_kw(name, wind=tw, mean=tm))
    timing = w.plan_timing()
    w.close()
    assert all(t[k] is out[k] and t[k].is_cuda for k in WANT)
    for k in WANT:
        assert _same(again[k], whole[k]), k
        assert _same(chunks[k], whole[k]), k
        assert _same(single[k], whole[k]), k
        assert _same(sub[k], np.ascontiguousarray(whole[k][farms])), k
        assert _same(t[k].cpu().numpy(), whole[k]), k
    assert (other["plan"] != whole["plan"]).any(axis=(1, 2)).any()
    assert _same(other["hold_return"], whole["hold_return"])  # (the hold does not see the seed)
    assert timing["total_ms"] > 0.0


def test_parent_untouched():
    """The parent's env state and its step outputs are the same bits before and after a run; a pending prev-wind speed is
    read (the hold's return is normalised by it) and not consumed."""
    c = plan_cases.case("B")
    w = _handle("B")
    yaw = np.asarray(c["state"]["yaw"]).copy()
    before, out0 = w.env_get_state(), w.step(yaw)
    plain = w.plan_actions(c["H"], **_kw("B", want=("hold_return",)))
    w.env_set_prev_wind(c["ws"] * 1.1)
    got = w.plan_actions(c["H"], **_kw("B", want=("hold_return",)))
    after, out1 = w.env_get_state(), w.step(yaw)
    w.close()
    for k in before:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], np.asarray(c["state"][k]).reshape(before[k].shape)), k
    for k in out0:
        assert np.array_equal(out0[k], out1[k]), k
    assert (got["hold_return"] != plain["hold_return"]).all()


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    N = 3
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.plan_actions(2)
    w.close()
    w = WfStep(x, y, env_batch=2)
    w.set_wind(8.0, 270.0)
    w.set_turbine_types([{}, {"gen_eff": 0.9}], [0, 1, 0])
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.plan_actions(2)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.plan_actions(2)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.plan_actions(2)
    w.env_config(discrete=True)
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*configured discrete"):
        w.plan_actions(2)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
        w.plan_actions(65, candidates=3, elites=1)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K must be >= 3"):
        w.plan_actions(2, candidates=2, elites=1)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K H <= 4096"):
        w.plan_actions(17, candidates=241, elites=8)  # 4097 rows
    with pytest.raises(ValueError, match="WF_E_INVALID.*E must be in 1..K"):
        w.plan_actions(2, candidates=8, elites=0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*E must be in 1..K"):
        w.plan_actions(2, candidates=8, elites=9)
    with pytest.raises(ValueError, match="WF_E_INVALID.*I must be >= 1"):
        w.plan_actions(2, sigma=())
    for bad in ((5.0, -1.0), (float("nan"),), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="WF_E_INVALID.*sigma must be finite and non-negative"):
            w.plan_actions(2, sigma=bad)
    for gamma in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.plan_actions(2, gamma=gamma)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.plan_actions(2, candidates=8, elites=2, max_eval_farms=15)  # K H = 16
    with pytest.raises(ValueError, match="farm index out of range"):
        w.plan_actions(2, farms=[0, 2])
    with pytest.raises(ValueError, match=r"\(n_farms, H, 2\)"):
        w.plan_actions(2, wind=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match=r"\(n_farms, H, num_turbines\)"):
        w.plan_actions(2, mean=np.zeros((2, 2, N + 1), np.float32))
    with pytest.raises(ValueError, match="want must name"):
        w.plan_actions(2, want=("returns",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.plan_timing()
    r = w.plan_actions(2, candidates=8, elites=2, farms=[1], max_eval_farms=16, want=WANT)  # (the handle still serves)
    assert r["plan"].shape == (1, 2, N) and np.isfinite(r["plan_return"]).all() and (r["plan_return"] >= r["hold_return"]).all()
    # the largest K; zero widths: every candidate holds, the plan is the hold
    full = w.plan_actions(1, candidates=4096, elites=4096, sigma=(0.0,), strict=True, want=("plan", "plan_return", "hold_return", "mean"))
    assert not full["plan"].any() and not full["mean"].any() and np.array_equal(full["plan_return"], full["hold_return"])
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_vec_env_round_trip():
    """VecWindFarmEnv.plan_actions after reset(seed=0) and two steps: torch tensors out, agreement with WfStep.plan_actions on
    the same state, the env left as it was; then executing first_action with `step` lands on the plan's first yaw row — the
    yaw lookahead_returns reports after step 0 of the plan — bit for bit."""
    import torch
    from wfcrl_env_amd import environments as envs

    B, Hv = 8, 3
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    N = env.num_turbines
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        env.step({"yaw": (torch.rand((B, N), generator=gen) * 10.0 - 5.0).cuda()})
    before = env.fi.env_get_state()
    r = env.plan_actions(Hv, candidates=16, elites=4, seed=3, gamma=0.95, want=WANT)
    assert set(r) == set(WANT) and all(v.is_cuda for v in r.values())
    assert tuple(r["plan"].shape) == (B, Hv, N) and r["plan"].dtype == torch.float32 and r["plan_return"].dtype == torch.float64
    direct = env.fi.plan_actions(Hv, candidates=16, elites=4, seed=3, gamma=0.95, want=WANT)
    for k in WANT:
        assert np.array_equal(r[k].cpu().numpy(), direct[k]), k
    sub = env.plan_actions(Hv, candidates=16, elites=4, seed=3, gamma=0.95, farms=[5, 2], strict=True, want=("plan",))
    strict = env.plan_actions(Hv, candidates=16, elites=4, seed=3, gamma=0.95, strict=True, want=("plan",))
    assert torch.equal(sub["plan"], strict["plan"][[5, 2]])
    assert (r["plan_return"] >= r["hold_return"]).all() and torch.equal(r["first_action"], r["plan"][:, 0])
    first_row = env.lookahead_returns(r["plan"][:, None, :1].contiguous())["final_yaw"][:, 0]  # the yaw after step 0 of the plan
    after = env.fi.env_get_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    env.step({"yaw": r["first_action"]})
    landed = env.fi.env_get_state()["yaw"]
    assert np.array_equal(landed.view(np.uint32), first_row.cpu().numpy().view(np.uint32))
    assert (landed != before["yaw"]).any()
    warm = torch.cat([r["mean"][:, 1:], r["mean"][:, -1:]], dim=1)  # the receding horizon: the mean shifted by one step
    nxt = env.plan_actions(Hv, candidates=16, elites=4, seed=4, gamma=0.95, mean=warm)
    assert set(nxt) == {"first_action", "plan_return"} and tuple(nxt["first_action"].shape) == (B, N)
    env.close()


def test_kernel_info_shows_no_scratch():
    w = _handle("A", state=False)
    info = w.plan_kernel_info()
    w.close()
    assert set(info) == {"advance"}
    assert info["advance"]["scratch_bytes"] == 0 and info["advance"]["vgprs"] > 0, info
