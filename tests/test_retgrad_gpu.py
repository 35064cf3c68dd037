"""GPU: the gradient of look-ahead returns with respect to the action sequences on the device (include/wfretgrad.h) against
tests/retgrad_ref.py — the same trajectories, flags, rows, quotients and sweep in NumPy over the float64 oracle.

The bounds need no measured number.  The step's contract is per turbine (tests/parity.py), carried through the reward's
formula by credit_ref.bound per ROW — TOL_F64 when every row is solved in float64 (strict), TOL in the handle's default mode —,
through the quotient as (bound(row+) + bound(row-)) / d and through the sweep, which is linear in the quotients, with the
reference's flags and discounts (retgrad_cases.bounds; the sweep's own float64 rounding is counted from its 2 H operations).
On EVERY entry; nothing is exempted.  What the flags, the trajectory and the terminal gradient contribute has no tolerance
at all.  tests/test_retgrad.py asserts on the reference alone that the strict bound is not vacuous on these inputs
(tests/retgrad_cases.py describes them and why their shapes are the smallest that take each loop of the kernels round twice).

Bit identity across chunk sizes and farm lists is asserted in STRICT mode, where every row is solved by the float64 kernel,
whose bits do not depend on the batch; in the default mode only two runs on the same evaluator are compared
(tests/test_lookahead_gpu.py: test_same_bits)."""
import functools

import numpy as np
import pytest

import lookahead_ref
import parity
import retgrad_cases
import retgrad_ref
from retgrad_cases import DELTA, GAMMA, LOAD_COEF, PARAMS
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

NAMES = tuple(retgrad_cases.CASES)
BASE = ("returns", "rewards", "farm_power", "final_yaw", "best")
WANT = BASE + ("action_gradient", "reward_gradient", "state_gradient", "yaw", "pass_mask")
SHAPES = {"returns": "BK", "rewards": "BKH", "farm_power": "BKH", "final_yaw": "BKN", "best": "B", "action_gradient": "BKHN",
          "reward_gradient": "BKHN", "state_gradient": "BKN", "yaw": "BKHN", "pass_mask": "BKHN"}
DTYPES = dict(dict.fromkeys(WANT, np.float64), final_yaw=np.float32, yaw=np.float32, best=np.int32, pass_mask=np.uint8)


def _handle(name, state=True, discrete=False):
    from wfcrl_env_amd.backend import WfStep

    c = retgrad_cases.case(name)
    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.set_wind(c["ws"], c["wd"])
    w.env_config(load_coef=LOAD_COEF, discrete=discrete, dt=PARAMS["dt"])
    if state:
        w.env_reset()
        w.env_set_state(c["state"])
    return w


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    w = _handle(name)
    r = w.return_gradient(retgrad_cases.case(name)["actions"], gamma=GAMMA, delta=DELTA, strict=strict, want=WANT)
    w.close()
    return retgrad_cases.freeze(r)


def _same(a, b, keys=WANT):
    for k in keys:
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (a[k], b[k]))
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def _inside(got, ref, b, label):
    """Every bounded output inside its bound; prints the largest error / bound ratios."""
    ratios = {}
    for k in ("rewards", "farm_power", "returns", "reward_gradient", "action_gradient", "state_gradient"):
        err = np.abs(got[k] - ref[k])
        ratios[k] = float(np.max(np.where(err == 0.0, 0.0, err / np.where(b[k] > 0.0, b[k], 1.0)))) if (b[k] > 0.0).any() else 0.0
        assert (err <= b[k]).all(), (label, k, ratios[k])
    print(f"{label}: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(name, strict):
    """yaw, final_yaw and pass_mask have the reference's bits in both modes; every base reward, farm power and return, every
    quotient, every action gradient and every state gradient lies inside the bound the step's contract implies."""
    c, ref, got = retgrad_cases.case(name), retgrad_cases.reference(name), _device(name, strict)
    dims = dict(B=c["B"], K=c["K"], H=c["H"], N=c["N"])
    for k in WANT:
        assert got[k].shape == tuple(dims[d] for d in SHAPES[k]) and got[k].dtype == DTYPES[k], k
    for k in ("yaw", "final_yaw", "pass_mask"):
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k
    assert np.array_equal(got["final_yaw"], got["yaw"][:, :, -1])
    b = retgrad_cases.bounds(ref, parity.TOL_F64 if strict else parity.TOL)
    _inside(got, ref, b, f"{name} {'strict' if strict else 'default mode'}")
    # what does not depend on the solver: the return and the sweep of the device's OWN rewards and quotients, bit for bit
    assert np.array_equal(got["returns"], lookahead_ref.discounted(got["rewards"], GAMMA))
    ag, sg = retgrad_ref.sweep(got["reward_gradient"], ref["pass_mask"], GAMMA)
    assert np.array_equal(got["action_gradient"], ag) and np.array_equal(got["state_gradient"], sg)
    assert np.array_equal(got["best"], np.argmax(got["returns"], axis=1))
    closed = (ref["pass_mask"] & 1) == 0
    assert (got["action_gradient"][closed] == 0.0).all() and (got["reward_gradient"][ref["d"] <= 0.0] == 0.0).all()


def test_terminal_gradient():
    """A terminal gradient enters the sweep before step H - 1's term.  With gamma = 0 (H = 5: g_{H-1} = 0) the entries of step
    H - 1 are s * terminal bit for bit, and every earlier entry but step 0's is the terminal value carried through the
    reference's t flags, exactly; with gamma = 0.9 every entry is inside the sweep's bound, whose terminal part is rounding
    alone."""
    name = "row3"
    c, ref = retgrad_cases.case(name), retgrad_cases.reference(name)
    terminal = np.random.default_rng(2).normal(0.0, 0.01, (c["B"], c["K"], c["N"]))
    w = _handle(name)
    kw = dict(delta=DELTA, strict=True, terminal=terminal, want=("action_gradient", "state_gradient", "reward_gradient", "returns"))
    zero = w.return_gradient(c["actions"], gamma=0.0, **kw)
    got = w.return_gradient(c["actions"], gamma=GAMMA, **kw)
    w.close()
    q0 = np.zeros(ref["reward_gradient"].shape)
    carried = retgrad_ref.sweep(q0, ref["pass_mask"], 0.0, terminal)[0]
    assert np.array_equal(zero["action_gradient"][:, :, 1:], carried[:, :, 1:]) and (carried[:, :, 1:] != 0.0).any()
    s_last = (ref["pass_mask"][:, :, -1] & 1) != 0
    assert np.array_equal(zero["action_gradient"][:, :, -1], np.where(s_last, terminal, 0.0))
    assert np.array_equal(zero["returns"], _device(name, True)["rewards"][:, :, 0])  # (the return excludes the terminal value)
    full = retgrad_ref.sweep(ref["reward_gradient"], ref["pass_mask"], GAMMA, terminal)
    b = retgrad_cases.bounds(ref, parity.TOL_F64, terminal=terminal)
    assert (np.abs(got["action_gradient"] - full[0]) <= b["action_gradient"]).all()
    assert (np.abs(got["state_gradient"] - full[1]) <= b["state_gradient"]).all()
    assert np.array_equal(got["reward_gradient"], _device(name, True)["reward_gradient"])
    own = retgrad_ref.sweep(got["reward_gradient"], ref["pass_mask"], GAMMA, terminal)
    assert np.array_equal(got["action_gradient"], own[0]) and np.array_equal(got["state_gradient"], own[1])


@pytest.mark.parametrize("name", ["row3", "abl"])
def test_base_outputs_are_lookahead_returns(name):
    """The same handle, state and actions: in strict mode returns, rewards, farm_power, final_yaw and best have the bits of
    lookahead_returns' (the float64 kernel's bits do not depend on the batch the row sits in); in the default mode every
    entry lies within the sum of the two runs' bounds."""
    c, ref = retgrad_cases.case(name), retgrad_cases.reference(name)
    w = _handle(name)
    la = w.lookahead_returns(c["actions"], gamma=GAMMA, strict=True, want=BASE)
    rg = w.return_gradient(c["actions"], gamma=GAMMA, delta=DELTA, strict=True, want=BASE)
    la32 = w.lookahead_returns(c["actions"], gamma=GAMMA, want=BASE)
    rg32 = w.return_gradient(c["actions"], gamma=GAMMA, delta=DELTA, want=BASE)
    w.close()
    assert set(rg) == set(BASE)
    _same(rg, la, BASE)
    b = retgrad_cases.bounds(ref, parity.TOL)
    for k in ("rewards", "farm_power", "returns"):
        assert (np.abs(rg32[k] - la32[k]) <= 2.0 * b[k]).all(), k
    assert np.array_equal(rg32["final_yaw"], la32["final_yaw"])


def test_same_bits():
    """Strict: two runs; max_eval_farms set so that the six farms need three chunks (2 R + 1) and a ragged last chunk
    (4 R + 1); a shuffled farm list; torch tensors in and out — all give the bits of the whole NumPy run.  Two default-mode
    runs on one evaluator agree bit for bit."""
    import torch

    name = "row3"
    c = retgrad_cases.case(name)
    act, B, R = c["actions"], c["B"], c["K"] * c["H"] * (2 * c["N"] + 1)
    whole = _device(name, True)
    kw = dict(gamma=GAMMA, delta=DELTA, strict=True, want=WANT)
    w = _handle(name)
    again = w.return_gradient(act, **kw)
    three = w.return_gradient(act, max_eval_farms=2 * R + 1, **kw)
    ragged = w.return_gradient(act, max_eval_farms=4 * R + 1, **kw)
    farms = np.random.default_rng(5).permutation(B)[:4]
    sub = w.return_gradient(act[farms], farms=farms, **kw)
    t = w.return_gradient(torch.from_numpy(act.copy()).cuda(), **kw)
    out = {"action_gradient": torch.empty(act.shape, dtype=torch.float64, device="cuda")}
    t0 = w.return_gradient(torch.from_numpy(act.copy()).cuda(), gamma=GAMMA, delta=DELTA, strict=True, want="action_gradient", out=out)
    d1, d2 = (w.return_gradient(act, gamma=GAMMA, delta=DELTA, want=WANT) for _ in range(2))
    timing = w.return_gradient_timing()
    w.close()
    assert all(v.is_cuda for v in t.values()) and t0["action_gradient"] is out["action_gradient"] and set(t0) == {"action_gradient"}
    assert t["pass_mask"].dtype == torch.uint8 and t["yaw"].dtype == torch.float32 and t["best"].dtype == torch.int32
    for other in (again, three, ragged, t):
        _same(other, whole)
    _same(sub, {k: whole[k][farms] for k in WANT})
    _same(t0, whole, ("action_gradient",))
    _same(d1, d2)
    assert timing["total_ms"] > 0.0


def test_wind_per_step():
    """wind= equal to the held wind gives the bits of wind=None (strict); a horizon whose speed changes at h = 2 and whose
    direction turns at h = 3 agrees with the reference on every entry — all rows of step h under wind h, normalised by the
    speed of step h - 1 — and the trajectory does not see the wind."""
    name = "row3"
    c = retgrad_cases.case(name)
    H = c["H"]
    held = np.stack([np.repeat(c["ws"][:, None], H, axis=1), np.repeat(c["wd"][:, None], H, axis=1)], axis=2)
    wind = held.copy()
    wind[:, 2:, 0] *= 1.2
    wind[:, 3, 1] += 4.0
    ref = retgrad_ref.return_gradient(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["actions"], PARAMS, GAMMA, LOAD_COEF, wind=wind,
                                      delta=DELTA)
    kw = dict(gamma=GAMMA, delta=DELTA, strict=True, want=WANT)
    w = _handle(name)
    same = w.return_gradient(c["actions"], wind=held, **kw)
    got = w.return_gradient(c["actions"], wind=wind, **kw)
    w.close()
    _same(same, _device(name, True))
    _inside(got, ref, retgrad_cases.bounds(ref, parity.TOL_F64), "row3 strict, a wind per step")
    _same(got, _device(name, True), ("yaw", "final_yaw", "pass_mask"))
    assert (got["reward_gradient"][:, :, 2:] != same["reward_gradient"][:, :, 2:]).any()


def test_wind_series():
    """A handle in series mode, right after reset (t = 1: the speed of tick 0 is still pending) and after a further tick and
    env step (nothing pending): wind="series" has the bits of the same call given wind_preview's rows in every output that
    does not see the pending speed, and in ALL outputs on the farms whose pending speed equals the current one — after the
    step: on every farm.  Step 0 is normalised as the coming env step will be — by the speed the handle holds now, which that
    step's tick makes the pending one —: inside the strict bounds of the reference with wr0 = the current speed."""
    import series_cases
    import series_ref
    from test_lookahead import PARAMS as LA_PARAMS
    from test_series_gpu import _handle as series_handle

    name = "Turb3_Row1_"
    c = series_cases.plan_case(name)
    B, N, H, T, K = c["farms"], c["N"], c["H"], c["T"], 2
    params = dict(LA_PARAMS, discrete=False)
    rng = np.random.default_rng(31)
    act = rng.uniform(-6.0, 6.0, (B, K, H, N)).astype(np.float32)
    kw = dict(gamma=GAMMA, delta=DELTA, strict=True, want=WANT)
    w = series_handle(name, B, T, c["start"])
    w.env_set_state(c["state"])
    for phase in ("after reset", "after a step"):
        if phase == "after a step":
            w.wind_series_step()
            w.env_step(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32), want=("reward",))
        cur = w.series_state()
        rows, avail = w.wind_preview(H)
        want_rows = series_ref.window(c["series"], cur["start"], cur["t"], 1, H)[0]
        assert avail == H and np.array_equal(rows, want_rows)
        ws, wd = w.get_wind()
        state = w.env_get_state()
        got = w.return_gradient(act, wind="series", **kw)
        by_rows = w.return_gradient(act, wind=rows, **kw)
        pending = series_ref.window(c["series"], cur["start"], cur["t"] - 1, 0, 1)[0][:, 0, 0]
        same = (pending == ws) if cur["prev_pending"] else np.ones(B, bool)
        assert cur["prev_pending"] == (phase == "after reset")
        _same(got, by_rows, ("farm_power", "final_yaw", "yaw", "pass_mask"))
        for k in ("rewards", "reward_gradient"):
            assert np.array_equal(got[k][:, :, 1:], by_rows[k][:, :, 1:]), (phase, k)
        _same({k: got[k][same] for k in WANT}, {k: by_rows[k][same] for k in WANT})
        if phase == "after reset":
            assert same.any() and (~same).any()
            assert (got["rewards"][~same][:, :, 0] != by_rows["rewards"][~same][:, :, 0]).all()
            assert (got["reward_gradient"][~same][:, :, 0] != by_rows["reward_gradient"][~same][:, :, 0]).any()
        else:
            assert same.all()
        ref = retgrad_ref.return_gradient(c["x"], c["y"], ws, wd, state, act, params, GAMMA, series_cases.LOAD_COEF, wind=rows, wr0=ws,
                                          delta=DELTA)
        _inside(got, ref, retgrad_cases.bounds(ref, parity.TOL_F64, load_coef=series_cases.LOAD_COEF), f"series, {phase}")
        _same(got, ref, ("yaw", "final_yaw", "pass_mask"))
        sub = w.return_gradient(act[[3, 0, 4]], wind="series", farms=[3, 0, 4], max_eval_farms=K * H * (2 * N + 1), **kw)
        _same(sub, {k: got[k][[3, 0, 4]] for k in WANT})
    # the C boundary: a caller's wind next to the mode is refused (the Python keyword cannot express it)
    raw = w._retgrad()
    raw._call("set_series", 1)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind of your own"):
        raw._call("run", act.ctypes.data, K, H, rows.ctypes.data, GAMMA, DELTA, None, B, None, *([None] * 10), 0)
    held = w.return_gradient(act, **kw)  # (the handle still serves; the mode is off again: the wind it holds, held)
    w.close()
    assert np.isfinite(held["action_gradient"]).all()


def test_series_env_needs_the_keyword(tmp_path):
    """A time-series env: the default call refuses, a caller's wind next to the mode is refused by name, wind="series" serves
    and agrees with the handle's own call; an env without a series refuses the keyword."""
    from test_series_gpu import _env

    B, K, H, N = 3, 2, 2, 3
    env = _env("Turb3_Row1_Floris", B, 12, tmp_path)
    env.reset(seed=1)
    act = np.random.default_rng(1).uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="time-series"):
        env.return_gradient({"yaw": act})
    with pytest.raises(ValueError, match='None or "series"'):
        env.return_gradient({"yaw": act}, wind=np.zeros((B, H, 2)))
    r = env.return_gradient({"yaw": act}, gamma=GAMMA, strict=True, wind="series")
    direct = env.fi.return_gradient(act, gamma=GAMMA, strict=True, wind="series", want=tuple(r))
    _same(r, direct, tuple(r))
    env.close()


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    N = 3
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.return_gradient(np.zeros((2, 2, 2, N), np.float32))
    w.close()
    w = WfStep(x, y, env_batch=2)
    zero = np.zeros((2, 2, 2, N), np.float32)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.return_gradient(zero)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.return_gradient(zero)
    w.env_config(discrete=True)
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*discrete encoding"):
        w.return_gradient(zero)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
        w.return_gradient(np.zeros((2, 1, 65, N), np.float32))
    with pytest.raises(ValueError, match=r"WF_E_INVALID.*max_eval_farms must hold one farm's rows: at least K H \(2 N \+ 1\)"):
        w.return_gradient(zero, max_eval_farms=27)  # K H (2 N + 1) = 28
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.return_gradient(np.zeros((2, 157, 60, N), np.float32))  # 65 940 rows > the default 65 536
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*delta"):
            w.return_gradient(zero, delta=delta)
    for gamma in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.return_gradient(zero, gamma=gamma)
    with pytest.raises(ValueError, match="farm index out of range"):
        w.return_gradient(zero, farms=[0, 2])
    with pytest.raises(ValueError, match=r"\(n_farms, K, H, num_turbines\)"):
        w.return_gradient(zero[:1])
    with pytest.raises(ValueError, match=r"\(n_farms, H, 2\)"):
        w.return_gradient(zero, wind=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match=r"\(n_farms, K, num_turbines\)"):
        w.return_gradient(zero, terminal=np.zeros((2, 2, N + 1)))
    with pytest.raises(ValueError, match="want must name"):
        w.return_gradient(zero, want=("gradient",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.return_gradient_timing()
    with pytest.raises(ValueError, match="WF_E_INVALID.*parent in series mode"):
        w.return_gradient(zero, wind="series")
    up = zero.copy()
    up[:, 1] = 5.0
    r = w.return_gradient(up[:1], farms=[1], max_eval_farms=28, want=WANT)  # (the handle still serves)
    assert r["returns"].shape == (1, 2) and np.isfinite(r["action_gradient"]).all()
    # from the reset state: the first 5 deg pass, and fill the budget (5 / 0.3 / 2 / 60 = 0.14 >= 0.1): the second step is gated
    assert r["final_yaw"][0, 1].tolist() == [5.0] * N and r["pass_mask"][0, 1].tolist() == [[3] * N, [2] * N]
    assert (r["pass_mask"][0, 0] == 3).all() and (r["action_gradient"][0, 1, 1] == 0.0).all()
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_vec_env_and_autograd():
    """VecWindFarmEnv.return_gradient after reset(seed=0) and two steps: shapes and dtypes, agreement with
    WfStep.return_gradient on the same state, and the env left as it was.  autograd.differentiable_return on the env's
    handle: (B, K) float64 returns with those bits, and actions.grad under returns.sum().backward() is action_gradient cast
    to float32 — from the forward's one run; a weighted sum scales every sequence's block."""
    import torch
    from wfcrl_env_amd import autograd
    from wfcrl_env_amd import environments as envs

    B, Kv, Hv = 4, 3, 3
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    N = env.num_turbines
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        env.step({"yaw": (torch.rand((B, N), generator=gen) * 10.0 - 5.0).cuda()})
    seqs = (torch.rand((B, Kv, Hv, N), generator=gen) * 8.0 - 4.0).cuda()
    before = env.get_state()
    r = env.return_gradient({"yaw": seqs}, gamma=0.95)
    keys = {"returns", "rewards", "action_gradient", "reward_gradient", "state_gradient", "yaw", "pass_mask"}
    assert set(r) == keys and all(v.is_cuda for v in r.values())
    dims = dict(B=B, K=Kv, H=Hv, N=N)
    for k in keys:
        assert tuple(r[k].shape) == tuple(dims[d] for d in SHAPES[k]) and r[k].dtype == getattr(torch, np.dtype(DTYPES[k]).name), k
    direct = env.fi.return_gradient(seqs, gamma=0.95, want=tuple(keys))
    for k in keys:
        assert torch.equal(r[k], direct[k]), k
    strict = env.return_gradient(seqs, gamma=0.95, strict=True)
    sub = env.return_gradient(seqs, gamma=0.95, farms=[3, 1], strict=True)
    for k in sub:
        assert torch.equal(sub[k], strict[k][[3, 1]]), k
    runs = []
    orig = env.fi._retgrad().run
    env.fi._retgrad().run = lambda *a, **kw: runs.append(1) or orig(*a, **kw)
    a = seqs.clone().requires_grad_(True)
    ret = autograd.differentiable_return(env.fi, a, gamma=0.95)
    assert tuple(ret.shape) == (B, Kv) and ret.dtype == torch.float64 and torch.equal(ret.detach(), r["returns"])
    ret.sum().backward()
    assert a.grad.dtype == torch.float32 and torch.equal(a.grad, r["action_gradient"].to(torch.float32))
    a2 = seqs.clone().requires_grad_(True)
    wgt = torch.arange(1, B * Kv + 1, dtype=torch.float64, device="cuda").reshape(B, Kv)
    (autograd.differentiable_return(env.fi, a2, gamma=0.95) * wgt).sum().backward()
    assert torch.equal(a2.grad, (wgt[..., None, None] * r["action_gradient"]).to(torch.float32))
    assert len(runs) == 2  # (one extension run per forward, none in backward)
    del env.fi._retgrad().run
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        autograd.differentiable_return(env.fi, seqs.double())
    after = env.get_state()
    for k in before:
        x, y = before[k], after[k]
        assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), k
    with pytest.raises(ValueError, match=r"\(num_envs, K, H, num_turbines\)"):
        env.return_gradient(seqs[:, 0])
    env.close()


def test_kernel_info_shows_no_scratch():
    w = _handle("row3", state=False)
    info = w.return_gradient_kernel_info()
    w.close()
    assert set(info) == {"layout", "reduce", "best"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
