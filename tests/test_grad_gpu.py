"""GPU: yaw sensitivities on the device (include/wfgrad.h) against tests/grad_ref.py — the same difference quotients in NumPy
over the float64 oracle.

The bounds need no measured number.  The step's contract is per turbine: |P_dev - P_ref| <= tol max(P_ref, 1 kW), with
tol = parity.TOL_F64["power"] when every row is solved in float64 (strict) and parity.TOL["power"] in the handle's default
mode.  The divisor d_i is the same float64 number on either side (the same float32 yaws), so

    |J_dev - J_ref|[i][j] <= tol (max(P+_j, 1e3) + max(P-_j, 1e3)) / d_i
    |G_dev - G_ref|[i]    <= sum_j |c_j| x that bound

hold on EVERY entry; nothing is exempted.  Inputs: the row of three under four winds and 32 farms of three layouts
(yawopt_ref.gpu_case, seed 40); yaw drawn once (seed 41), float32, uniform in [-20, 20], farm 0 at zeros and farm 1 at hi
everywhere, bounds (-25, 25): farm 1 exercises the clipped, one-sided branch.

Bit identity across chunk sizes, farm lists and evaluators is asserted in STRICT mode, where every row is solved by the
float64 kernel, whose bits do not depend on the batch (level stages, helper waves).  In the default mode an
evaluator of another batch size may pick another float32 kernel family (tests/test_yawopt_gpu.py: test_chunking), so there
only two runs on the same evaluator are compared."""
import functools

import numpy as np
import pytest

import grad_ref
import parity
import yawopt_ref
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

BOUNDS = (-25.0, 25.0)
NAMES = ("row3", "Ablaincourt_", "Turb6_Row2_", "Turb16_Row5_")


@functools.lru_cache(maxsize=None)
def _case(name):
    """An input with its reference, computed once for the tests that share them: x, y, ws, wd, yaw, a random cotangent, the
    reference at c = 1 and the reference gradient at the random c."""
    x, y, ws, wd = yawopt_ref.gpu_input(name)
    B, N = len(ws), len(x)
    rng = np.random.default_rng(41)
    yaw = rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32)
    yaw[0], yaw[1] = 0.0, BOUNDS[1]
    c = rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32)
    ref = grad_ref.gradient(x, y, ws, wd, yaw, bounds=BOUNDS)
    assert (ref["d"][1] == 1.0).all() and (ref["d"][0] == 2.0).all()  # farm 1: one-sided
    g_c = grad_ref.vjp(ref["p_plus"], ref["p_minus"], ref["d"], c)
    for v in (yaw, c, g_c, *ref.values()):
        v.setflags(write=False)
    return x, y, ws, wd, yaw, c, ref, g_c


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    """The device's answer at c = 1 (with the Jacobian) and at the random c, from one handle."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, yaw, c, _, _ = _case(name)
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    one = w.yaw_gradient(yaw, bounds=BOUNDS, strict=strict, jacobian=True)
    rnd = w.yaw_gradient(yaw, c, bounds=BOUNDS, strict=strict, jacobian=True)
    w.close()
    return one, rnd


def _check(name, strict, tol, ptol):
    x, y, ws, wd, yaw, c, ref, g_c = _case(name)
    one, rnd = _device(name, strict)
    B, N = yaw.shape
    assert one["power"].shape == (B, N) and one["power"].dtype == np.float32
    assert one["gradient"].shape == (B, N) and one["gradient"].dtype == np.float64 and one["jacobian"].shape == (B, N, N)
    d = ref["d"]
    jb = tol * (np.maximum(ref["p_plus"], 1e3) + np.maximum(ref["p_minus"], 1e3)) / d[:, :, None]  # [b, i, j]
    label = f"{name} {'strict' if strict else 'default mode'}"
    worst = {}
    for tag, got, cc, g_ref in (("c = 1", one, np.ones((B, N)), ref["gradient"]), ("random c", rnd, c.astype(np.float64), g_c)):
        ej = np.abs(got["jacobian"] - ref["jacobian"])
        gb = (np.abs(cc)[:, None, :] * jb).sum(axis=2)
        eg = np.abs(got["gradient"] - g_ref)
        ep = np.abs(got["power"].astype(np.float64) - ref["power"]) / np.maximum(ref["power"], 1e3)
        worst[tag] = ((ej / jb).max(), (eg / gb).max(), ep.max())
        print(f"{label}, {tag}: largest error / bound: Jacobian {worst[tag][0]:.3f}, gradient {worst[tag][1]:.3f}; power {ep.max():.2e} (tol {ptol:g})")
    for tag, got, g_ref in (("c = 1", one, ref["gradient"]), ("random c", rnd, g_c)):
        cc = np.ones((B, N)) if tag == "c = 1" else c.astype(np.float64)
        assert (np.abs(got["jacobian"] - ref["jacobian"]) <= jb).all(), (label, tag, worst[tag])
        assert (np.abs(got["gradient"] - g_ref) <= (np.abs(cc)[:, None, :] * jb).sum(axis=2)).all(), (label, tag, worst[tag])
        assert worst[tag][2] <= ptol, (label, tag, worst[tag])
    assert np.array_equal(one["jacobian"], rnd["jacobian"]) and np.array_equal(one["power"], rnd["power"])  # c plays no part in them
    assert (one["gradient"] != rnd["gradient"]).any()


@pytest.mark.parametrize("name", NAMES)
def test_strict_against_the_reference(name):
    """Every row solved in float64: every entry of J and G inside the bound that follows from TOL_F64, with c = 1 and with
    a random c; the forward power inside TOL_F64 itself."""
    _check(name, True, parity.TOL_F64["power"], parity.TOL_F64["power"])


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_against_the_reference(name):
    """The handle's own resolve mode: the same inequalities with the project's 1e-4."""
    _check(name, False, parity.TOL["power"], parity.TOL["power"])


def test_same_bits():
    """Two runs; max_eval_farms = 3 R (32 farms in chunks of 3 and a ragged 2); a shuffled sub-list of farms; torch tensors in
    and out: all the bits of the whole NumPy run (strict: see the module docstring).  Two default-mode runs on one evaluator
    agree bit for bit as well.  yaw=None is zero yaw, cotangent=None is ones."""
    import torch
    from wfcrl_env_amd.backend import WfStep

    name = "Ablaincourt_"
    x, y, ws, wd, yaw, c, _, _ = _case(name)
    B, N = yaw.shape
    R = 2 * N + 1
    whole = _device(name, True)[1]
    kw = dict(bounds=BOUNDS, strict=True, jacobian=True)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    again = w.yaw_gradient(yaw, c, **kw)
    chunks = w.yaw_gradient(yaw, c, max_eval_farms=3 * R, **kw)
    farms = np.random.default_rng(5).permutation(B)[:13]
    sub = w.yaw_gradient(yaw[farms], c[farms], farms=farms, **kw)
    t = w.yaw_gradient(torch.from_numpy(yaw.copy()).cuda(), torch.from_numpy(c.copy()).cuda(), **kw)
    out = {"power": torch.empty((B, N), dtype=torch.float32, device="cuda"), "gradient": torch.empty((B, N), dtype=torch.float64, device="cuda")}
    t0 = w.yaw_gradient(None, None, bounds=BOUNDS, strict=True, out=out)
    z = w.yaw_gradient(np.zeros((B, N), np.float32), np.ones((B, N), np.float32), bounds=BOUNDS, strict=True)
    d1, d2 = w.yaw_gradient(yaw, c, bounds=BOUNDS, jacobian=True), w.yaw_gradient(yaw, c, bounds=BOUNDS, jacobian=True)
    w.close()
    assert all(v.is_cuda for v in t.values()) and t0["gradient"] is out["gradient"] and "jacobian" not in t0
    for k in ("power", "gradient", "jacobian"):
        assert np.array_equal(again[k], whole[k]), k
        assert np.array_equal(chunks[k], whole[k]), k
        assert np.array_equal(sub[k], whole[k][farms]), k
        assert np.array_equal(t[k].cpu().numpy(), whole[k]), k
        assert np.array_equal(d1[k], d2[k]), k
    for k in ("power", "gradient"):
        assert np.array_equal(t0[k].cpu().numpy(), z[k]), k
    assert (z["gradient"] != 0.0).any()


@pytest.mark.parametrize("name", ["row3", "Turb16_Row5_"])
def test_gradient_is_the_jacobian_contracted(name):
    """The device's G against sum_j c_j J[i][j] recomputed in NumPy from the device's own J, within 1e-12 sum_j |c_j J[i][j]|
    (the device divides the sum once, NumPy every term: a few ulps per term).  On the row of three, strict: a turbine's yaw
    does not reach upwind — J[i][j] == 0.0 exactly for every j upstream of i under 270 and 268 deg, mirrored under 90 deg
    (in strict mode both perturbed rows are solved by the same float64 kernel and an upstream turbine sees the same inputs in
    both; the default mode may re-solve only one of the two rows in float64, so the zeros are asserted in strict mode)."""
    x, y, ws, wd, yaw, c, _, _ = _case(name)
    for strict in (True, False):
        one, rnd = _device(name, strict)
        for got, cc in ((one, np.ones(yaw.shape)), (rnd, c.astype(np.float64))):
            terms = cc[:, None, :] * got["jacobian"]
            err = np.abs(got["gradient"] - terms.sum(axis=2))
            assert (err <= 1e-12 * np.abs(terms).sum(axis=2)).all(), (name, strict, err.max())
    if name == "row3":
        J = _device(name, True)[0]["jacobian"]
        lower, upper = np.tril_indices(3, -1), np.triu_indices(3, 1)
        for b in (0, 1):
            assert (J[b][lower] == 0.0).all() and (J[b][upper] != 0.0).all(), b
        assert (np.diag(J[1]) != 0.0).all()  # (farm 0 sits at zero yaw, where P_i is even in yaw_i: its diagonal is ~ 0)
        assert (J[2][upper] == 0.0).all() and (J[2][np.tril_indices(3)] != 0.0).all()


def test_autograd():
    """differentiable_power: forward is w.step bit for bit; .sum().backward() leaves float32(G) in yaw.grad bit for bit, a
    weighted loss (power * c).sum() the float32 of the VJP with that c."""
    import torch
    from wfcrl_env_amd.autograd import differentiable_power
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, yaw, c, _, _ = _case("Ablaincourt_")
    yaw = np.clip(yaw, -20.0, 20.0)  # (default bounds (-45, 45): farm 1 is not special here)
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    ty = torch.from_numpy(yaw).cuda().requires_grad_(True)
    p = differentiable_power(w, ty)
    assert p.shape == ty.shape and p.dtype == torch.float32 and p.requires_grad
    assert torch.equal(p.detach(), w.step(ty.detach())["power"])
    p.sum().backward()
    g1 = w.yaw_gradient(yaw)
    assert ty.grad.dtype == torch.float32 and np.array_equal(ty.grad.cpu().numpy(), g1["gradient"].astype(np.float32))
    assert np.array_equal(p.detach().cpu().numpy(), g1["power"])
    ty.grad = None
    tc = torch.from_numpy(c.copy()).cuda()
    (differentiable_power(w, ty) * tc).sum().backward()
    gc = w.yaw_gradient(yaw, c)
    assert np.array_equal(ty.grad.cpu().numpy(), gc["gradient"].astype(np.float32))
    assert (gc["gradient"] != g1["gradient"]).any() and (ty.grad != 0).any()
    # a few steps of a torch optimiser run through it
    ty = torch.zeros_like(ty).requires_grad_(True)
    opt = torch.optim.SGD([ty], lr=1e-4)
    p0 = float(differentiable_power(w, ty).detach().sum())
    for _ in range(3):
        opt.zero_grad()
        (-differentiable_power(w, ty).sum()).backward()
        opt.step()
        with torch.no_grad():
            ty.clamp_(-25.0, 25.0)
    assert float(differentiable_power(w, ty).detach().sum()) > p0
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        differentiable_power(w, yaw)
    w.close()


def test_env_power_gradient_reads_the_state_and_leaves_it():
    import torch
    from wfcrl_env_amd import environments as envs

    B = 8
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    env.reset(seed=5)
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        env.step({"yaw": (torch.rand((B, env.num_turbines), generator=gen) * 10.0 - 5.0).cuda()})
    before = env.get_state()
    got = env.power_gradient()
    lo, hi = env.controls["yaw"][0], env.controls["yaw"][1]
    yaw = env.fi.env_get_state(as_torch=True)["yaw"]
    assert bool((yaw != 0).any())
    want = env.fi.yaw_gradient(yaw, bounds=(lo, hi))
    assert got["gradient"].is_cuda and tuple(got["gradient"].shape) == (B, env.num_turbines)
    assert torch.equal(got["gradient"], want["gradient"]) and torch.equal(got["power"], want["power"])
    c = torch.zeros((B, env.num_turbines))
    c[:, 3] = 1.0  # turbine 3's credit
    sub = env.power_gradient(cotangent=c[[5, 2]], farms=[5, 2], strict=True)
    full = env.fi.yaw_gradient(yaw, c.cuda(), bounds=(lo, hi), strict=True, jacobian=True)
    assert torch.equal(sub["gradient"], full["gradient"][[5, 2]]) and torch.equal(sub["gradient"], full["jacobian"][[5, 2], :, 3])
    after = env.get_state()
    assert before.keys() == after.keys()
    for k in before:
        a, b = before[k], after[k]
        assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), k
    env.close()


def test_interface_single_farm():
    from wfcrl_env_amd.backend import WfStep
    from wfcrl_env_amd.interface import HipFlorisInterface

    x, y = ROW3
    fi = HipFlorisInterface(3, list(x), list(y))
    fi.init(wind_speed=8.0, wind_direction=270.0)
    r = fi.yaw_gradient(yaw=[5.0, -7.0, 3.0], strict=True, jacobian=True)
    assert r["gradient"].shape == (3,) and r["jacobian"].shape == (3, 3) and r["power"].shape == (3,)
    w = WfStep(x, y, env_batch=1)
    w.set_wind(8.0, 270.0)
    ref = w.yaw_gradient(np.float32([[5.0, -7.0, 3.0]]), strict=True, jacobian=True)
    w.close()
    for k in r:
        assert np.array_equal(r[k], ref[k][0].astype(np.float64)), k
    assert r["gradient"][0] > 0.0  # steering the first turbine of the row pays


def test_refusals_name_their_cause():
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.yaw_gradient()
    w.close()
    w = WfStep(x, y, env_batch=2, model=dict(turbine_defs=[{}, {"tsr": 7.0}], turbine_type_of=[0, 1, 0]))  # two definitions
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.yaw_gradient()
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.yaw_gradient()
    w.set_wind(8.0, 270.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*step h"):
            w.yaw_gradient(step=bad)
    for bad in ((10.0, 10.0), (5.0, -5.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="WF_E_INVALID.*lo < hi"):
            w.yaw_gradient(bounds=bad)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.yaw_gradient(max_eval_farms=6)  # R = 7
    with pytest.raises(ValueError, match="farm index out of range"):
        w.yaw_gradient(farms=[0, 2])
    with pytest.raises(ValueError, match="a row per listed farm"):
        w.yaw_gradient(np.zeros((1, 3), np.float32))
    r = w.yaw_gradient(farms=[1], max_eval_farms=7)  # (the handle still serves after refusals)
    assert r["gradient"].shape == (1, 3) and np.isfinite(r["gradient"]).all()
    assert w.step(np.zeros((2, 3), np.float32))["power"].shape == (2, 3)
    info = w.grad_kernel_info()
    assert set(info) == {"layout", "reduce"} and all(v["scratch_bytes"] == 0 for v in info.values())
    t = w.grad_timing()
    assert t["total_ms"] > 0.0
    w.close()
