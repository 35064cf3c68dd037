"""GPU: expected power under wind-direction uncertainty and the robust yaw search on the device (include/wfrobust.h) against
tests/robust_ref.py — the same definition in NumPy over the float64 oracle.

Decisions are compared by the method of tests/test_yawopt_gpu.py: yaw angles on the farms whose smallest reference margin is
>= 1e-5 (MARGIN), at most 10 % of a test's farms below it, powers on EVERY farm against the oracle evaluated at the yaw the
device returned.  Margins are much tighter under uncertainty than without it, so the inputs are the ones checked on the CPU
with the oracle against that cap: members (-6, -3, 0, 3, 6) deg with weights exp(-d^2 / 18), 32 farms of yawopt_ref.gpu_case
(seed 40), and per layout the passes named in CASES (farms below the margin, FIXED / RELATIVE: row of three 0 / 0, Ablaincourt
2 / 3, Turb6_Row2 1 / 2, Turb16_Row5 with passes (5,) 1 / 1; Turb16_Row5 with (5, 4) has 9 and 13: not used)."""
import functools
import json
import os

import numpy as np
import pytest

import robust_ref
import yawopt_ref
from yawopt_ref import ROW3
from conftest import ROOT

pytestmark = pytest.mark.gpu

MARGIN = 1e-5   # smallest reference margin at which a farm's yaw is compared
YAW_TOL = 1e-4  # degrees
POW_TOL = 2e-6  # relative; the strict kernels are held to 5e-7 per turbine in tests/test_resolve_gpu.py
CASES = {"row3": (5, 4), "Ablaincourt_": (5, 4), "Turb6_Row2_": (5, 2), "Turb16_Row5_": (5,)}
FRAMES = ("fixed", "relative")
DELTA, W = robust_ref.members(*robust_ref.MEMBERS5)


def _unc(frame, delta=robust_ref.MEMBERS5[0], weight=robust_ref.MEMBERS5[1]):
    return dict(delta=delta, weight=weight, frame=frame)


@functools.lru_cache(maxsize=None)
def _case(name, frame):
    """An input of CASES with the reference and the device's strict run, computed once for the tests that share them."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd = yawopt_ref.gpu_input(name)
    ref = robust_ref.optimize(x, y, ws, wd, DELTA, W, frame, passes=CASES[name])
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    strict = w.optimize_yaw(strict=True, passes=CASES[name], wd_uncertainty=_unc(frame))
    w.close()
    return x, y, ws, wd, ref, strict


def _check_against_reference(x, y, ws, wd, got, ref, frame, label, members=(DELTA, W)):
    """The comparison of the strict tests; returns the farms whose yaw was compared."""
    safe = ref["margin"] >= MARGIN
    n = len(safe)
    print(f"{label}: {n - safe.sum()} of {n} farms below margin {MARGIN:g} (smallest {ref['margin'].min():.2e})")
    assert (~safe).sum() <= 0.1 * n, (label, ref["margin"])
    dy = np.abs(got["yaw"].astype(np.float64) - ref["yaw"].astype(np.float64)).max(axis=1)
    at_yaw = robust_ref.expected_power(x, y, ws, wd, got["yaw"], members[0], members[1], frame)[0]
    e_pow = np.abs(got["power"] / at_yaw - 1.0)
    e_init = np.abs(got["power_initial"] / ref["power_initial"] - 1.0)
    e_ref = np.abs(got["power"][safe] / ref["power"][safe] - 1.0)
    print(f"{label}: yaw diff (compared farms) {dy[safe].max():.2e} deg, E vs oracle at the device's yaw {e_pow.max():.2e}, "
          f"power_initial {e_init.max():.2e}, E vs reference (compared farms) {e_ref.max():.2e}")
    assert dy[safe].max() <= YAW_TOL, (label, np.where(safe & (dy > YAW_TOL))[0])
    assert e_pow.max() <= POW_TOL and e_init.max() <= POW_TOL and e_ref.max() <= POW_TOL, label
    assert (got["power"] >= got["power_initial"]).all()
    return safe


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", list(CASES))
def test_strict_search(name, frame):
    x, y, ws, wd, ref, strict = _case(name, frame)
    assert strict["yaw"].shape == (len(ws), len(x)) and strict["power"].shape == (len(ws),)
    safe = _check_against_reference(x, y, ws, wd, strict, ref, frame, f"{name} {frame}")
    assert (strict["yaw"][safe] != 0.0).any()
    if name == "row3":
        assert ref["margin"].min() >= MARGIN  # (all four farms are compared)


@pytest.mark.parametrize("frame", FRAMES)
def test_robust_optimum_differs_from_the_nominal_one_and_is_worth_more(frame):
    """The row of three: under uncertainty the search steers less than optimize_yaw() does for the sharp direction, and when
    both are scored by uncertain_power the robust optimum has the larger expected power."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, ref, strict = _case("row3", frame)
    w = WfStep(x, y, env_batch=4)
    w.set_wind(ws, wd)
    nominal = w.optimize_yaw(strict=True)
    e_nom = w.uncertain_power(nominal["yaw"], wd_uncertainty=_unc(frame), strict=True)["expected_power"]
    e_rob = w.uncertain_power(strict["yaw"], wd_uncertainty=_unc(frame), strict=True)["expected_power"]
    w.close()
    along = slice(0, 3)  # (the fourth wind blows across the row: nothing to steer, both searches stay at zero)
    assert (nominal["yaw"][along] != strict["yaw"][along]).any(axis=1).all()
    assert (e_rob[along] > e_nom[along]).all() and e_rob[3] == e_nom[3]
    assert np.abs(e_rob / strict["power"] - 1.0).max() <= POW_TOL
    print(f"{frame}: expected power of the nominal optimum is {np.max(1.0 - e_nom[along] / e_rob[along]):.3%} (largest) below the robust one")
    if frame == "fixed":
        assert np.array_equal(nominal["yaw"][0], np.float32([25.0, 25.0, 0.0])) and np.array_equal(strict["yaw"][0], np.float32([22.5, 22.5, 0.0]))


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["row3", "Ablaincourt_"])
def test_uncertain_power(name, frame):
    """Random yaw within +-20 deg.  Strict: E, the per-turbine expectation and every member power within 2e-6 of the
    reference; the handle's default mode within the project's 1e-4; yaw=None is zero yaw; two calls give the same bits."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd = yawopt_ref.gpu_input(name)
    B, N = len(ws), len(x)
    yaw = np.random.default_rng(7).uniform(-20.0, 20.0, (B, N)).astype(np.float32)
    E, pm, Et = robust_ref.expected_power(x, y, ws, wd, yaw, DELTA, W, frame)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    got = w.uncertain_power(yaw, wd_uncertainty=_unc(frame), strict=True)
    again = w.uncertain_power(yaw, wd_uncertainty=_unc(frame), strict=True)
    default = w.uncertain_power(yaw, wd_uncertainty=_unc(frame))
    zero = w.uncertain_power(None, wd_uncertainty=_unc(frame), strict=True)
    zero2 = w.uncertain_power(np.zeros((B, N), np.float32), wd_uncertainty=_unc(frame), strict=True)
    w.close()
    assert got["expected_power"].shape == (B,) and got["turbine_expected_power"].shape == (B, N) and got["member_power"].shape == (B, 5)
    assert got["expected_power"].dtype == np.float64 and got["member_power"].dtype == np.float32
    assert np.array_equal(got["delta"], DELTA) and np.array_equal(got["weight"], W)
    ref = {"expected_power": E, "turbine_expected_power": Et, "member_power": pm}
    for k, r in ref.items():
        e_s, e_d = np.abs(got[k] / r - 1.0).max(), np.abs(default[k] / r - 1.0).max()
        print(f"{name} {frame} {k}: strict {e_s:.2e}, default mode {e_d:.2e}")
        assert e_s <= POW_TOL, k
        assert e_d <= 1e-4, k
        assert np.array_equal(got[k], again[k]), k
        assert np.array_equal(zero[k], zero2[k]), k
    E0 = robust_ref.expected_power(x, y, ws, wd, np.zeros((B, N), np.float32), DELTA, W, frame)[0]
    assert np.abs(zero["expected_power"] / E0 - 1.0).max() <= POW_TOL


def test_one_member_is_the_nominal_search():
    """M = 1 with delta 0, strict: the yaw of optimize_yaw(strict=True) on the farms whose decisions are safe, its powers
    within 2e-6; uncertain_power within 2e-6 of `step` (every farm solved in float64) summed in float64."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd = yawopt_ref.gpu_input("Ablaincourt_")
    nom_ref = yawopt_ref.optimize(x, y, ws, wd)
    safe = nom_ref["margin"] >= MARGIN
    assert (~safe).sum() <= 0.1 * len(safe)
    one = dict(delta=[0.0], weight=[2.0])
    w = WfStep(x, y, env_batch=len(ws))
    w.set_risk_resolve(2)
    w.set_wind(ws, wd)
    nominal = w.optimize_yaw(strict=True)
    for frame in FRAMES:
        got = w.optimize_yaw(strict=True, wd_uncertainty=dict(one, frame=frame))
        assert np.array_equal(got["yaw"][safe], nominal["yaw"][safe]), frame
        assert np.abs(got["power"] / nominal["power"] - 1.0).max() <= POW_TOL
        assert np.abs(got["power_initial"] / nominal["power_initial"] - 1.0).max() <= POW_TOL
        _check_against_reference(x, y, ws, wd, got, nom_ref, frame, f"one member, {frame}", robust_ref.members([0.0], [2.0]))
        yaw = np.random.default_rng(11).uniform(-20.0, 20.0, nominal["yaw"].shape).astype(np.float32)
        pw = w.step(yaw)["power"].astype(np.float64)
        s = np.zeros(len(ws))
        for t in range(len(x)):
            s = s + pw[:, t]
        u = w.uncertain_power(yaw, wd_uncertainty=dict(one, frame=frame), strict=True)
        assert u["member_power"].shape == (len(ws), 1) and np.array_equal(u["weight"], [1.0])
        assert np.abs(u["expected_power"] / s - 1.0).max() <= POW_TOL
        assert np.abs(u["turbine_expected_power"] / pw - 1.0).max() <= POW_TOL
    w.close()


def test_chunking():
    """max_eval_farms = 390 holds 13 farms x 6 rows x 5 members: the 32 farms run as chunks of 13, 13 and a ragged 6.  Strict
    mode: the yaw of the unchunked run on the farms whose decisions are safe, powers within 2e-6 on every farm — not bit
    identity: the evaluator's batch size may pick another kernel family.  uncertain_power in chunks of 7 farms likewise."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, ref, strict = _case("Ablaincourt_", "fixed")
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    got = w.optimize_yaw(strict=True, max_eval_farms=390, wd_uncertainty=_unc("fixed"))
    whole = w.uncertain_power(strict["yaw"], wd_uncertainty=_unc("fixed"), strict=True)
    parts = w.uncertain_power(strict["yaw"], wd_uncertainty=_unc("fixed"), strict=True, max_eval_farms=35)
    w.close()
    safe = ref["margin"] >= MARGIN
    assert np.array_equal(got["yaw"][safe], strict["yaw"][safe])
    assert np.abs(got["power"] / strict["power"] - 1.0).max() <= POW_TOL
    assert np.abs(got["power_initial"] / strict["power_initial"] - 1.0).max() <= POW_TOL
    _check_against_reference(x, y, ws, wd, got, ref, "fixed", "chunked")
    for k in ("expected_power", "turbine_expected_power", "member_power"):
        assert np.abs(parts[k] / whole[k] - 1.0).max() <= POW_TOL, k
    assert np.abs(whole["expected_power"] / strict["power"] - 1.0).max() <= POW_TOL


@pytest.mark.parametrize("frame", FRAMES)
def test_farm_subset_start_bounds_and_torch(frame):
    """48 farms of the row of three (winds and starts from seed 100, every other farm within 15 deg of the row), a shuffled
    30 of them, a non-zero start per listed farm with entries outside the bounds (0, 25), passes (3,).  Every returned angle
    lies in the bounds or is a start value that was outside them (an incumbent is never clipped); E is what the oracle
    computes at the returned yaw.  The torch path (tensors in, tensors out, nothing waited for) returns the NumPy path's bits."""
    import torch
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    rng = np.random.default_rng(100)
    B = 48
    ws, wd = rng.uniform(6.0, 10.5, B), rng.uniform(0.0, 360.0, B)
    yaw0 = rng.uniform(-10.0, 30.0, (B, 3)).astype(np.float32)
    wd = np.where(np.arange(B) % 2 == 0, rng.uniform(255.0, 285.0, B), wd)
    farms = rng.permutation(B)[:30]
    y0 = yaw0[farms]
    assert ((y0 < 0.0) | (y0 > 25.0)).any() and (y0 != 0.0).all()
    kw = dict(farms=farms, bounds=(0.0, 25.0), passes=(3,), strict=True, wd_uncertainty=_unc(frame))
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    got = w.optimize_yaw(y0, **kw)
    assert got["yaw"].shape == (30, 3)
    inside = (got["yaw"] >= 0.0) & (got["yaw"] <= 25.0)
    assert (inside | (got["yaw"] == y0)).all()
    assert (~inside).any() and (got["yaw"] != y0).any()  # an outside start that survived; and the search did move something
    at_yaw = robust_ref.expected_power(x, y, ws[farms], wd[farms], got["yaw"], DELTA, W, frame)[0]
    at_start = robust_ref.expected_power(x, y, ws[farms], wd[farms], y0, DELTA, W, frame)[0]
    assert np.abs(got["power"] / at_yaw - 1.0).max() <= POW_TOL and np.abs(got["power_initial"] / at_start - 1.0).max() <= POW_TOL
    assert (got["power"] >= got["power_initial"]).all()
    t = w.optimize_yaw(torch.from_numpy(y0).cuda(), **kw)
    assert all(v.is_cuda for v in t.values())
    for k in got:
        assert np.array_equal(t[k].cpu().numpy(), got[k]), k
    u = w.uncertain_power(got["yaw"], farms=farms, wd_uncertainty=_unc(frame), strict=True)
    tu = w.uncertain_power(t["yaw"], farms=farms, wd_uncertainty=_unc(frame), strict=True)
    for k in ("expected_power", "turbine_expected_power", "member_power"):
        assert tu[k].is_cuda and np.array_equal(tu[k].cpu().numpy(), u[k]), k
    assert np.abs(u["expected_power"] / at_yaw - 1.0).max() <= POW_TOL
    w.close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("n", [1, 2])
def test_smallest_farms(n, frame):
    """One turbine and two turbines 5 D apart under three winds: one visit per pass, a yaw block shorter than a wave.  One
    turbine is not trivial in the FIXED frame — the members meet the rotor at yaw + delta — but a symmetric member set leaves
    zero yaw optimal: it stays there."""
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3[0][:n], ROW3[1][:n]
    ws, wd = np.array([8.0, 9.0, 7.0]), np.array([270.0, 262.0, 90.0])
    ref = robust_ref.optimize(x, y, ws, wd, DELTA, W, frame)
    assert ref["margin"].min() >= MARGIN
    w = WfStep(x, y, env_batch=3)
    w.set_wind(ws, wd)
    got = w.optimize_yaw(strict=True, wd_uncertainty=_unc(frame))
    one = w.optimize_yaw(strict=True, farms=[2], wd_uncertainty=_unc(frame))
    w.close()
    safe = ref["margin"] >= MARGIN
    dy = np.abs(got["yaw"].astype(np.float64) - ref["yaw"].astype(np.float64)).max(axis=1)
    assert dy[safe].max() <= YAW_TOL
    at_yaw = robust_ref.expected_power(x, y, ws, wd, got["yaw"], DELTA, W, frame)[0]
    assert np.abs(got["power"] / at_yaw - 1.0).max() <= POW_TOL
    assert np.abs(got["power_initial"] / ref["power_initial"] - 1.0).max() <= POW_TOL
    assert np.array_equal(one["yaw"][0], got["yaw"][2])
    if n == 1:
        assert (got["yaw"] == 0.0).all() and (got["power"] == got["power_initial"]).all()
    else:
        assert got["yaw"][0, 0] != 0.0 and got["yaw"][0, 1] == 0.0 and got["yaw"][2, 1] != 0.0 and got["yaw"][2, 0] == 0.0


def test_largest_block():
    """HornsRev1 (80 turbines) x 2 farms, one pass of 31 candidates, 9 members, the handle's default mode: a slot's power block
    is 32 x 9 x 80 floats = 92 KB, more than a workgroup's LDS — the row sums have their own pass, whatever the size.  E never
    decreases, and the reported E is what the oracle computes at the returned yaw within the project's 1e-4."""
    from wfcrl_env_amd.backend import WfStep, wd_uncertainty_members

    l = yawopt_ref.layouts()["HornsRev1_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    ws, wd = np.array([8.0, 9.5]), np.array([270.0, 222.0])
    spec = dict(std=3.0, resolution=1.5, cutoff=0.975)  # bound = ceil(1.96 x 2) = 4: nine members, -6 .. 6 deg
    delta, weight, frame = wd_uncertainty_members(spec)
    assert delta.size == 9 and frame == "fixed"
    w = WfStep(x, y, env_batch=2)
    w.set_wind(ws, wd)
    got = w.optimize_yaw(passes=(31,), wd_uncertainty=spec)
    w.close()
    assert got["yaw"].shape == (2, 80) and (np.abs(got["yaw"]) <= 25.0).all() and (got["yaw"] != 0.0).any(axis=1).all()
    assert (got["power"] >= got["power_initial"]).all()
    at_yaw = robust_ref.expected_power(x, y, ws, wd, got["yaw"], *robust_ref.members(delta, weight), frame)[0]
    print(f"HornsRev1 x 2, 31 candidates x 9 members: E vs oracle at the returned yaw {np.abs(got['power'] / at_yaw - 1.0).max():.2e}, "
          f"gain {np.min(got['power'] / got['power_initial'] - 1.0):.2%}")
    assert np.abs(got["power"] / at_yaw - 1.0).max() <= 1e-4


@pytest.mark.parametrize("frame", FRAMES)
def test_default_mode(frame):
    """The handle's own resolve mode on Ablaincourt x 32: E never decreases; the reported E is what the oracle computes at the
    returned yaw within the project's 1e-4; the distance to the strict run's E stays within twice the largest one MEASURED
    (profiles/robust_timing.json, written by tools/robust_timing.py on these very farms), or 2e-4 if that is larger: the 1e-4
    contract counted once for each of the two evaluations compared."""
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, ref, strict = _case("Ablaincourt_", frame)
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    default = w.optimize_yaw(wd_uncertainty=_unc(frame))
    w.close()
    assert (default["power"] >= default["power_initial"]).all()
    at_yaw = robust_ref.expected_power(x, y, ws, wd, default["yaw"], DELTA, W, frame)[0]
    e = np.abs(default["power"] / at_yaw - 1.0)
    gap = np.abs(default["power"] / strict["power"] - 1.0)
    with open(os.path.join(ROOT, "profiles", "robust_timing.json")) as f:
        rec = json.load(f)["default_vs_strict"]
    bound = max(2.0 * rec["max_rel_gap"], 2e-4)
    print(f"{frame}: default-mode E vs oracle at its yaw {e.max():.2e}; gap to the strict run {gap.max():.2e} "
          f"(recorded {rec['max_rel_gap']:.2e}, bound {bound:.2e})")
    assert e.max() <= 1e-4
    assert gap.max() <= bound


def test_the_parent_is_untouched():
    """The robust object reads its handle and stores nothing in it: step outputs before and after are the same bits, and so
    are the env state, the wind, the calibration and the kernel choice.  An env that asks for
    optimal_yaw(wd_uncertainty=...) mid-episode goes on exactly as a twin that did not.  (The env's yaw bounds are +-40 deg
    and the float64 oracle is defined up to |yaw| = 45 deg — beyond it yields NaN —, so the env is asked with members
    (-3, 0, 3): in the FIXED frame a member's yaw reaches 43 deg.)"""
    import torch
    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd = yawopt_ref.gpu_case(yawopt_ref.layouts(), "Ablaincourt_", 16)
    w = WfStep(x, y, env_batch=16)
    w.set_wind(ws, wd)
    w.env_config()
    w.env_reset()
    yaw = np.random.default_rng(3).uniform(-20.0, 20.0, (16, len(x))).astype(np.float32)
    w.env_step(yaw * 0.1)
    before = w.step(yaw)
    snap = (w.env_get_state(), w.get_wind(), w.calibration(), w.kernel_choice(), w.risk_resolve())
    r = w.optimize_yaw(wd_uncertainty=_unc("fixed"))
    w.optimize_yaw(farms=[3, 1], strict=True, wd_uncertainty=_unc("relative"))
    w.uncertain_power(yaw, wd_uncertainty=_unc("fixed"))
    assert (r["power"] >= r["power_initial"]).all()
    after = w.step(yaw)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    now = (w.env_get_state(), w.get_wind(), w.calibration(), w.kernel_choice(), w.risk_resolve())
    for a, b in zip(snap[0].values(), now[0].values()):
        assert np.array_equal(a, b)
    assert np.array_equal(snap[1][0], now[1][0]) and np.array_equal(snap[1][1], now[1][1])
    assert snap[2] == now[2] and snap[3] == now[3] and snap[4] == now[4]
    w.close()

    B = 8
    kw = dict(env_batch=B, max_num_steps=20, kernel_choice=dict(calibrate=False))
    env, twin = envs.make("Ablaincourt_Floris", **kw), envs.make("Ablaincourt_Floris", **kw)
    env.reset(seed=5), twin.reset(seed=5)
    gen = torch.Generator().manual_seed(0)
    for _ in range(3):
        a = (torch.rand((B, env.num_turbines), generator=gen) * 10.0 - 5.0).cuda()
        env.step({"yaw": a}), twin.step({"yaw": a})
    d3, w3 = np.array([-3.0, 0.0, 3.0]), np.exp(-np.array([-3.0, 0.0, 3.0]) ** 2 / 18.0)
    opt = env.optimal_yaw(wd_uncertainty=_unc("fixed", d3, w3))
    assert all(v.is_cuda for v in opt.values()) and tuple(opt["yaw"].shape) == (B, env.num_turbines)
    lo, hi = env.controls["yaw"][0], env.controls["yaw"][1]
    assert bool((opt["yaw"] >= lo).all()) and bool((opt["yaw"] <= hi).all()) and bool((opt["power"] >= opt["power_initial"]).all())
    ws_e, wd_e = env.fi.get_wind()
    xs, ys = (np.asarray(env.farm_case.simul_params[k], float) for k in ("xcoords", "ycoords"))
    at_yaw = robust_ref.expected_power(xs, ys, ws_e, wd_e, opt["yaw"].cpu().numpy(), *robust_ref.members(d3, w3), "fixed")[0]
    assert np.abs(opt["power"].cpu().numpy() / at_yaw - 1.0).max() <= 1e-4  # (the env's farms under the env's wind)
    sub = env.optimal_yaw(passes=(3,), farms=[5, 2], wd_uncertainty=_unc("relative"))
    assert tuple(sub["yaw"].shape) == (2, env.num_turbines)
    a = (torch.rand((B, env.num_turbines), generator=gen) * 10.0 - 5.0).cuda()
    ra, rb = env.step({"yaw": a}), twin.step({"yaw": a})
    for k in ra[0]:
        assert torch.equal(ra[0][k], rb[0][k]), k
    assert torch.equal(ra[1], rb[1]) and torch.equal(ra[4]["power"], rb[4]["power"]) and torch.equal(ra[4]["load"], rb[4]["load"])
    env.close()
    twin.close()


def test_build_yaw_table_under_uncertainty():
    """A 3 x 2 axis on the row of three: every node of the table is what optimize_yaw(wd_uncertainty=...) returns for that
    node's wind alone (strict: float64 on either side; powers to 2e-6, the evaluators' batches differ); and the interface's
    single-farm surface returns the same answer."""
    from wfcrl_env_amd.backend import WfStep
    from wfcrl_env_amd.interface import HipFlorisInterface

    x, y = ROW3
    wd_axis, ws_axis = np.array([266.0, 270.0, 274.0]), np.array([7.0, 9.0])
    w = WfStep(x, y, env_batch=1)
    tab = w.build_yaw_table(wd_axis, ws_axis, strict=True, wd_uncertainty=_unc("fixed"))
    assert tab["table"].shape == (3, 2, 3) and tab["power"].shape == (3, 2)
    for i, d in enumerate(wd_axis):
        for j, s in enumerate(ws_axis):
            w.set_wind(s, d)
            node = w.optimize_yaw(strict=True, wd_uncertainty=_unc("fixed"))
            assert np.array_equal(node["yaw"][0], tab["table"][i, j]), (d, s)
            assert abs(node["power"][0] / tab["power"][i, j] - 1.0) <= POW_TOL
            assert abs(node["power_initial"][0] / tab["power_initial"][i, j] - 1.0) <= POW_TOL
    nominal = w.build_yaw_table(wd_axis, ws_axis, strict=True)
    assert (nominal["table"] != tab["table"]).any()
    w.close()
    fi = HipFlorisInterface(3, list(x), list(y))
    fi.init(wind_speed=9.0, wind_direction=270.0)
    yaw, power = fi.optimize_yaw(strict=True, wd_uncertainty=_unc("fixed"))
    assert np.array_equal(yaw.astype(np.float32), tab["table"][1, 1]) and abs(power / tab["power"][1, 1] - 1.0) <= POW_TOL


def test_refusals_name_their_cause():
    from wfcrl_env_amd import _lib
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    unc = _unc("fixed")
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.optimize_yaw(wd_uncertainty=unc)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.uncertain_power(wd_uncertainty=unc)
    w.close()
    w = WfStep(x, y, env_batch=2, model=dict(turbine_defs=[{}, {"tsr": 7.0}], turbine_type_of=[0, 1, 0]))  # two definitions
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.optimize_yaw(wd_uncertainty=unc)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several turbine definitions"):
        w.uncertain_power(wd_uncertainty=unc)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.optimize_yaw(wd_uncertainty=unc)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.uncertain_power(wd_uncertainty=unc)
    w.set_wind(8.0, 270.0)
    # no members: the C boundary itself, on a fresh handle (the Python surface always sets them first)
    w.close()
    w = WfStep(x, y, env_batch=2)
    w.set_wind(8.0, 270.0)
    rob = w._robust()
    out = (np.empty((2, 3), np.float32), np.empty(2, np.float32), np.empty(2, np.float32))
    with pytest.raises(ValueError, match="WF_E_INVALID.*no members"):
        _lib.check_robust(rob._lib.wf_robust_optimize(rob._r, None, 2, None, *[o.ctypes.data for o in out], 0), rob._r)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no members"):
        _lib.check_robust(rob._lib.wf_robust_evaluate(rob._r, None, 2, None, None, None, None, 0), rob._r)
    with pytest.raises(ValueError, match="wd_uncertainty"):
        w.uncertain_power()
    with pytest.raises(ValueError, match="members must be in 1..33"):
        w.optimize_yaw(wd_uncertainty=dict(delta=[], weight=[]))
    with pytest.raises(ValueError, match="members must be in 1..33"):
        w.optimize_yaw(wd_uncertainty=dict(delta=np.arange(34.0), weight=np.ones(34)))
    with pytest.raises(ValueError, match="strictly ascending"):
        w.optimize_yaw(wd_uncertainty=dict(delta=[-3.0, 3.0, 3.0], weight=[1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="strictly ascending"):
        w.uncertain_power(wd_uncertainty=dict(delta=[0.0, np.nan], weight=[1.0, 1.0]))
    with pytest.raises(ValueError, match="negative weight"):
        w.optimize_yaw(wd_uncertainty=dict(delta=[-3.0, 0.0, 3.0], weight=[1.0, -0.5, 1.0]))
    with pytest.raises(ValueError, match="all zero"):
        w.optimize_yaw(wd_uncertainty=dict(delta=[-3.0, 0.0, 3.0], weight=[0.0, 0.0, 0.0]))
    with pytest.raises(ValueError, match="frame"):
        w.optimize_yaw(wd_uncertainty=dict(delta=[0.0], weight=[1.0], frame="ground"))
    d1, w1 = np.array([0.0]), np.array([1.0])
    with pytest.raises(ValueError, match="WF_E_INVALID.*frame must be"):
        _lib.check_robust(rob._lib.wf_robust_set_members(rob._r, 1, d1.ctypes.data, w1.ctypes.data, 2), rob._r)
    with pytest.raises(ValueError, match="max_eval_farms must hold one farm's rows"):
        w.optimize_yaw(max_eval_farms=29, wd_uncertainty=unc)  # (5, 4): 6 rows x 5 members = 30
    with pytest.raises(ValueError, match="max_eval_farms must hold one farm's rows"):
        w.optimize_yaw(passes=(8,), max_eval_farms=44, wd_uncertainty=unc)  # 9 rows x 5 members = 45
    with pytest.raises(ValueError, match="lo < hi"):
        w.optimize_yaw(bounds=(10.0, 10.0), wd_uncertainty=unc)
    with pytest.raises(ValueError, match="K_p"):
        w.optimize_yaw(passes=(5, 16), wd_uncertainty=unc)
    with pytest.raises(ValueError, match="farm index out of range"):
        w.uncertain_power(farms=[0, 2], wd_uncertainty=unc)
    r = w.optimize_yaw(farms=[1], max_eval_farms=30, wd_uncertainty=unc)  # (the handle still serves after refusals)
    assert r["yaw"].shape == (1, 3) and r["power"][0] > r["power_initial"][0]
    u = w.uncertain_power(r["yaw"], farms=[1], wd_uncertainty=unc)
    assert abs(u["expected_power"][0] / r["power"][0] - 1.0) <= 2e-4  # (two default-mode evaluations, 1e-4 each)
    assert w.step(np.zeros((2, 3), np.float32))["power"].shape == (2, 3)
    w.close()
