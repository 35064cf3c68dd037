"""GPU: wake-model calibration on the device (include/wfcalib.h: wf_calib_score, wf_calib_fit; csrc/calib/,
csrc/modelset/wf_resolve_set.h) against tests/calib_ref.py — the NumPy restatement over the unchanged float64 oracle.

What is compared with what: powers with the oracle's per set inside parity.TOL_F64; losses inside the bound that tolerance
implies (calib_ref.loss); best_set, mean and n_invalid BIT FOR BIT on the problems the reference alone finds safe
(tests/test_calib.py asserts that on the CPU); the device with itself, bit for bit, across chunking, shapes of the reduce, host
and device arrays and two runs."""
import numpy as np
import pytest

from wfcrl_env_amd._lib import CALIB_ABI  # noqa: F401  (the new binding table: without the extension nothing here runs)

pytestmark = pytest.mark.gpu

SCALE = 5.0e6


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _four_sets():
    from test_modelset_gpu import FIELDS, SETS

    return {f: np.asarray(SETS[f], np.float64) for f in FIELDS}


def _power_fraction(got, ref):
    """The largest power error in units of the float64 contract's tolerance, as parity.within applies it (N <= 128)."""
    import parity

    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(ref, 1e3)).max() / parity.TOL_F64["power"])


@pytest.mark.parametrize("name,C", [("Ablaincourt_", 3), ("HornsRev1_", 2)])
def test_device_built_constants_are_the_oracle_per_set(layouts, name, C):
    """The four sets of tests/test_modelset_gpu.py — all eighteen fields differ, veer on and off — through the device-side
    construction of their constants: row_power inside TOL_F64 of the oracle per set, every loss inside its bound, the same
    best.  HornsRev1: N = 80, the four-wave kernel, rows past one wave."""
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    l = layouts[name]
    x, y = np.asarray(l["xcoords"], np.float64), np.asarray(l["ycoords"], np.float64)
    N = x.size
    rng = np.random.default_rng(C)
    ws, wd = rng.uniform(6.5, 11.0, C), 270.0 + rng.uniform(-15.0, 15.0, C)
    yaw = rng.uniform(-25.0, 25.0, (C, N)).astype(np.float32)
    sets = _four_sets()
    arr = cr.as_array(sets)
    obs = cr.powers(x, y, ws, wd, yaw, cr.as_array(cr.DEFAULT)[None])[0]  # "measured" under the default model
    ref = cr.score(x, y, ws, wd, yaw, obs, arr, scale=SCALE)
    w = WfStep(x, y, env_batch=1)
    got = w.model_loss(sets, ws, wd, yaw, obs, scale=SCALE, want=("loss", "best", "row_power"))
    assert got["loss"].shape == (4,) and got["row_power"].shape == (4, C, N) and got["row_power"].dtype == np.float32
    frac = [_power_fraction(got["row_power"][s], ref["power"][s]) for s in range(4)]
    lfrac = np.abs(got["loss"] - ref["loss"]) / ref["bound"]
    print(f"{name}: row_power at {max(frac):.3f} of TOL_F64, losses at {lfrac.max():.3f} of their bounds")
    assert max(frac) <= 1.0, frac
    assert (lfrac <= 1.0).all(), lfrac
    assert int(got["best"]) == ref["best"]
    assert (np.abs(np.diff(np.sort(ref["loss"]))) > 100.0 * ref["bound"].max()).all()  # (the four are told apart by far)
    w.close()


@pytest.fixture(scope="module")
def shapes_case(layouts):
    """G = 3 problems on Ablaincourt with S = 70 candidates (past a wave) of C = 5 conditions, and what one chunk gives."""
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    x, y = np.asarray(l["xcoords"], np.float64), np.asarray(l["ycoords"], np.float64)
    G, S, C, N = 3, 70, 5, x.size
    rng = np.random.default_rng(11)
    ws, wd = rng.uniform(6.5, 11.0, (G, C)), 270.0 + rng.uniform(-15.0, 15.0, (G, C))
    yaw = rng.uniform(-25.0, 25.0, (G, C, N)).astype(np.float32)
    lo, hi, init = cr.bounds_arrays({"ambient_ti": (0.03, 0.15), "ka": (0.2, 0.6), "alpha": (0.3, 0.9), "veer": (-3.0, 3.0)})
    arr = rng.uniform(lo, hi, (G, S, cr.NF))
    power = rng.uniform(0.4e6, 3.0e6, (G, C, N))
    weight = rng.uniform(0.0, 2.0, (G, C, N))
    weight[rng.uniform(size=weight.shape) < 0.2] = 0.0
    weight[2, 3:] = 0.0  # a problem with fewer conditions, padded
    w = WfStep(x, y, env_batch=1)
    one = w.model_loss(cr.as_dict(arr), ws, wd, yaw, power, weight, SCALE, want=("loss", "best", "row_power"))
    one = {k: np.array(v) for k, v in one.items()}
    yield dict(w=w, G=G, S=S, C=C, N=N, ws=ws, wd=wd, yaw=yaw, arr=arr, power=power, weight=weight, one=one)
    w.close()


def test_chunks_runs_and_device_arrays_give_the_same_bits(shapes_case):
    import torch

    import calib_ref as cr

    c = shapes_case
    w, one = c["w"], c["one"]
    sets = cr.as_dict(c["arr"])
    args = (c["ws"], c["wd"], c["yaw"], c["power"], c["weight"], SCALE)
    want = ("loss", "best", "row_power")
    assert one["loss"].shape == (c["G"], c["S"]) and one["best"].dtype == np.int32 and np.isfinite(one["loss"]).all()
    assert np.array_equal(one["best"], np.argmin(one["loss"], axis=1))
    three = w.model_loss(sets, *args, want=want, max_eval_farms=c["S"] * c["C"])  # three chunks of one problem
    again = w.model_loss(sets, *args, want=want)
    dev = w.model_loss(sets, *[torch.as_tensor(a).cuda() for a in args[:5]], SCALE, want=want)
    assert all(v.is_cuda for v in dev.values())
    for k in want:
        assert _same(one[k], three[k]), k
        assert _same(one[k], again[k]), k
        assert _same(one[k], dev[k]), k
    # a ragged last chunk: two problems per chunk, the second chunk half empty
    two = w.model_loss(sets, *args, want=want, max_eval_farms=2 * c["S"] * c["C"])
    for k in want:
        assert _same(one[k], two[k]), k


def test_problem_alone_fewer_candidates_and_fewer_conditions(shapes_case):
    """G = 1 against its rows of G = 3; S = 3 and C = 1 against the sums they are part of."""
    import calib_ref as cr

    c = shapes_case
    w, one = c["w"], c["one"]
    g = 1
    alone = w.model_loss(cr.as_dict(c["arr"][g]), c["ws"][g], c["wd"][g], c["yaw"][g], c["power"][g], c["weight"][g], SCALE,
                         want=("loss", "best", "row_power"))
    assert alone["loss"].shape == (c["S"],) and alone["row_power"].shape == (c["S"], c["C"], c["N"])  # (no G axis in, none out)
    for k in alone:
        assert _same(alone[k], one[k][g]), k
    few = w.model_loss(cr.as_dict(c["arr"][:, :3]), c["ws"], c["wd"], c["yaw"], c["power"], c["weight"], SCALE)
    assert _same(few["loss"], one["loss"][:, :3])
    assert np.array_equal(few["best"], np.argmin(one["loss"][:, :3], axis=1))
    first = w.model_loss(cr.as_dict(c["arr"]), c["ws"][:, :1], c["wd"][:, :1], c["yaw"][:, :1], c["power"][:, :1], c["weight"][:, :1],
                         SCALE, want=("loss", "row_power"))
    assert _same(first["row_power"], one["row_power"][:, :, :1])
    # C = 1: the loss is the one row's sum, 0.0 + row; the reference's formula on the device's own powers gives its bits
    L = np.stack([cr.loss(first["row_power"][q].astype(np.float64), c["power"][q, :1], c["weight"][q, :1], SCALE)[0] for q in range(c["G"])])
    assert _same(first["loss"], L)
    # ... and so for C = 5: the summation order is the header's
    L5 = np.stack([cr.loss(one["row_power"][q].astype(np.float64), c["power"][q], c["weight"][q], SCALE)[0] for q in range(c["G"])])
    assert _same(one["loss"], L5)


def test_shared_sets_and_masked_entries(shapes_case):
    import calib_ref as cr

    c = shapes_case
    w = c["w"]
    shared = c["arr"][0]
    args = (c["ws"], c["wd"], c["yaw"], c["power"], c["weight"], SCALE)
    a = w.model_loss(cr.as_dict(shared), *args, want=("loss", "best", "row_power"))
    b = w.model_loss(cr.as_dict(np.broadcast_to(shared, c["arr"].shape)), *args, want=("loss", "best", "row_power"))
    for k in a:
        assert _same(a[k], b[k]), k
    assert _same(a["loss"][0], c["one"]["loss"][0])
    # what stands under a zero weight does not matter
    garbage = c["power"].copy()
    masked = c["weight"] == 0.0
    garbage[masked] = np.random.default_rng(5).uniform(-1e9, 1e9, int(masked.sum()))
    garbage[tuple(np.argwhere(masked)[0])] = np.nan  # (an off-line turbine as a logger records it)
    d = w.model_loss(cr.as_dict(shared), c["ws"], c["wd"], c["yaw"], garbage, c["weight"], SCALE)
    assert _same(a["loss"], d["loss"]) and np.array_equal(a["best"], d["best"])
    # a NaN that is NOT masked: every loss of its problem counts as +inf and candidate 0 wins; the other problems keep their bits
    # (a host caller is refused by name: the device caller's arrays are not read on the host)
    import torch

    poisoned = c["power"].copy()
    poisoned[1][tuple(np.argwhere(c["weight"][1] > 0.0)[0])] = np.nan
    with pytest.raises(ValueError, match="a measured power is not finite"):
        w.model_loss(cr.as_dict(shared), c["ws"], c["wd"], c["yaw"], poisoned, c["weight"], SCALE)
    n = w.model_loss(cr.as_dict(shared), *[torch.as_tensor(v).cuda() for v in (c["ws"], c["wd"], c["yaw"], poisoned, c["weight"])], SCALE)
    nl, nb = n["loss"].cpu().numpy(), n["best"].cpu().numpy()
    assert (nl[1] == np.inf).all() and nb[1] == 0
    assert _same(nl[[0, 2]], a["loss"][[0, 2]]) and np.array_equal(nb[[0, 2]], a["best"][[0, 2]])
    # ... and no weight is a weight of ones
    e = w.model_loss(cr.as_dict(shared), c["ws"], c["wd"], c["yaw"], c["power"], None, SCALE)
    f = w.model_loss(cr.as_dict(shared), c["ws"], c["wd"], c["yaw"], c["power"], np.ones_like(c["power"]), SCALE)
    assert _same(e["loss"], f["loss"]) and not _same(e["loss"], a["loss"])


@pytest.mark.parametrize("name", ["row3", "Ablaincourt_"])
def test_the_fit_has_the_references_bits(name):
    """The twin problem, G = 2 with different truths, S = 16, E = 4, I = 3, three free fields: safe by the reference alone
    (tests/test_calib.py), so best_set, mean and n_invalid are the reference's bit for bit; losses inside their bounds."""
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    c, r = cr.fit_case(name), cr.fit_reference(name)
    assert r["safe"].all()
    w = WfStep(c["x"], c["y"], env_batch=1)
    got = w.calibrate_model(c["ws"], c["wd"], c["yaw"], c["obs"], cr.FIT_FREE, candidates=c["S"], elites=c["E"], sigma=c["sigma"],
                            seed=c["seed"], scale=SCALE)
    best, mean = cr.as_array(got["best_set"]), cr.as_array(got["mean"])
    assert _same(best, r["best_set"]) and _same(mean, r["mean"])
    assert np.array_equal(got["n_invalid"], r["n_invalid"]) and got["n_invalid"].dtype == np.int32
    fr = {"best_loss": np.abs(got["best_loss"] - r["best_loss"]) / r["best_bound"],
          "init_loss": np.abs(got["init_loss"] - r["init_loss"]) / r["init_bound"],
          "history": np.abs(got["history"] - r["history"]) / r["history_bound"]}
    print(f"{name}: losses at {max(v.max() for v in fr.values()):.3f} of their bounds; fit_power at "
          f"{_power_fraction(got['fit_power'], r['fit_power']):.3f} of TOL_F64")
    for k, v in fr.items():
        assert (v <= 1.0).all(), (k, v)
    assert (got["best_loss"] <= got["init_loss"]).all() and (np.diff(got["history"], axis=1) <= 0.0).all()
    assert _same(got["best_loss"], got["history"][:, -1])
    assert _power_fraction(got["fit_power"], r["fit_power"]) <= 1.0
    # the best set through the scoring call: its rows are fit_power and its loss is best_loss, bit for bit
    sc = w.model_loss(cr.as_dict(best[:, None]), c["ws"], c["wd"], c["yaw"], c["obs"], scale=SCALE, want=("loss", "row_power"))
    assert _same(sc["row_power"][:, 0], got["fit_power"])
    assert _same(sc["loss"][:, 0], got["best_loss"])
    # one problem alone is its rows of the two (a problem's draws are its index's: problem 0), in chunks too
    solo = w.calibrate_model(c["ws"][0], c["wd"][0], c["yaw"][0], c["obs"][0], cr.FIT_FREE, candidates=c["S"], elites=c["E"],
                             sigma=c["sigma"], seed=c["seed"], scale=SCALE)
    assert _same(cr.as_array(solo["best_set"]), best[0]) and _same(solo["history"], got["history"][0])
    chunks = w.calibrate_model(c["ws"], c["wd"], c["yaw"], c["obs"], cr.FIT_FREE, candidates=c["S"], elites=c["E"], sigma=c["sigma"],
                               seed=c["seed"], scale=SCALE, max_eval_farms=c["S"] * c["C"])
    for k in ("best_loss", "init_loss", "history", "fit_power", "n_invalid"):
        assert _same(chunks[k], got[k]), k
    assert _same(cr.as_array(chunks["best_set"]), best) and _same(cr.as_array(chunks["mean"]), mean)
    w.close()


def test_invalid_candidates_are_counted_and_never_win():
    """Bounds that let ka TI + kb go non-positive: n_invalid is the reference's, no loss is NaN, the winner is valid."""
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    c = cr.invalid_case()
    r = c["ref"]
    assert r["n_invalid"][0] >= 3 and r["safe"].all()
    w = WfStep(c["x"], c["y"], env_batch=1)
    got = w.calibrate_model(c["ws"], c["wd"], c["yaw"], c["obs"], cr.INVALID_FREE, candidates=c["S"], elites=c["E"], sigma=c["sigma"],
                            seed=c["seed"], scale=SCALE)
    assert np.array_equal(got["n_invalid"], r["n_invalid"])
    for k in ("best_loss", "init_loss", "history", "fit_power"):
        assert np.isfinite(got[k]).all(), k
    best = cr.as_array(got["best_set"])
    assert cr.valid(best).all() and _same(best, r["best_set"]) and _same(cr.as_array(got["mean"]), r["mean"])
    assert (np.abs(got["best_loss"] - r["best_loss"]) <= r["best_bound"]).all()
    w.close()


def test_a_fit_whose_losses_are_all_not_finite_keeps_its_start():
    """include/wfcalib.h, WHAT A NaN DOES: an unmasked NaN power (device arrays: not read on the host) makes every loss of the
    problem +inf; candidate 0 wins every iteration, so the fit keeps init; the problem beside it is not touched."""
    import torch

    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    x, y = cr.ROW3
    ws, wd, yaw = cr.conditions("row3", 2, 2)
    obs = np.stack([cr.powers(x, y, ws[g], wd[g], yaw[g], cr.as_array(cr.FIT_TRUTH[g])[None])[0] for g in range(2)])
    kw = dict(candidates=8, elites=2, sigma=(0.2, 0.1), seed=4, scale=SCALE)
    w = WfStep(x, y, env_batch=1)
    clean = w.calibrate_model(ws, wd, yaw, obs, cr.FIT_FREE, **kw)
    bad = obs.copy()
    bad[1, 0, 2] = np.nan
    got = w.calibrate_model(*[torch.as_tensor(v).cuda() for v in (ws, wd, yaw, bad)], cr.FIT_FREE, **kw)
    got = {k: ({f: v.cpu().numpy() for f, v in a.items()} if isinstance(a, dict) else a.cpu().numpy()) for k, a in got.items()}
    best = cr.as_array(got["best_set"])
    assert _same(best[1], cr.as_array(cr.DEFAULT)) and got["best_loss"][1] == np.inf and (got["history"][1] == np.inf).all()
    assert got["n_invalid"][1] == 0 and np.isfinite(got["fit_power"]).all() and np.isfinite(cr.as_array(got["mean"])).all()
    for k in ("best_loss", "init_loss", "history", "fit_power"):
        assert _same(got[k][0], clean[k][0]), k
    assert _same(best[0], cr.as_array(clean["best_set"])[0])
    w.close()


def test_refusals_by_name(layouts):
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    x, y = cr.ROW3
    C = 2
    ws, wd, yaw = cr.conditions("row3", 1, C)
    ws, wd, yaw = ws[0], wd[0], yaw[0]
    power = np.full((C, 3), 1.0e6)
    free = {"ka": (0.2, 0.6)}
    w = WfStep(x, y, env_batch=4)
    ok = w.calibrate_model(ws, wd, yaw, power, free, candidates=3, elites=1, sigma=(0.1,), scale=SCALE)
    assert np.isfinite(ok["best_loss"])
    with pytest.raises(ValueError, match="S must be >= 3"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=2, elites=1, sigma=(0.1,))
    with pytest.raises(ValueError, match="at least S C"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=8, sigma=(0.1,), max_eval_farms=15)
    with pytest.raises(ValueError, match="at least S C"):
        w.model_loss([{}] * 8, ws, wd, yaw, power, max_eval_farms=15)
    with pytest.raises(ValueError, match="iterations I must be in 1..16"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=8, sigma=(0.1,) * 17)
    with pytest.raises(ValueError, match="elites E must be in 1..S"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=8, elites=9, sigma=(0.1,))
    with pytest.raises(ValueError, match="sigma must be finite and non-negative"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=8, sigma=(0.1, -0.1))
    with pytest.raises(ValueError, match="outside the bounds"):
        w.calibrate_model(ws, wd, yaw, power, free, init={"ka": 0.7}, candidates=8, sigma=(0.1,))
    with pytest.raises(ValueError, match="init: parameter set 0: must be > 0: ka"):
        w.calibrate_model(ws, wd, yaw, power, {"ka": (-1.0, 0.6)}, init={"ka": -0.5}, candidates=8, sigma=(0.1,))
    with pytest.raises(ValueError, match="weight must be finite and >= 0"):
        w.calibrate_model(ws, wd, yaw, power, free, candidates=8, sigma=(0.1,), weight=np.full((C, 3), -1.0))
    with pytest.raises(ValueError, match="weight must be finite and >= 0"):
        w.model_loss([{}], ws, wd, yaw, power, weight=np.full((C, 3), -1.0))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale must be finite and > 0"):
            w.model_loss([{}], ws, wd, yaw, power, scale=bad)
    with pytest.raises(ValueError, match="must be > 0: alpha"):
        w.model_loss([{"alpha": 0.0}], ws, wd, yaw, power)
    with pytest.raises(ValueError, match="candidates S must be in 1..1024"):
        w.model_loss([{}] * 1025, ws, wd, yaw, power)
    # a parent that holds sets, several layouts or turbine definitions
    w.set_model_sets([{"ka": 0.3}], np.zeros(4, np.int32))
    with pytest.raises(Exception, match="calibration serves one wake model.*wf_set_model_sets"):
        w.model_loss([{}], ws, wd, yaw, power)
    w.clear_model_sets()
    assert np.isfinite(w.model_loss([{}], ws, wd, yaw, power)["loss"]).all()  # (and the refusal leaves the object usable)
    w.close()
    w = WfStep(np.stack([x, x]), np.stack([y, y + 100.0]), env_batch=2, layout_of=np.array([0, 1], np.int32))
    with pytest.raises(Exception, match="calibration serves a handle with ONE layout"):
        w.model_loss([{}], ws, wd, yaw, power)
    w.close()
    w = WfStep(x, y, env_batch=1, model=dict(turbine_defs=[{}, {"tsr": 7.5}], turbine_type_of=[0, 1, 0]))
    with pytest.raises(Exception, match="calibration serves one turbine definition"):
        w.model_loss([{}], ws, wd, yaw, power)
    w.close()


def test_kernel_reports_no_private_segment_and_the_evaluator_holds_the_sets():
    import calib_ref as cr
    from wfcrl_env_amd.backend import WfStep

    x, y = cr.ROW3
    w = WfStep(x, y, env_batch=1)
    info = w.calib_kernel_info()["advance"]
    assert info["scratch_bytes"] == 0 and 0 < info["vgprs"] <= 128 and info["lds_bytes"] <= 32768, info
    ws, wd, yaw = cr.conditions("row3", 2, 3)
    w.calib_timing(detail=True)
    w.model_loss([{}, {"ka": 0.3}], ws, wd, yaw, np.full((2, 3, 3), 1.0e6))
    t = w.calib_timing()
    assert t["total_ms"] > 0.0 and t["step_ms"] > 0.0 and t["glue_ms"] > 0.0
    assert w._calib().evaluator() is not None
    w.close()
