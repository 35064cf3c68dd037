"""CPU: the calib extension (include/wfcalib.h) — header, binding table, kernel metadata — and the properties of the reference
the GPU tests use (tests/calib_ref.py: the loss and the cross-entropy fit restated in NumPy over the float64 oracle)."""
import os
import re

import numpy as np

from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile
from wfcrl_env_amd._lib import CALIB_ABI  # noqa: F401  (the new binding table: without the extension nothing here runs)

KERNELS = ("wf_calib_advance_kernel",)
ENTRY_POINTS = {"wf_calib_create", "wf_calib_destroy", "wf_calib_config", "wf_calib_score", "wf_calib_fit", "wf_calib_set_timing",
                "wf_calib_last_timing", "wf_calib_evaluator", "wf_calib_kernel_info", "wf_calib_last_error"}


def test_calib_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfcalib.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.CALIB_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.CALIB_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.MODELSET_ABI, _lib.PLAN_ABI, _lib.SCENPLAN_ABI):
        assert not set(table) & set(_lib.CALIB_ABI)
    text = open(os.path.join(ROOT, "include", "wfcalib.h")).read()
    assert "PARITY UNPINNED" in text and "tests/calib_ref.py" in text and "NOT bit-identical" in text
    assert "NO LONGER DESCRIBE ITS DEVICE TABLE" in text  # (said where wf_calib_evaluator is declared)
    for name, value in (("WF_CALIB_KERNELS", 1), ("WF_CALIB_FIELDS", 18), ("WF_CALIB_MIN_S", 3), ("WF_CALIB_MAX_S", 1024),
                        ("WF_CALIB_MAX_ITER", 16)):
        assert re.search(r"^#define %s %d\b" % (name, value), text, flags=re.M), name
    import calib_ref

    assert calib_ref.FIELDS == _lib._MODEL_SET_FIELDS


def test_calib_kernel_has_no_private_segment(tmp_path):
    """The one glue kernel, compiled with the Makefile's flags: exactly this one, no private segment, no spilled register,
    no out-of-line call.  Metadata only."""
    mk = makefile()
    assert "CALIBOBJ = calib/wf_calib_kernels.o calib/wf_calib_abi.o" in mk and "$(CALIBOBJ): %.o: %.hip" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(CALIBOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*calib/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("calib/wf_calib_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text


def test_the_device_restatement_stands_beside_the_host_code():
    """modelset/wf_resolve_set.h writes exactly the set-owned members of WfResolveConsts, with the general-range routines of
    wf_f64_math.h and no libm call; the deviate and the generator are the shared ones."""
    csrc = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    text = open(os.path.join(csrc, "modelset", "wf_resolve_set.h")).read()
    code = re.sub(r"//.*", "", text)
    written = set(re.findall(r"\br\.(\w+)(?:\[k\])? = ", code))
    owned = {"amb", "shearf", "uinf1", "nu1", "vel_top", "vel_bot", "alpha", "beta", "ka", "kb", "ad", "bd", "dm", "defl_alpha",
             "defl_beta", "defl_ka", "defl_kb", "ch_constant", "ch_ai", "ch_amb_pow", "ch_down", "cos_veer", "cos2_veer", "sin2_veer",
             "sin_2veer"}
    assert written == owned, written ^ owned
    assert "pow_any(" in code and "sincos_any(" in code and not re.search(r"\b(std::)?(pow|cos|sin|exp)\(", code)
    assert "NOT BIT-IDENTICAL" in text
    kern = open(os.path.join(csrc, "calib", "wf_calib_kernels.hip")).read()
    assert "wf_deviate.h" in kern and "wf_deviate(" in kern and "0xD2511F53" not in kern and "atomic" not in re.sub(r"//.*", "", kern)


def test_the_default_set_is_the_librarys_and_the_oracles():
    import calib_ref
    from oracle.floris_gch_numpy import ModelParams
    from wfcrl_env_amd.backend import default_model

    lib, p = default_model(), ModelParams()
    for f in calib_ref.FIELDS:
        assert calib_ref.DEFAULT[f] == lib[f], f
        assert calib_ref.DEFAULT[f] == (getattr(p, f) if getattr(p, f) is not None else getattr(p, f[len("defl_"):])), f


def test_the_loss_at_the_generating_set_is_exactly_zero():
    import calib_ref as cr

    c = cr.fit_case("row3")
    for g in range(c["G"]):
        r = cr.score(c["x"], c["y"], c["ws"][g], c["wd"][g], c["yaw"][g], c["obs"][g], np.stack([c["truth"][g], c["init"]]))
        assert r["loss"][0] == 0.0 and r["bound"][0] > 0.0 and r["loss"][1] > 100.0 * r["bound"][1] and r["best"] == 0
    # the order of the sums: a sum that NumPy's pairwise reduction would round differently
    p = np.zeros((1, 2, 3))
    obs = np.array([[1e4, 1.0, 1e-4], [3.0, 0.0, 0.0]])
    w = np.array([[1.0, 1.0, 2.0], [0.5, 0.0, 7.0]])
    L, _ = cr.loss(p, obs, w, scale=2.0)
    q = obs / 2.0
    by_hand = (0.0 + (((0.0 + 1.0 * (q[0, 0] * q[0, 0])) + 1.0 * (q[0, 1] * q[0, 1])) + 2.0 * (q[0, 2] * q[0, 2]))) + \
        (((0.0 + 0.5 * (q[1, 0] * q[1, 0])) + 0.0) + 0.0)
    assert L[0] == by_hand
    # a zero weight masks whatever stands there
    obs2 = obs.copy()
    obs2[1, 1] = 123456.0
    assert cr.loss(p, obs2, w, scale=2.0)[0][0] == L[0]
    obs2[1, 1] = np.nan  # (an off-line turbine recorded as NaN, masked)
    assert cr.loss(p, obs2, w, scale=2.0)[0][0] == L[0]


def test_a_loss_that_is_not_finite_is_plus_inf_and_candidate_0_wins_among_them():
    """A NaN observation under a positive weight makes every loss of the problem NaN: each counts as +inf, as an invalid
    candidate's does — a NaN would compare false with everything, rank first and leave the argmin without a winner — and the
    winner among equals is the lowest index, candidate 0."""
    import calib_ref as cr

    p = np.random.default_rng(0).uniform(1e5, 2e6, (5, 2, 3))
    obs = p[2].copy()
    obs[0, 1] = np.nan
    L, b = cr.loss(p, obs)
    assert (L == np.inf).all() and (b == 0.0).all()
    assert int(np.argmin(L)) == 0 and cr.ranks(L).tolist() == [0, 1, 2, 3, 4]
    w = np.ones((2, 3))
    w[0, 1] = 0.0
    L, b = cr.loss(p, obs, w)
    assert np.isfinite(L).all() and L[2] == 0.0 and int(np.argmin(L)) == 2
    # one candidate's NaN alone (a solve that left the model's domain) ranks last, not first
    p2 = p.copy()
    p2[1, 1, 2] = np.nan
    L, _ = cr.loss(p2, p[2])
    assert L[1] == np.inf and cr.ranks(L)[1] == 4 and int(np.argmin(L)) == 2
    # the kernel guards the same two places: the argmin's index and the sum's terms
    import os

    kern = open(os.path.join(ROOT, "wfcrl-env_amd", "csrc", "calib", "wf_calib_kernels.hip")).read()
    assert "bi[0] == INT_MAX ? 0 : bi[0]" in kern and "best_s == INT_MAX ? 0 : best_s" in kern
    assert "w == 0.0 ? 0.0 : w * (q * q)" in kern and "!(fabs(L) < HUGE_VAL)" in kern


def test_candidates_and_update_rules():
    """Candidate 0 is the best so far, candidate 1 the mean; a fixed field never moves; a clipped candidate sits on the bound
    bit for bit; ranks break ties by index and put +inf last; the elite mean adds in ascending s and divides once."""
    import calib_ref as cr
    import plan_ref

    lo, hi, init = cr.bounds_arrays(cr.FIT_FREE)
    mu = init.copy()
    mu[cr.FIELDS.index("ka")] = 0.58
    S = 40
    a = cr.candidates(mu, init, lo, hi, 0.5, 9, 3, 2, S)
    assert a.shape == (S, cr.NF) and np.array_equal(a[0], init) and np.array_equal(a[1], mu)
    free = [cr.FIELDS.index(f) for f in cr.FIT_FREE]
    fixed = [j for j in range(cr.NF) if j not in free]
    assert (a[:, fixed] == init[fixed]).all()  # bit for bit: lo == hi
    assert (a[:, free] >= lo[free]).all() and (a[:, free] <= hi[free]).all()
    on_lo, on_hi = a[2:, free] == lo[free], a[2:, free] == hi[free]
    assert on_lo.any() and on_hi.any() and (~on_lo & ~on_hi).any()
    j = cr.FIELDS.index("alpha")
    z = plan_ref.deviate(9, 3, 5 * cr.NF + j, 2)  # problem 3, candidate 5, field alpha, iteration 2
    assert a[5, j] == min(max(mu[j] + (0.5 * (hi[j] - lo[j])) * z, lo[j]), hi[j])
    assert np.array_equal(cr.candidates(mu, init, lo, hi, 0.0, 9, 3, 2, S)[1:], np.broadcast_to(mu, (S - 1, cr.NF)))
    # a problem's draws are its index's
    assert not np.array_equal(cr.candidates(mu, init, lo, hi, 0.5, 9, 4, 2, S), a)
    L = np.array([1.0, np.inf, 0.5, 1.0, np.inf, 0.25])
    assert cr.ranks(L).tolist() == [2, 4, 1, 3, 5, 0]
    sets = np.zeros((4, cr.NF))
    sets[:, 0] = [1e16, 1.0, -1e16, 1.0]
    assert cr.elite_mean(sets, np.array([True, True, True, True]), 4)[0] == ((((0.0 + 1e16) + 1.0) + -1e16) + 1.0) / 4.0
    # validity, with the roundings of the host check
    bad = cr.as_array([dict(ka=-0.07), dict(ka=-0.06), dict(ambient_ti=0.0), dict(ch_constant=-1.0), dict(defl_alpha=0.0), {}])
    assert cr.valid(bad).tolist() == [False, True, False, False, False, True]


def test_the_gpu_cases_are_safe_by_the_reference_alone():
    """The twin problems the GPU tests compare bits on: every problem's elite / non-elite and winner / runner-up pairs are
    further apart than the sum of their bounds in every iteration, with the seeds chosen here; the fit does something."""
    import calib_ref as cr

    for name in ("row3", "Ablaincourt_"):
        c, r = cr.fit_case(name), cr.fit_reference(name)
        print(f"case {name}: margins {r['margin']}, bounds {r['best_bound']}, init loss {r['init_loss']}, best loss {r['best_loss']}, "
              f"winners {r['winners'].tolist()}")
        assert r["safe"].all() and np.isfinite(r["margin"]).all()
        assert (r["margin"] > 50.0 * r["history_bound"].max(axis=1)).all()  # (not by a hair)
        assert (np.diff(r["history"], axis=1) <= 0.0).all()  # candidate 0 is the best so far
        assert (r["best_loss"] < 0.1 * r["init_loss"]).all() and (r["best_loss"] == r["history"][:, -1]).all()
        assert (r["winners"] >= 2).any() and (r["n_invalid"] == 0).all()
        free = [cr.FIELDS.index(f) for f in cr.FIT_FREE]
        fixed = [j for j in range(cr.NF) if j not in free]
        assert (r["best_set"][:, fixed] == c["init"][fixed]).all() and (r["mean"][:, fixed] == c["init"][fixed]).all()
        assert not np.array_equal(r["best_set"][0], r["best_set"][1])  # different truths, different fits


def test_invalid_candidates_rank_last_and_are_counted():
    import calib_ref as cr

    c = cr.invalid_case()
    r = c["ref"]
    print(f"invalid case: {r['n_invalid']} invalid candidates, margin {r['margin']}, winners {r['winners'].tolist()}")
    assert r["n_invalid"][0] >= 3 and r["safe"].all()
    assert cr.valid(r["best_set"]).all() and np.isfinite(r["best_loss"]).all() and (r["best_loss"] <= r["init_loss"]).all()
    # one iteration by hand: the invalid candidates are exactly the ones ranked last
    a = cr.candidates(c["init"], c["init"], c["lo"], c["hi"], c["sigma"][0], c["seed"], 0, 0, c["S"])
    ok = cr.valid(a)
    assert 0 < (~ok).sum() < c["S"] - c["E"]
    L = np.full(c["S"], np.inf)
    L[ok] = cr.loss(cr.powers(c["x"], c["y"], c["ws"][0], c["wd"][0], c["yaw"][0], a[ok]), c["obs"][0])[0]
    assert set(np.argsort(cr.ranks(L))[-(~ok).sum():]) == set(np.flatnonzero(~ok))
