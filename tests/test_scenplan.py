"""CPU: the scenplan extension (include/wfscenplan.h) — header, binding table, kernel metadata — and the properties of the
reference the GPU tests use (tests/scenplan_ref.py: the planner's search scored by the scenario look-ahead's statistics,
composed from plan_ref and scenario_ref over the float64 oracle)."""
import os
import re

import numpy as np

import plan_cases
import plan_ref
import scenario_ref
import scenplan_cases as C
import scenplan_ref
from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile
from test_lookahead import PARAMS

KERNELS = ("wf_scenplan_paths_kernel", "wf_scenplan_advance_kernel")
ENTRY_POINTS = {"wf_scenplan_" + n for n in ("create", "destroy", "config", "run", "set_timing", "last_timing", "evaluator",
                                            "kernel_info", "last_error")}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def test_scenplan_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfscenplan.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.SCENPLAN_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.SCENPLAN_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI,
                  _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.SERIES_ABI, _lib.ROLLOUT_ABI, _lib.RETGRAD_ABI, _lib.WINDGEN_ABI,
                  _lib.SCENARIO_ABI):
        assert not set(table) & set(_lib.SCENPLAN_ABI)
    # the entry points mirror wfplan.h name for name
    assert {s.replace("wf_scenplan_", "") for s in syms} == {s.replace("wf_plan_", "") for s in declared("wfplan.h")}
    text = open(os.path.join(ROOT, "include", "wfscenplan.h")).read()
    assert "THE PROJECT'S OWN" in text and "PARITY UNPINNED" in text and "tests/scenplan_ref.py" in text
    assert "WHY I <= 16" in text and "streams 16, 17" in text
    assert '#include "wfplan.h"' in text and '#include "wfscenario.h"' in text  # (the limits of both parents, named there once)
    for name, value in (("WF_SCENPLAN_KERNELS", len(KERNELS)), ("WF_SCENPLAN_MIN_K", 3),
                        ("WF_SCENPLAN_MAX_ITERATIONS", scenplan_ref.MAX_ITERATIONS)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name
    for header, name in (("wflookahead.h", "WF_LOOKAHEAD_MAX_H"), ("wfscenario.h", "WF_SCENARIO_MAX_MEMBERS"),
                         ("wfscenario.h", "WF_SCENARIO_MAX_ROWS")):
        assert re.search(r"^#define %s \d+$" % name, open(os.path.join(ROOT, "include", header)).read(), flags=re.M), name
        assert name in text, name


def test_scenplan_kernels_have_no_private_segment(tmp_path):
    """The two glue kernels, compiled with the Makefile's flags: exactly these two, no private segment, no spilled register,
    no out-of-line call.  Metadata only."""
    mk = makefile()
    assert "SCENPLANOBJ = scenplan/wf_scenplan_kernels.o scenplan/wf_scenplan_abi.o" in mk and "$(SCENPLANOBJ): %.o: %.hip" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(SCENARIOOBJ\) \$\(SCENPLANOBJ\)$", mk, flags=re.M)
    assert re.search(r"^\trm -f .*scenplan/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("scenplan/wf_scenplan_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "csrc", "scenplan", "wf_scenplan_kernels.hip")).read()
    for header in ("../wf_philox.h", "../ext/wf_deviate.h", "wf_scenplan.h"):
        assert '#include "%s"' % header in src, header
    assert "0xD2511F53" not in src and "wf_staged_row_rewards(" in src  # (the generator and the reward tile are defined once)


def _plan(name, **over):
    c = C.case(name)
    kw = dict(H=c["H"], K=c["K"], E=c["E"], sigma=c["sigma"], seed=c["seed"], M=c["M"], process=C.PROCESS,
              scenario_seed=c["scenario_seed"], tail=c["tail"], lam=c["lam"], anchor=c["anchor"], bounds=C.BOUNDS, mean0=c["mean0"])
    kw.update(over)
    return scenplan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, kw.pop("H"), kw.pop("K"), kw.pop("E"),
                             kw.pop("sigma"), kw.pop("seed"), C.GAMMA, C.LOAD_COEF, kw.pop("M"), kw.pop("process"),
                             kw.pop("scenario_seed"), **kw)


def test_zero_width_plans_are_the_hold_or_the_warm_start():
    """sigma all zero: every candidate but 0 equals the mean, so the plan is the hold — or, with one iteration and a warm
    start inside +-yaw_step, the warm start where that scores more (candidate 1, the lowest index among equals)."""
    c = C.case("A")
    cold = _plan("A", sigma=(0.0, 0.0))
    assert not cold["plan"].any() and not cold["mean"].any() and np.array_equal(_bits(cold["plan_score"]), _bits(cold["hold_score"]))
    assert np.array_equal(_bits(cold["final_yaw"]), _bits(np.asarray(c["state"]["yaw"])))
    assert (cold["winners"] == 0).all() and np.isinf(cold["margin"]).all()  # (all trajectories identical: nothing to decide)
    warm0 = np.random.default_rng(1).uniform(-4.0, 4.0, (c["farms"], c["H"], c["N"])).astype(np.float32)
    warm = _plan("A", sigma=(0.0,), mean0=warm0)
    took = warm["winners"][0] != 0
    assert took.any() and (~took).any() and (warm["winners"][0][took] == 1).all()
    assert np.array_equal(warm["plan"][took], warm0[took]) and not warm["plan"][~took].any()
    assert (warm["plan_score"] >= warm["hold_score"]).all() and (warm["plan_score"][took] > warm["hold_score"][took]).all()
    assert np.array_equal(warm["mean"][took], warm0[took])


def test_the_gpu_cases_are_safe_by_the_reference_alone():
    """On the cases the GPU tests compare bits on, under the strict bounds: at most 10 % of the farms unsafe (a cap) — with the
    seeds chosen, the first of 0, 1, 2, ... that leave none unsafe, none is — and the search does something: the plan never
    scores below the hold and beats it on most farms, candidate 0's score never decreases from one iteration to the next (the
    same paths, the same rows: the same bits again, or a better sequence), winners other than 0 and 1 occur."""
    for name in ("A", "B"):
        c, r = C.case(name), C.reference(name)
        unsafe = int((~r["safe"]).sum())
        print(f"case {name}: {unsafe} of {c['farms']} farms unsafe, smallest margin {r['margin'].min():.2e}, largest strict score "
              f"bound {r['score_bounds'].max():.2e}, median gain over the hold {np.median(r['plan_score'] - r['hold_score']):.3f}")
        assert unsafe <= 0.1 * c["farms"]
        assert unsafe == 0 and C.first_safe_seed(name) == c["seed"] == c["scenario_seed"]  # (what the seeds were chosen for)
        assert np.isfinite(r["margin"]).all() and r["plan"].shape == (c["farms"], c["H"], c["N"])
        assert r["winners"].shape == (len(c["sigma"]), c["farms"]) and r["scores"].shape == (len(c["sigma"]), c["farms"], c["K"])
        assert (r["plan_score"] >= r["hold_score"]).all() and (r["plan_score"] > r["hold_score"] + 100.0 * r["hold_bound"]).mean() > 0.5
        assert np.array_equal(_bits(r["hold_score"]), _bits(r["zero_scores"][0]))
        assert (np.diff(r["zero_scores"], axis=0) >= 0.0).all()
        kept = r["winners"][1:] == 0  # the best so far won again: its score has the bits it won with
        assert np.array_equal(_bits(r["scores"][1:].max(axis=2)[kept]), _bits(r["scores"][:-1].max(axis=2)[kept]))
        assert np.array_equal(_bits(r["plan_score"]), _bits(r["scores"][-1].max(axis=1)))
        assert (r["winners"] >= 2).any() and (np.abs(r["plan"]) <= 5.0).all()
        assert np.array_equal(r["first_action"], r["plan"][:, 0])
        assert r["plan_member_returns"].shape == (c["farms"], c["M"]) and r["wind_paths"].shape == (c["farms"], c["M"], c["H"], 2)
        loose = C.reference(name, strict=False)  # the default mode's bounds: the same plan, wider bounds, smaller margins
        assert np.array_equal(loose["plan"], r["plan"]) and (loose["margin"] <= r["margin"]).all()
        assert (loose["score_bounds"] > r["score_bounds"]).all()


def test_the_limit_shapes_are_safe_and_fill_the_row_limit():
    """The GPU tests' limit shapes, by the reference alone: K M H is the row limit (R N the wide slot's threshold), both farms are safe under the strict bounds
    with a finite margin (something is decided), and the path tile's second tile cannot be reached with K >= 3."""
    assert scenario_ref.MAX_ROWS // 3 < 2048  # M H <= 1365: one tile of member paths
    for name, (K, M, H, *_rest) in C.LIMITS.items():
        r = C.limit_reference(name)
        N = C.limit_case(name)["N"]
        assert K * M * H == scenario_ref.MAX_ROWS if N == 3 else K * M * H * N == 8192, name  # the row limit; the wide slot's threshold
        assert M <= scenario_ref.MAX_MEMBERS and H <= 64, name
        assert r["safe"].all() and np.isfinite(r["margin"]).all(), (name, r["margin"])
        assert (r["plan_score"] >= r["hold_score"]).all() and (r["winners"] >= 2).any(), name


def test_one_still_member_without_risk_weight_is_the_planner():
    """M = 1, an all-zero process, risk_weight 0 and current speeds inside the bounds: the one path is the held wind, the score
    is the return ((1 mean) + (0 cvar), mean = ret / 1), and the reference equals plan_ref.plan(wind=None) bit for bit on case
    A's farms — plan, mean, first action, final yaw, scores and winners."""
    c = plan_cases.case("A")
    args = (c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], c["sigma"], c["seed"], plan_cases.GAMMA,
            plan_cases.LOAD_COEF)
    want = plan_ref.plan(*args)
    got = scenplan_ref.plan(*args, 1, (0.0,) * 5, 123, tail=1, lam=0.0)
    assert ((c["ws"] > 3.0) & (c["ws"] < 28.0)).all()
    for k in ("plan", "mean", "first_action", "final_yaw"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert np.array_equal(_bits(got["plan_score"]), _bits(want["plan_return"]))
    assert np.array_equal(_bits(got["hold_score"]), _bits(want["hold_return"]))
    for k in ("plan_expected", "plan_cvar"):
        assert np.array_equal(_bits(got[k]), _bits(want["plan_return"])), k
    assert np.array_equal(_bits(got["plan_member_returns"][:, 0]), _bits(want["plan_return"]))
    assert np.array_equal(got["winners"], want["winners"]) and np.array_equal(got["safe"], want["safe"])
    assert np.array_equal(_bits(got["wind_paths"][:, 0, :, 0]), _bits(np.repeat(c["ws"][:, None], c["H"], axis=1)))


def test_the_plan_scores_what_the_scenario_reference_scores():
    """Feeding the reference's plan to scenario_ref.scenario under the same scenario seed gives the same wind paths and the
    plan's score, mean, tail mean and member returns, bit for bit."""
    for name in ("A", "B"):
        c, r = C.case(name), C.reference(name)
        s = scenario_ref.scenario(c["x"], c["y"], c["ws"], c["wd"], c["state"], r["plan"][:, None], dict(PARAMS, discrete=False),
                                  C.GAMMA, C.LOAD_COEF, c["M"], C.PROCESS, c["scenario_seed"], c["tail"], c["lam"], c["anchor"], C.BOUNDS)
        assert np.array_equal(_bits(s["wind_paths"]), _bits(r["wind_paths"])), name
        for mine, theirs in (("plan_score", "score"), ("plan_expected", "expected_returns"), ("plan_cvar", "cvar")):
            assert np.array_equal(_bits(r[mine]), _bits(s[theirs][:, 0])), (name, mine)
        assert np.array_equal(_bits(r["plan_member_returns"]), _bits(s["member_returns"][:, 0])), name
        assert np.array_equal(_bits(r["final_yaw"]), _bits(s["final_yaw"][:, 0])), name


def test_margin_counts_only_deciding_pairs_of_different_trajectories():
    """By hand: K = 4, E = 2.  The elite / non-elite pairs and the winner's pairs decide; two candidates of one trajectory do
    not, however close."""
    score = np.array([[4.0, 3.0, 2.9, 1.0]])
    bound = np.full((1, 4), 0.01)
    yaw = np.arange(4, dtype=np.float32).reshape(1, 4, 1, 1)
    elite = plan_ref.ranks(score) < 2
    m = scenplan_ref.margin(score, bound, yaw, elite, np.array([0]))
    assert np.isclose(m[0], 0.1 - 0.02)  # the last elite (3.0) and the first non-elite (2.9)
    same = yaw.copy()
    same[0, 2] = same[0, 1]  # ... walk the same trajectory: the pair ties on both sides; next is the winner and candidate 1
    m = scenplan_ref.margin(score, bound, same, elite, np.array([0]))
    assert np.isclose(m[0], 1.0 - 0.02)
    assert np.isinf(scenplan_ref.margin(score, bound, np.zeros_like(yaw), elite, np.array([0]))[0])
