"""CPU: the scenario extension (include/wfscenario.h) — header, binding table, kernel metadata — and the properties of the
reference the GPU tests use (tests/scenario_ref.py: member paths, statistics and the bound carry restated in NumPy over
lookahead_ref and the float64 oracle)."""
import os
import re

import numpy as np

import parity
import scenario_ref as S
from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

KERNELS = ("wf_scenario_layout_kernel", "wf_scenario_reduce_kernel")
ENTRY_POINTS = {"wf_scenario_" + n for n in ("create", "destroy", "config", "run", "set_timing", "last_timing", "evaluator",
                                            "kernel_info", "last_error")}


def test_scenario_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfscenario.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.SCENARIO_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.SCENARIO_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI,
                  _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.SERIES_ABI, _lib.ROLLOUT_ABI, _lib.RETGRAD_ABI, _lib.WINDGEN_ABI):
        assert not set(table) & set(_lib.SCENARIO_ABI)
    # the entry points mirror wflookahead.h name for name
    assert {s.replace("wf_scenario_", "") for s in syms} == {s.replace("wf_lookahead_", "") for s in declared("wflookahead.h")}
    text = open(os.path.join(ROOT, "include", "wfscenario.h")).read()
    assert "THE PROJECT'S OWN" in text and "PARITY UNPINNED" in text and "tests/scenario_ref.py" in text
    assert "streams 16, 17 and 18" in text and "NO OTHER KERNEL" in text
    for name, value in (("WF_SCENARIO_KERNELS", 2), ("WF_SCENARIO_MAX_MEMBERS", S.MAX_MEMBERS), ("WF_SCENARIO_MAX_ROWS", S.MAX_ROWS)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name


def test_scenario_kernels_have_no_private_segment(tmp_path):
    """The two glue kernels, compiled with the Makefile's flags: exactly these two, no private segment, no spilled
    register, no out-of-line call.  Metadata only.  The streams they draw from are named by the ensemble's header, which the
    kernel file takes through its own (tests/test_ensemble.py: by no other file)."""
    mk = makefile()
    assert "SCENARIOOBJ = scenario/wf_scenario_kernels.o scenario/wf_scenario_abi.o" in mk and "$(SCENARIOOBJ): %.o: %.hip" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(SCENARIOOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*scenario/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("scenario/wf_scenario_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    csrc = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    src = open(os.path.join(csrc, "scenario", "wf_scenario_kernels.hip")).read()
    ens = open(os.path.join(csrc, "ensemble", "wf_ensemble.h")).read()
    for stream in (S.STREAM_RATE, S.STREAM_WS, S.STREAM_WD):
        assert re.search(r"\b%du\b" % stream, ens) and not re.search(r"\b%du\b" % stream, src), stream
    for header in ("../wf_philox.h", "../ext/wf_deviate.h", "../ext/wf_ext_kernels.h"):
        assert '#include "%s"' % header in ens, header
    assert '#include "wf_scenario.h"' in src and "wf_ensemble_tiles(" in src
    own = open(os.path.join(csrc, "scenario", "wf_scenario.h")).read()
    assert '#include "../ext/wf_ext_kernels.h"' in own and '#include "../ensemble/wf_ensemble.h"' in own


def test_zero_sigmas_and_zero_ramp_are_the_held_wind_in_every_member():
    """With a process that does not move and no anchor every member's path is the current wind at every tick, and every
    member's rewards and return are lookahead_ref's under the held wind, bit for bit; mean, tail mean and score are then
    that return too (two equal terms: r + r, / 2 and 0.5 r + 0.5 r are exact)."""
    import lookahead_ref

    x, y, ws, wd, state, actions, _ = S.gpu_case("row3")
    params = dict(S.PARAMS, discrete=False)
    for process in ((0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.0, 0.7, 0.0, 0.0)):  # (reverting to where it is does not move it either)
        r = S.scenario(x, y, ws, wd, state, actions, params, S.GAMMA, 0.1, 2, process, 5, tail=2, lam=0.5)
        held = lookahead_ref.lookahead(x, y, ws, wd, state, actions, params, S.GAMMA, 0.1)
        assert np.array_equal(r["wind_paths"][..., 0], np.broadcast_to(ws[:, None, None], (len(ws), 2, S.H)))
        assert np.array_equal(r["wind_paths"][..., 1], np.broadcast_to(wd[:, None, None], (len(ws), 2, S.H)))
        for m in range(2):
            assert np.array_equal(r["rewards"][:, :, m], held["rewards"]) and np.array_equal(r["member_returns"][:, :, m], held["returns"])
        for k in ("expected_returns", "cvar", "score"):
            assert np.array_equal(r[k], held["returns"]), k
        assert np.array_equal(r["best"], held["best"]) and np.array_equal(r["final_yaw"].view(np.uint32), held["final_yaw"].view(np.uint32))


def test_paths_depend_on_seed_farm_member_process_anchor_and_bounds_only():
    """Not on K (the paths never see the actions), not on the batch size, not on a farm list: farm b of a list has the paths
    of farm b of the whole batch.  Members, farms, seeds, anchors and bounds do tell paths apart."""
    ws, wd, anchor, whole = S.edge_case()
    e = S.EDGE
    args = (e["M"], e["H"], e["process"])
    farms = np.random.default_rng(3).permutation(e["B"])[:9]
    sub = S.paths(e["seed"], farms, *args, ws[farms], wd[farms], anchor[farms], e["bounds"])
    for k in ("wind", "x", "y", "rate"):
        assert np.array_equal(sub[k], whole[k][farms]), k
    few = S.paths(e["seed"], np.arange(e["B"]), 7, 5, e["process"], ws, wd, anchor, e["bounds"])  # fewer members, fewer ticks: a prefix
    assert np.array_equal(few["wind"], whole["wind"][:, :7, :5])
    w = whole["wind"]
    assert (w[:, 0, :, 1] != w[:, 1, :, 1]).all()  # members differ (the directions: a clipped speed is the bound in both)
    same_wind = S.paths(e["seed"], [0, 1], *args, ws[:1].repeat(2), wd[:1].repeat(2), anchor[:1].repeat(2, axis=0), e["bounds"])
    assert (same_wind["y"][0] != same_wind["y"][1]).all() and (same_wind["x"][0] != same_wind["x"][1]).all()  # farms differ under one wind
    other = S.paths(e["seed"] + 1, np.arange(e["B"]), *args, ws, wd, anchor, e["bounds"])
    assert (other["x"] != whole["x"]).all() and (other["y"] != whole["y"]).all()
    moved = S.paths(e["seed"], np.arange(e["B"]), *args, ws, wd, anchor + [0.5, 10.0], e["bounds"])
    assert (moved["x"] != whole["x"]).all() and (moved["y"] != whole["y"]).all()
    wide = S.paths(e["seed"], np.arange(e["B"]), *args, ws, wd, anchor, (1.0, 30.0))
    assert np.array_equal(wide["x"], whole["x"]) and (wide["wind"][..., 0] != w[..., 0]).any()  # (the latent is not clipped)
    # the speed's deviate is stream 17's, the direction's stream 18's, the ramp's stream 16's — by hand for one entry
    import plan_ref
    import wind_ref

    b, m, p = 3, 2, S.process_of(e["process"])
    r = plan_ref.philox4x32_10(e["seed"], np.uint64((b << 32) | m), 16)
    rate = p["wd_ramp"] * (2.0 * wind_ref.u01(r[..., 0], r[..., 1]) - 1.0)
    assert rate == whole["rate"][b, m] and abs(rate) < p["wd_ramp"]
    x1 = (ws[b] + p["ws_revert"] * (anchor[b, 0] - ws[b])) + p["ws_sigma"] * plan_ref.deviate(e["seed"], b, m * 64, 17)
    y1 = (wd[b] + p["wd_revert"] * ((anchor[b, 1] + rate * 1.0) - wd[b])) + p["wd_sigma"] * plan_ref.deviate(e["seed"], b, m * 64, 18)
    assert x1 == whole["x"][b, m, 0] and y1 == whole["y"][b, m, 0]


def test_clipped_speeds_and_wrapped_directions_occur_in_the_test_inputs():
    """The edge case — current winds and anchors at the circle's seam and at the speed bounds — stores clipped speeds on
    both bounds and directions wrapped from below 0 and from 360 and above, by whole turns too; the base cases store
    clipped speeds on every 32-farm input and wrapped directions on the row of three (a farm at 0 degrees)."""
    _, _, _, pt = S.edge_case()
    lo, hi = S.EDGE["bounds"]
    x, y, w = pt["x"], pt["y"], pt["wind"]
    assert 0.1 < (x < lo).mean() < 0.5 and 0.1 < (x > hi).mean() < 0.5
    assert np.array_equal(w[..., 0], np.clip(x, lo, hi)) and (w[..., 0][x < lo] == lo).all() and (w[..., 0][x > hi] == hi).all()
    assert 0.1 < (y < 0.0).mean() < 0.5 and 0.1 < (y >= 360.0).mean() < 0.5
    assert ((w[..., 1] >= 0.0) & (w[..., 1] < 360.0)).all()
    turns = np.round((y - w[..., 1]) / 360.0)
    assert np.abs(y - (w[..., 1] + 360.0 * turns)).max() < 1e-9 and turns.min() <= -1 and turns.max() >= 1
    clipped = wrapped = 0
    for name in S.NAMES:
        r = S.gpu_ref(name, 0.1)
        c = (r["latent"]["x"] != r["wind_paths"][..., 0]).sum()
        assert c > 0 or name == "row3", name
        clipped += c
        wrapped += (r["latent"]["y"] != r["wind_paths"][..., 1]).sum()
    assert clipped > 100 and wrapped > 0
    assert (S.gpu_ref("row3", 0.1)["latent"]["y"] < 0.0).any()


def test_statistics_orders_ranks_and_ties():
    """Mean in ascending m, ranks by (return, m) — a count —, the tail in ascending rank, on hand-made tables where another
    order gives other bits; equal members keep their order; tail = 1 is the minimum, tail = M the mean up to the order."""
    t = np.array([[[1e16, 1.0, -1e16, 1.0], [3.0, 1.0, 2.0, 1.0]]])
    s = S.statistics(t, 2, 0.25)
    assert s["expected_returns"].tolist() == [[1.0 / 4.0, 7.0 / 4.0]]  # ascending m: ((1e16 + 1) - 1e16) + 1 = 1
    assert s["ranks"].tolist() == [[[3, 1, 0, 2], [3, 0, 2, 1]]]  # the two 1.0 by index
    assert s["sorted"].tolist() == [[[-1e16, 1.0, 1.0, 1e16], [1.0, 1.0, 2.0, 3.0]]]
    assert s["cvar"].tolist() == [[(-1e16 + 1.0) / 2.0, 1.0]]
    assert s["score"][0, 1] == (0.75 * 1.75) + (0.25 * 1.0) and s["best"].tolist() == [1]
    r = np.random.default_rng(2).normal(size=(6, 7, 9))
    lo, full = S.statistics(r, 1, 1.0), S.statistics(r, 9, 0.0)
    assert np.array_equal(lo["cvar"], r.min(axis=2)) and np.array_equal(lo["score"], lo["cvar"])
    assert np.array_equal(full["score"], full["expected_returns"])  # (weight 0: the mean's bits)
    assert np.abs(full["cvar"] - full["expected_returns"]).max() <= 9 * 2.0 ** -52 * np.abs(r).sum(axis=2).max() / 9
    assert np.array_equal(np.sort(r, axis=2), full["sorted"])
    one = S.statistics(r[:, :, :1], 1, 0.5)
    for k in ("expected_returns", "cvar"):
        assert np.array_equal(one[k], r[:, :, 0]), k
    dup = np.concatenate([r[:, 2:3], r[:, 2:3]], axis=1)
    assert (S.statistics(dup, 3, 0.4)["best"] == 0).all()  # equal scores: the lower index


def test_the_reference_separates_what_the_gpu_tests_check():
    """On the reference alone, for every base case and load coefficient: the spread of the scores within a farm is at least
    50 median score bounds in the default mode (more in strict), so that a wrong order, normaliser or member mix-up cannot
    hide; and at least three quarters of the farms have a top-two gap beyond the two strict bounds — what SEED was picked
    for.  A member mix-up is visible: members' returns of one sequence differ by far more than the bounds."""
    for name in S.NAMES:
        for lc in (0.1, 1.0):
            r = S.gpu_ref(name, lc)
            sc = r["score"]
            rows = np.arange(sc.shape[0])
            for tol in (parity.TOL, parity.TOL_F64):
                c = S.carry(r, lc, tol, S.GAMMA, S.LAM)
                assert np.median(sc.max(axis=1) - sc.min(axis=1)) >= 50.0 * np.median(c["score"]), (name, lc)
            order = np.argsort(-sc, axis=1, kind="stable")
            first, second = order[:, 0], order[:, 1]
            clear = sc[rows, first] - sc[rows, second] > c["score"][rows, first] + c["score"][rows, second]
            assert clear.mean() >= 0.75, (name, lc, clear.mean())
            mr = r["member_returns"]
            assert np.median(mr.max(axis=2) - mr.min(axis=2)) > 50.0 * np.median(S.carry(r, lc, parity.TOL, S.GAMMA, S.LAM)["member_returns"])
