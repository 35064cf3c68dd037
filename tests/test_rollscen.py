"""CPU: the scenario-rollout extension (include/wfrollscen.h) — header, binding table, kernel metadata — and the properties of
the reference and of the cases the GPU tests use (tests/rollscen_ref.py: scenario_ref's paths and statistics around
rollout_ref's closed loop over the float64 oracle; no new physics)."""
import os
import re

import numpy as np
import pytest

import parity
import rollout_ref as rr
import rollscen_ref as R
import scenario_ref as S
from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

KERNELS = ("wf_rollscen_layout_kernelILb0EE", "wf_rollscen_layout_kernelILb1EE", "wf_rollscen_reduce_kernel")
ENTRY_POINTS = {"wf_rollscen_" + n for n in ("create", "destroy", "config", "run", "set_timing", "last_timing", "evaluator",
                                            "kernel_info", "last_error")}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def test_rollscen_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfrollscen.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.ROLLSCEN_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.ROLLSCEN_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI,
                  _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.SERIES_ABI, _lib.ROLLOUT_ABI, _lib.RETGRAD_ABI, _lib.WINDGEN_ABI,
                  _lib.SCENARIO_ABI, _lib.SCENPLAN_ABI):
        assert not set(table) & set(_lib.ROLLSCEN_ABI)
    # the entry points mirror wfscenario.h name for name
    assert {s.replace("wf_rollscen_", "") for s in syms} == {s.replace("wf_scenario_", "") for s in declared("wfscenario.h")}
    text = open(os.path.join(ROOT, "include", "wfrollscen.h")).read()
    assert "THE PROJECT'S OWN" in text and "PARITY UNPINNED" in text and "tests/rollscen_ref.py" in text
    assert "perfect forecast inside each scenario" in text  # (what a lead >= 1 means under an ensemble is said in the header)
    for name, value in (("WF_ROLLSCEN_KERNELS", 3), ("WF_ROLLSCEN_MAX_K", R.MAX_K), ("WF_ROLLSCEN_MAX_ROWS", R.MAX_ROWS),
                        ("WF_ROLLSCEN_LDS_RECORDS", R.LDS_RECORDS)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name
    # the sources that trigger a rebuild
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "_lib.py")).read()
    assert '"rollscen")' in src and '"wfrollscen.h")' in src and "ROLLSCEN_ABI):" in src


def test_rollscen_kernels_have_no_private_segment(tmp_path):
    """The glue kernels, compiled with the Makefile's flags: exactly these — the lay-out with its brackets in LDS, the lay-out
    with its brackets in global memory, the reduce —, no private segment (a thread holds one turbine: at any N), no spilled
    register, no out-of-line call.  Metadata only.  The look-up is the rose extension's header, the reduce the scenario
    extension's body: ONE definition of each."""
    mk = makefile()
    assert "ROLLSCENOBJ = rollscen/wf_rollscen_kernels.o rollscen/wf_rollscen_abi.o" in mk and "$(ROLLSCENOBJ): %.o: %.hip" in mk
    assert re.search(r"^ROLLSCENHDRS = ", mk, flags=re.M) and "scenario/wf_scenario_reduce.h" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(ROLLSCENOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*rollscen/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("rollscen/wf_rollscen_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    for m in seen.values():
        assert m["group_segment_fixed_size"] == 0  # (all LDS is sized at launch)
    csrc = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    src = open(os.path.join(csrc, "rollscen", "wf_rollscen_kernels.hip")).read()
    assert "wf_rose_lookup.h" in src and "RoseBracket rose_bracket(" not in src
    assert "wf_scenario_reduce.h" in src and "wf_scenario_statistics(a," in src
    scen = open(os.path.join(csrc, "scenario", "wf_scenario_kernels.hip")).read()
    assert "wf_scenario_reduce.h" in scen and "wf_scenario_statistics(a," in scen and "rank +=" not in scen and "rank +=" not in src
    ens = open(os.path.join(csrc, "ensemble", "wf_ensemble.h")).read()  # (the path walk is the ensemble's: the streams are named there)
    assert "wf_ensemble_tiles(" in src and "wf_ensemble_tiles(" in scen and "ensemble/wf_ensemble.h" in mk
    for stream in (S.STREAM_RATE, S.STREAM_WS, S.STREAM_WD):
        assert re.search(r"\b%du\b" % stream, ens) and not re.search(r"\b%du\b" % stream, src), stream


def test_one_still_member_is_the_rollout_under_the_held_wind():
    """One member of a process of all zeros: the path is the current wind at every tick, and every output is
    rollout_ref.rollout's held at the current wind, bit for bit — the statistics of one member are that member."""
    for name in ("row3", "row3_discrete"):
        c = R.case(name)
        r = R.rollscen(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["controllers"], c["tables"], c["H"], c["env"], c["gamma"], 0.1, 1,
                       (0.0, 0.0, 0.0, 0.0, 0.0), 5)
        held = rr.rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["controllers"], c["tables"], c["H"], c["env"], c["gamma"], 0.1)
        B = c["B"]
        assert np.array_equal(r["wind_paths"][..., 0], np.broadcast_to(c["ws"][:, None, None], (B, 1, c["H"])))
        assert np.array_equal(r["wind_paths"][..., 1], np.broadcast_to(c["wd"][:, None, None], (B, 1, c["H"])))
        for k in ("expected_returns", "cvar", "score"):
            assert np.array_equal(_bits(r[k]), _bits(held["returns"])), k
        assert np.array_equal(_bits(r["member_returns"][:, :, 0]), _bits(held["returns"]))
        assert np.array_equal(_bits(r["rewards"][:, :, 0]), _bits(held["rewards"]))
        assert np.array_equal(_bits(r["actions"][:, :, 0]), _bits(held["actions"]))
        assert np.array_equal(_bits(r["final_yaw"][:, :, 0]), _bits(held["final_yaw"]))
        assert np.array_equal(r["gated"][:, :, 0], held["gated_count"]) and np.array_equal(r["best"], held["best"])
        assert np.array_equal(_bits(r["first_action"]), _bits(held["actions"][:, :, 0]))


def test_controllers_that_differ_in_lead_differ_where_the_observation_does():
    """Two controllers that differ only in `lead`, alpha 1 and deadband 0 (the filter is the observation, the target its
    look-up): up to the first step at which min(h + lead, H) selects another observation their actions are the same bits; at
    that step the targets are the look-ups of two different observations.  With lead >= H every step sees obs[H]: leads 5 and
    9 under H = 4 are the same controller."""
    c = R.case("row3")
    H, M = c["H"], c["M"]
    ctl = dict(alpha=[1.0] * 4, deadband=[0.0] * 4, lead=[0, 1, 5, 9], slot=[1] * 4)
    r = R.rollscen(c["x"], c["y"], c["ws"], c["wd"], c["state"], ctl, c["tables"], H, c["env"], c["gamma"], 0.1, M, c["process"], c["seed"],
                   c["tail"], c["lam"], c["anchor"], c["bounds"])
    for k in ("actions", "final_yaw", "rewards", "member_returns"):
        assert np.array_equal(_bits(r[k][:, 2]), _bits(r[k][:, 3])), k  # the clamp
    obs_index = r["members"][0]["obs_index"]
    assert obs_index.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [4, 4, 4, 4], [4, 4, 4, 4]]
    for m in range(M):
        t = r["members"][m]["target"]  # (B, K, H, N) float32, clipped
        # lead 1 at step h looks up what lead 0 looks up at step h + 1: the same observation
        assert np.array_equal(_bits(t[:, 1, :-1]), _bits(t[:, 0, 1:])), m
        assert np.array_equal(_bits(t[:, 2, :]), _bits(np.repeat(t[:, 1, -1:], H, axis=1))), m  # obs[H] at every step
    # step 0: lead 0 sees obs[0] under every member — one action; lead 1 sees its own member's tick 1 — the members differ
    a0 = r["actions"][:, :, :, 0]  # (B, K, M, N)
    assert (_bits(a0[:, 0]) == _bits(a0[:, 0, :1])).all()
    assert (a0[:, 1] != a0[:, 1, :1]).any()
    assert np.array_equal(_bits(r["first_action"]), _bits(a0[:, :, 0]))


def test_paths_are_the_scenario_reference_s_and_do_not_see_the_controllers():
    c = R.case("Turb16_Row5_")
    r = R.reference("Turb16_Row5_")
    pt = S.paths(c["seed"], np.arange(c["B"]), c["M"], c["H"], c["process"], c["ws"], c["wd"], c["anchor"], c["bounds"])
    assert np.array_equal(_bits(r["wind_paths"]), _bits(pt["wind"]))
    assert (pt["x"] != pt["wind"][..., 0]).sum() > 20  # clipped speeds occur
    more = R.reference("row3", 0.1, extra=1)
    base = R.reference("row3", 0.1)
    K = R.case("row3")["K"]
    for k in R.WANT:
        if k not in ("wind_paths", "best"):
            assert np.array_equal(_bits(more[k][:, :K]), _bits(base[k])), k  # a fourth controller changes nothing of the first three
    assert np.array_equal(_bits(more["wind_paths"]), _bits(base["wind_paths"]))


def test_the_cases_show_what_they_are_aimed_at():
    """Counts on the reference alone: closed gates, held and moved turbines, clipped speeds, wrapped directions and the table's
    circular bracket at the seam, members that differ, the clamp, and the two sides of the switch between brackets in LDS and in
    global memory."""
    for name in R.BASE:
        c, r = R.case(name), R.reference(name)
        assert r["gated"].sum() > 0 and (r["gated"] < c["H"] * c["N"]).any(), name
        assert 0.2 < (r["actions"] != (1.0 if c["env"]["discrete"] else 0.0)).mean() < 0.95, name
        assert (r["final_yaw"] != r["final_yaw"][:, :, :1]).any(), name  # feedback: the members end on different yaws
        assert (r["member_returns"].max(axis=2) - r["member_returns"].min(axis=2) > 0).all(), name
        assert max(c["controllers"]["lead"]) > c["H"] or name == "seam"
    c, r = R.case("seam"), R.reference("seam")
    y = r["latent"]["y"]
    assert (y < 0.0).any() and (y >= 360.0).any() and ((r["wind_paths"][..., 1] >= 0.0) & (r["wind_paths"][..., 1] < 360.0)).all()
    assert (r["latent"]["x"] != r["wind_paths"][..., 0]).mean() > 0.2
    assert any(m["circular"].any() for m in r["members"])  # the bracket from the table's last node to its first
    filt = np.stack([m["filt"][..., 1] for m in r["members"]])
    assert (filt < 0.0).any() or (filt >= 360.0).any()  # a filter state is not reduced: the look-up reduces it
    assert (np.abs(c["filter0"][..., 1] - c["wd"][:, None]) > 300.0).all()  # the filter starts across the seam
    rows = {n: R.case(n)["K"] * R.case(n)["M"] * R.case(n)["H"] for n in R.CASES}
    assert all(rows[n] <= R.LDS_RECORDS for n in R.BASE + ("records1024", "chunks")) and rows["records1024"] == R.LDS_RECORDS
    assert all(rows[n] > R.LDS_RECORDS for n in ("records1040", "members64", "controllers64", "steps64"))
    assert all(rows[n] == R.MAX_ROWS for n in ("members64", "controllers64", "steps64"))
    assert [(R.case(n)["K"], R.case(n)["M"], R.case(n)["H"]) for n in ("members64", "controllers64", "steps64")] == [(1, 64, 64), (64, 8, 8), (4, 16, 64)]
    ctl = R.case("controllers64")["controllers"]
    assert len({tuple(float(ctl[f][k]) for f in rr.FIELDS) for k in range(64)}) == 64  # 64 different controllers


@pytest.mark.parametrize("name", list(R.CASES))
def test_best_is_separated_on_every_farm_of_every_case(name):
    """What the seeds were picked for, on the reference alone: on EVERY farm, under both load coefficients, the two best scores
    are further apart than the sum of their two bounds in the default mode (and so in strict mode, whose bounds are smaller) —
    the GPU tests compare `best` with the reference's on every farm and exempt none."""
    c = R.case(name)
    for lc in R.COEFS:
        r = R.reference(name, lc)
        for tol in (parity.TOL, parity.TOL_F64):
            ok = R.clear(r, lc, tol, c["gamma"], c["lam"])
            assert ok.all(), (name, lc, np.flatnonzero(~ok))
