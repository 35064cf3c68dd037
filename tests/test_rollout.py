"""CPU: the rollout extension (include/wfrollout.h) — header, binding table, kernel metadata — and the properties of the
reference and of the cases the GPU tests use (tests/rollout_ref.py: the closed-loop rollouts of yaw-table controllers restated
in NumPy over the float64 oracle).  Every case shows, with counts, what it is aimed at; the cases that compare `best` and the
order of the returns hold controllers whose returns are pairwise further apart than the sum of their two bounds."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

KERNELS = ("wf_rollout_layout_kernel", "wf_rollout_reduce_kernel")
ENTRY_POINTS = {"wf_rollout_create", "wf_rollout_destroy", "wf_rollout_config", "wf_rollout_set_series", "wf_rollout_run",
                "wf_rollout_set_timing", "wf_rollout_last_timing", "wf_rollout_evaluator", "wf_rollout_kernel_info",
                "wf_rollout_last_error"}
NAMES = ("row3", "row3_discrete", "Ablaincourt_", "HornsRev1_")


def test_rollout_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfrollout.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.ROLLOUT_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.ROLLOUT_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI,
                  _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.SERIES_ABI):
        assert not set(table) & set(_lib.ROLLOUT_ABI)
    # the entry points are the lookahead extension's name for name, plus the series-ahead switch
    assert {s.replace("wf_rollout_", "") for s in syms} == {s.replace("wf_lookahead_", "") for s in declared("wflookahead.h")} | {"set_series"}
    text = open(os.path.join(ROOT, "include", "wfrollout.h")).read()
    assert "PARITY UNPINNED" in text and "ON-THE-FLY" in text and "tests/rollout_ref.py" in text
    for name, value in (("WF_ROLLOUT_KERNELS", 2), ("WF_ROLLOUT_MAX_K", 64), ("WF_ROLLOUT_MAX_H", 1024), ("WF_ROLLOUT_MAX_ROWS", 4096),
                        ("WF_ROLLOUT_MAX_LEAD", 16)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name


def test_rollout_kernels_have_no_private_segment(tmp_path):
    """The two glue kernels, compiled with the Makefile's flags: exactly these two, no private segment, no spilled
    register, no out-of-line call.  Metadata only.  The look-up they compile is the rose extension's header."""
    mk = makefile()
    assert "ROLLOUTOBJ = rollout/wf_rollout_kernels.o rollout/wf_rollout_abi.o" in mk and "$(ROLLOUTOBJ): %.o: %.hip" in mk
    assert re.search(r"^ROLLOUTHDRS = ", mk, flags=re.M)
    assert re.search(r"^\$\(OUT\):.*\$\(ROLLOUTOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*rollout/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("rollout/wf_rollout_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    csrc = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    for hip in ("rollout/wf_rollout_kernels.hip", "rose/wf_rose_kernels.hip"):  # ONE definition of the look-up
        src = open(os.path.join(csrc, hip)).read()
        assert "wf_rose_lookup.h" in src and "RoseBracket rose_bracket(" not in src, hip
    assert "RoseBracket rose_bracket(" in open(os.path.join(csrc, "rose", "wf_rose_lookup.h")).read()


def test_filter_wraps_and_copies():
    """wrap rounds ties to even, the filter takes the short way round the circle, and alpha == 1 copies with no arithmetic."""
    import rollout_ref as rr

    assert rr.wrap(180.0) == 180.0 and rr.wrap(-180.0) == -180.0  # rint(0.5) = 0
    assert rr.wrap(540.0) == -180.0 and rr.wrap(-540.0) == 180.0  # rint(1.5) = 2
    assert rr.wrap(356.0) == -4.0 and rr.wrap(-356.0) == 4.0 and rr.wrap(3.0) == 3.0
    fs, fd = rr.filter_step(np.float64(8.0), np.float64(358.0), 9.0, 2.0, 0.5)
    assert (fs, fd) == (8.5, 360.0)  # 358 + 0.5 * wrap(-356) — not 180, and not reduced: the look-up reduces it
    fs, fd = rr.filter_step(np.float64(8.0), np.float64(1.0), 9.0, 355.0, 0.25)
    assert fd == -0.5
    o = np.float64(0.1) + np.float64(0.2)
    assert rr.filter_step(np.float64(7.0), np.float64(10.0), o, o, 1.0) == (o, o)
    assert rr.filter_step(np.float64(7.0), np.float64(10.0), o, o, np.nextafter(1.0, 0.0)) != (o, o)


@pytest.mark.parametrize("name", NAMES)
def test_untuned_controller_starts_with_the_table_policy(name):
    """alpha 1, deadband 0, lead 0: the step-0 action has the bits of rose_ref.policy at the wind the env holds — in every
    case controller 0 is that controller."""
    import rollout_ref as rr
    import rose_ref

    c, r = rr.case(name), rr.reference(name)
    ctl = c["controllers"]
    assert ctl["alpha"][0] == 1.0 and ctl["deadband"][0] == 0.0 and ctl["lead"][0] == 0
    T, twd, tws, interp = c["tables"][int(ctl["slot"][0])]
    e = c["env"]
    target, action = rose_ref.policy(T, twd, tws, interp, c["ws"], c["wd"], c["state"]["yaw"], e["yaw_lo"], e["yaw_hi"], e["yaw_step"], e["discrete"])
    assert np.array_equal(r["actions"][:, 0, 0].view(np.uint32), action.view(np.uint32))
    assert np.array_equal(r["target"][:, 0, 0].view(np.uint32), target.view(np.uint32))
    assert (action != (1.0 if e["discrete"] else 0.0)).any()  # (the controller moves)


@pytest.mark.parametrize("name", NAMES)
def test_reference_trajectory_is_lookahead_of_its_own_actions(name):
    """The reference's yaw after every step, its gates and its final state are lookahead_ref.trajectories fed with the
    reference's own raw actions: the rollout is the look-ahead of the sequence the controller issues."""
    import lookahead_ref
    import rollout_ref as rr

    c, r = rr.case(name), rr.reference(name)
    yaw, gated, final = lookahead_ref.trajectories(c["state"], r["actions"], c["env"])
    assert np.array_equal(yaw.view(np.uint32), r["yaw"].view(np.uint32)) and np.array_equal(gated, r["gated"])
    assert np.array_equal(final["yaw"].view(np.uint32), r["final_yaw"].view(np.uint32))
    assert np.array_equal(final["acc"].view(np.uint32), r["final"]["acc"].view(np.uint32))
    assert np.array_equal(r["gated_count"], r["gated"].sum(axis=(2, 3)))


def _previous_yaw(c, r):
    y0 = np.broadcast_to(c["state"]["yaw"][:, None, None, :], r["yaw"][:, :, :1].shape)
    return np.concatenate([y0, r["yaw"][:, :, :-1]], axis=2)


@pytest.mark.parametrize("name", NAMES)
def test_cases_show_what_they_are_aimed_at(name):
    """Counts on the reference: the gate closes and (continuous control) opens; the deadband holds turbines that would otherwise move; filters
    with alpha < 1 lag the observation; `lead` clamps at the end of the horizon; both interpolations and (over the cases) both
    encodings; on Ablaincourt_ the filtered direction crosses 0 / 360 and the table's circular bracket is used."""
    import rollout_ref as rr

    c, r = rr.case(name), rr.reference(name)
    ctl, H, K = c["controllers"], c["H"], c["K"]
    g = r["gated"]
    assert g.any(axis=(0, 2, 3)).all() and 0.02 < g.mean() < 0.8  # every controller meets a closed gate, none only closed ones
    assert (g[:, :, 1:] & ~g[:, :, :-1]).any()  # it closes along the horizon ...
    if not c["env"]["discrete"]:  # ... and opens again (in the discrete encoding a closed gate means "down": it moves, and stays closed)
        assert (~g[:, :, 1:] & g[:, :, :-1]).any()
    hold = np.float32(1.0 if c["env"]["discrete"] else 0.0)
    e = r["target"] - _previous_yaw(c, r)
    band = ctl["deadband"][None, :, None, None]
    held = (np.abs(e) <= band) & (e != 0.0)
    assert (r["actions"][held] == hold).all()
    for k in range(K):
        if ctl["deadband"][k] > 0.0:
            assert held[:, k].sum() >= 5, (k, held[:, k].sum())  # the deadband holds turbines a deadband of 0 would move
            if not c["env"]["discrete"]:
                assert (r["actions"][:, k][~held[:, k] & (e[:, k] != 0.0)] != hold).all()
        else:
            assert not held[:, k].any()
    # lead: the observation index, and its clamp at H
    want = np.minimum(np.arange(H)[None, :] + ctl["lead"][:, None], H)
    assert np.array_equal(r["obs_index"], want)
    assert ctl["lead"].max() >= 1 and (np.arange(H)[None, :] + ctl["lead"][:, None] > H).sum() >= 1  # it clamps at the end
    # filters: alpha 1 tracks the observation exactly, alpha < 1 differs from it
    obs = np.concatenate([np.stack([c["ws"], c["wd"]], axis=1)[:, None, :], c["wind"]], axis=1)
    for k in range(K):
        seen = obs[:, r["obs_index"][k]]  # (B, H, 2)
        if ctl["alpha"][k] == 1.0:
            assert np.array_equal(r["filt"][:, k], seen)
        else:
            assert (r["filt"][:, k, 1:] != seen[:, 1:]).mean() > 0.9  # (step 0 of lead 0 observes what the filter starts from)
    assert (ctl["alpha"] < 1.0).any() and (ctl["alpha"] == 1.0).any()
    kinds = {c["tables"][int(s)][3] for s in ctl["slot"]}
    assert kinds == {"linear", "nearest"}
    fd = r["filt"][..., 1]
    if name == "Ablaincourt_":
        assert (fd >= 360.0).sum() >= 10 and (fd < 360.0).sum() >= 10 and r["circular"].sum() >= 10
        assert (np.diff(np.floor(fd / 360.0), axis=2) != 0).sum() >= 3  # the filtered direction crosses north along the horizon
    else:
        assert not r["circular"].any()
    if name == "HornsRev1_":
        assert K * c["N"] > 256 and K * H > 256 and H > 64  # more trajectories than a block's threads, rows past a tile, H past lookahead's


def test_both_encodings_are_covered():
    import rollout_ref as rr

    assert {rr.case(n)["env"]["discrete"] for n in NAMES} == {False, True}
    d = rr.reference("row3_discrete")["actions"]
    assert set(np.unique(d).tolist()) == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("name", NAMES)
def test_returns_are_further_apart_than_their_bounds(name):
    """The condition on the inputs under which `best` and the order of the returns can be compared: on every farm the
    controllers' returns are pairwise further apart than the sum of their two bounds (credit_ref.bound carried through the
    discounted sum) — the default-mode bounds, hence the strict ones too.  No two controllers share a trajectory."""
    import parity
    import rollout_ref as rr

    c, r = rr.case(name), rr.reference(name)
    K = c["K"]
    for tol in (parity.TOL, parity.TOL_F64):
        rb = rr.bounds(r, rr.LOAD_COEF, tol, c["gamma"])[2]
        ratio = min((np.abs(r["returns"][:, i] - r["returns"][:, j]) / (rb[:, i] + rb[:, j])).min() for i in range(K) for j in range(i + 1, K))
        print(f"{name}: smallest |return_i - return_j| / (bound_i + bound_j) = {ratio:.1f} under {'TOL' if tol is parity.TOL else 'TOL_F64'}")
        assert ratio > 2.0
    for i in range(K):
        for j in range(i + 1, K):
            assert (r["yaw"][:, i] != r["yaw"][:, j]).any(axis=(1, 2)).all(), (i, j)
    assert np.array_equal(r["best"], np.argmax(r["returns"], axis=1))


def test_series_case_holds_its_last_row():
    """The series-ahead case: 4 rows are left of a horizon of 6 — entries 4 and 5 of every farm's window repeat entry 3 —, the
    rows differ along the window, and the farms see different windows (their start rows differ)."""
    import rollout_ref as rr

    c, r = rr.series_case(), rr.series_reference()
    H, avail = c["H"], c["available"]
    assert avail == c["T"] - c["t"] - 1 == 4 < H
    rows = c["rows"]
    assert (rows[:, avail:] == rows[:, avail - 1:avail]).all() and (rows[:, 1:avail] != rows[:, :avail - 1]).any(axis=2).all()
    assert len({rows[b].tobytes() for b in range(c["B"])}) == c["B"]
    assert r["gated"].any() and not r["gated"].all() and (r["actions"] != 0.0).any()
    assert np.array_equal(r["obs_index"][2], np.minimum(np.arange(H) + 1, H))  # controller 2 previews one step
    # step 0 is normalised by the CURRENT speed: the reference was given it
    assert np.array_equal(r["wr_rows"].reshape(c["B"], c["K"], H)[:, :, 0], np.repeat(c["ws"][:, None], c["K"], axis=1))


def test_controller_grid():
    """WfStep.controller_grid: the full grid, alpha slowest and lead fastest, and the index -> parameters map."""
    from wfcrl_env_amd.backend import WfStep

    ctl, params = WfStep.controller_grid([1.0, 0.5], [0.0, 2.5, 5.0], [0, 1], slot=2)
    assert len(params) == 12 and all(v.shape == (12,) for v in ctl.values())
    assert ctl["slot"].dtype == np.int32 and ctl["alpha"].dtype == np.float64 and ctl["deadband"].dtype == np.float32 and ctl["lead"].dtype == np.int32
    assert params[0] == {"slot": 2, "alpha": 1.0, "deadband": 0.0, "lead": 0} and params[1]["lead"] == 1 and params[2]["deadband"] == 2.5
    assert params[6] == {"slot": 2, "alpha": 0.5, "deadband": 0.0, "lead": 0}
    for i, p in enumerate(params):
        assert all(ctl[k][i] == p[k] for k in p)
