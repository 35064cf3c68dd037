"""CPU: the lookahead extension (include/wflookahead.h) — header, binding table, kernel metadata — and the properties of the
reference the GPU tests use (tests/lookahead_ref.py: the look-ahead returns restated in NumPy over the float64 oracle)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile
from yawopt_ref import ROW3

KERNELS = ("wf_lookahead_layout_kernel", "wf_lookahead_reduce_kernel")
ENTRY_POINTS = {"wf_lookahead_create", "wf_lookahead_destroy", "wf_lookahead_config", "wf_lookahead_run", "wf_lookahead_set_timing",
                "wf_lookahead_last_timing", "wf_lookahead_evaluator", "wf_lookahead_kernel_info", "wf_lookahead_last_error"}
PARAMS = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1)


def test_lookahead_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wflookahead.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.LOOKAHEAD_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.LOOKAHEAD_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI):
        assert not set(table) & set(_lib.LOOKAHEAD_ABI)
    # the entry points mirror wfcredit.h name for name
    assert {s.replace("wf_lookahead_", "") for s in syms} == {s.replace("wf_credit_", "") for s in declared("wfcredit.h")}
    text = open(os.path.join(ROOT, "include", "wflookahead.h")).read()
    assert "PARITY UNPINNED" in text and "ON-THE-FLY" in text and "tests/lookahead_ref.py" in text
    for name, value in (("WF_LOOKAHEAD_KERNELS", 2), ("WF_LOOKAHEAD_MAX_H", 64), ("WF_LOOKAHEAD_MAX_ROWS", 4096)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name


def test_lookahead_kernels_have_no_private_segment(tmp_path):
    """The two glue kernels, compiled with the Makefile's flags: exactly these two, no private segment, no spilled
    register, no out-of-line call.  Metadata only."""
    mk = makefile()
    assert "LOOKAHEADOBJ = lookahead/wf_lookahead_kernels.o lookahead/wf_lookahead_abi.o" in mk and "$(LOOKAHEADOBJ): %.o: %.hip" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(LOOKAHEADOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*lookahead/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("lookahead/wf_lookahead_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text


def _state(rng, B, N):
    moves = rng.integers(0, 6, B)
    acc = (rng.uniform(0.0, 3.6, (B, N)) * (moves[:, None] + 1)).astype(np.float32)  # the gate closes at 1.8 (moves + 1)
    return {"yaw": rng.uniform(-40.0, 40.0, (B, N)).astype(np.float32), "acc": acc, "moves": moves}


def test_one_step_one_sequence_is_the_credit_reference():
    """K = 1, H = 1: the return, the reward and the farm power are credit_ref.counterfactual's row 0 for an ACTION base — the
    transition applied by the caller, as tests/test_credit_gpu.py does — bit for bit, with a normalising speed of its own."""
    import credit_ref
    import lookahead_ref

    x, y = ROW3
    rng = np.random.default_rng(4)
    B, N = 6, 3
    ws, wd = rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B)
    wr = ws * 1.1
    state = _state(rng, B, N)
    for discrete in (False, True):
        params = dict(PARAMS, discrete=discrete)
        actions = (rng.integers(0, 3, (B, N)) if discrete else rng.uniform(-7.0, 7.0, (B, N))).astype(np.float32)
        base = credit_ref.transition(state["yaw"], state["acc"], state["moves"], actions, params)
        cf = credit_ref.counterfactual(x, y, ws, wd, base, base[:, :, None], 0.1, wr=wr)
        la = lookahead_ref.lookahead(x, y, ws, wd, state, actions[:, None, None, :], params, 0.9, 0.1, wr0=wr)
        assert la["returns"].shape == (B, 1) and la["rewards"].shape == (B, 1, 1) and la["final_yaw"].dtype == np.float32
        assert np.array_equal(la["final_yaw"][:, 0].view(np.uint32), base.view(np.uint32))
        assert np.array_equal(la["rewards"][:, 0, 0], cf["reward"][:, 0]) and np.array_equal(la["returns"][:, 0], cf["reward"][:, 0])
        assert np.array_equal(la["farm_power"][:, 0, 0], cf["farm_power"][:, 0])
        assert (la["best"] == 0).all() and la["gated"].any() and not la["gated"].all()


@pytest.mark.parametrize("continuous", [True, False])
def test_reference_trajectory_is_the_host_mdp_plus_gate(continuous):
    """lookahead_ref.trajectories against H successive steps of the package's host env — FarmEpisode.over_budget (the gate,
    zeroing the raw action) on the MDP's own accumulator, then WindFarmMDP.get_controlled_state_transition — from random
    states with open and closed gates: the yaw after every step and the final accumulator, bit for bit in both encodings."""
    import lookahead_ref
    from helpers import OracleFlorisInterface
    from wfcrl_env_amd.env_core import FarmEpisode
    from wfcrl_env_amd.environments.data_cases import named_cases_dictionary

    case = named_cases_dictionary["Turb3_Row1_"][1].clone()
    ep = FarmEpisode(OracleFlorisInterface, case, {"yaw": (-40, 40, 5)}, continuous, None, 0, 10, 0.1)
    params = dict(PARAMS, dt=float(case.dt), discrete=not continuous)
    rng = np.random.default_rng(13)
    B, K, H, N = 24, 2, 5, 3
    state = _state(rng, B, N)
    state["yaw"][:4] = np.float32([38.0, -38.0, 40.0])  # the setpoint clip takes
    state["acc"][4:8] = 0.0
    actions = (rng.uniform(-7.0, 7.0, (B, K, H, N)) if continuous else rng.integers(0, 3, (B, K, H, N))).astype(np.float32)
    yaw, gated, final = lookahead_ref.trajectories(state, actions, params)
    assert yaw.shape == (B, K, H, N) and yaw.dtype == np.float32 and final["acc"].dtype == np.float32
    assert (final["moves"] == state["moves"][:, None] + H).all()
    for b in range(B):
        for k in range(K):
            ep.mdp._actuation_accumulator["yaw"] = state["acc"][b].copy()
            cur = state["yaw"][b].copy()
            for h in range(H):
                a = actions[b, k, h].copy()
                blocked = ep.over_budget("yaw", ep.mdp.get_accumulated_actions()["yaw"], int(state["moves"][b]) + 1 + h)
                a[blocked] = 0.0
                assert np.array_equal(blocked, gated[b, k, h]), (b, k, h)
                cur = np.asarray(ep.mdp.get_controlled_state_transition({"yaw": cur}, {"yaw": a})["yaw"], np.float32)
                assert np.array_equal(cur.view(np.uint32), yaw[b, k, h].view(np.uint32)), (b, k, h)
            acc = np.asarray(ep.mdp.get_accumulated_actions()["yaw"], np.float32)
            assert np.array_equal(acc.view(np.uint32), final["acc"][b, k].view(np.uint32)), (b, k)
    assert gated.any() and (~gated).any() and not gated[4:8, :, 0].any()
    assert gated[:, :, 1:].any() and (gated[:, :, 0] != gated[:, :, -1]).any()  # (the gate moves along the horizon)


def test_discount_and_summation_order():
    """g_0 = 1, g_h = g_{h-1} gamma, and ret = sum_h g_h r_h added in ascending h from 0.0, on a hand-made table where
    another order or gamma ** h gives other bits."""
    import lookahead_ref

    g = lookahead_ref.discounts(0.9, 6)
    want, v = [], 1.0
    for _ in range(6):
        want.append(v)
        v = v * 0.9
    assert g.tolist() == want and g[0] == 1.0
    assert (g != 0.9 ** np.arange(6)).any()  # (repeated products are not the powers, in the last bits)
    table = np.array([[1e16, 1.0, -1e16, 1.0], [1.0, 1.0, 1e16, -1e16], [0.1, 0.2, 0.3, 0.4]])
    assert lookahead_ref.discounted(table, 1.0).tolist() == [1.0, 2.0, ((0.1 + 0.2) + 0.3) + 0.4]  # (descending h: 0.0, 2.0)
    r = table[2]
    by_hand = ((0.0 + 1.0 * r[0]) + 0.9 * r[1]) + (0.9 * 0.9) * r[2]
    by_hand = by_hand + ((0.9 * 0.9) * 0.9) * r[3]
    assert lookahead_ref.discounted(table, 0.9)[2] == by_hand
    assert lookahead_ref.discounted(table, 0.0).tolist() == [1e16, 1.0, 0.1]  # gamma = 0: the first reward alone
    assert lookahead_ref.discounted(np.zeros((2, 3, 1)), 0.5).shape == (2, 3)
