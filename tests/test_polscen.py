"""CPU: the policy-scenario extension (include/wfpolscen.h) — header, binding table, kernel metadata — and the properties of the
reference and of the cases the GPU tests use (tests/polscen_ref.py: scenario_ref's paths and statistics around policy_ref's
closed loop, over the float64 oracle)."""
import os
import re

import numpy as np
import pytest

import policy_ref
import polscen_ref as sr
from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

KERNELS = ("wf_polscen_paths_kernel", "wf_polscen_returns_kernel", "wf_polscen_stats_kernel")
ENTRY_POINTS = {"wf_polscen_" + n for n in ("create", "destroy", "config", "set_network", "run", "set_timing", "last_timing", "evaluator",
                                            "kernel_info", "last_error")}


def test_polscen_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfpolscen.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.POLSCEN_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.POLSCEN_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.POLICY_ABI, _lib.SCENARIO_ABI, _lib.ROLLSCEN_ABI, _lib.SCENPLAN_ABI):
        assert not set(table) & set(_lib.POLSCEN_ABI)
    assert _lib.POLSCEN_ABI["wf_polscen_set_network"] == _lib.POLICY_ABI["wf_policy_set_network"]  # the policy setter's arguments
    text = open(os.path.join(ROOT, "include", "wfpolscen.h")).read()
    assert "THE PROJECT'S OWN" in text and "PARITY UNPINNED" in text and "ON-THE-FLY" in text and "tests/polscen_ref.py" in text
    assert "include/wfpolicy.h" in text and "include/wfscenario.h" in text  # cited, not restated
    for name, value in (("WF_POLSCEN_KERNELS", 6), ("WF_POLSCEN_MAX_K", 64), ("WF_POLSCEN_MAX_MEMBERS", 64), ("WF_POLSCEN_MAX_H", 64)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "_lib.py")).read()
    assert '"polscen",' in src and '"wfpolscen.h",' in src and "POLSCEN_ABI," in src  # the sources that trigger a rebuild


def test_polscen_kernels_have_no_private_segment(tmp_path):
    """The three kernels of the extension's own, compiled with the Makefile's flags: exactly these, no private segment, no
    spilled register, no out-of-line call, all LDS sized at launch.  The five phases of the closed loop are not among them:
    they are the policy extension's advance kernel (tests/test_policy.py reads its metadata), which this file does not restate."""
    mk = makefile()
    assert "POLSCENOBJ = polscen/wf_polscen_kernels.o polscen/wf_polscen_abi.o" in mk and "$(POLSCENOBJ): %.o: %.hip" in mk
    assert re.search(r"^POLSCENHDRS = .*\$\(POLICYHDRS\)", mk, flags=re.M)
    assert re.search(r"^\$\(OUT\):.*\$\(POLSCENOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*polscen/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("polscen/wf_polscen_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    for m in seen.values():
        assert m["group_segment_fixed_size"] == 0
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "csrc", "polscen", "wf_polscen_kernels.hip")).read()
    assert "wf_staged_row_rewards(" in src and "atomicAdd" not in src
    assert "wf_env_transition(" not in src and "policy_act" not in src  # (the network and the transition exist once, in policy/)
    abi = open(os.path.join(ROOT, "wfcrl-env_amd", "csrc", "polscen", "wf_polscen_abi.hip")).read()
    assert "wfk_launch_policy_advance(" in abi and "wfk_launch_policy_begin(" in abi and "wfk_launch_policy_transpose(" in abi


@pytest.mark.parametrize("name", sr.NAMES)
def test_cases_show_what_they_are_aimed_at(name):
    """On the reference's paths alone: a member path crosses 0 / 360 and a stored speed is clipped where the latent is not; on
    the reference's run: the shapes, a first action that does not depend on the member, and members that differ."""
    s = sr.case(name)
    ref = sr.reference(name)
    B, N, K, M, H = s["B"], s["N"], s["K"], s["M"], s["H"]
    wind, lat = ref["wind_paths"], ref["latent"]
    assert wind.shape == (B, M, H, 2)
    seam = np.concatenate([np.broadcast_to(s["wd"][:, None, None], (B, M, 1)), wind[..., 1]], axis=2)
    lo = s["bounds"][0]
    if M * H > 1:  # (the edge case is one member of one tick)
        assert (np.abs(np.diff(seam, axis=2)) > 180.0).any()      # a stored direction wraps between two ticks
        assert ((lat["y"] < 0.0) | (lat["y"] >= 360.0)).any()     # ... because the latent, which is not wrapped, left [0, 360)
        assert ((wind[..., 0] == lo) & (lat["x"] < lo)).any()     # a stored speed is clipped, its latent is not
    assert (wind[..., 0] >= lo).all() and (wind[..., 1] >= 0.0).all() and (wind[..., 1] < 360.0).all()
    shapes = {"expected_returns": (B, K), "cvar": (B, K), "score": (B, K), "member_returns": (B, K, M), "rewards": (B, K, M, H),
              "farm_power": (B, K, M, H), "actions": (B, K, M, H, N), "observations": (B, K, M, H, 3 * N + 2),
              "final_yaw": (B, K, M, N), "gated": (B, K, M), "first_action": (B, K, N), "best": (B,)}
    for k, shape in shapes.items():
        assert ref[k].shape == shape, k
    assert (ref["actions"][:, :, :, 0] == ref["first_action"][:, :, None]).all()  # observation 0 is the same for every member
    assert (ref["observations"][:, :, :, 0] == ref["observations"][:, :, :1, 0]).all()
    if M > 1:
        assert (ref["member_returns"][:, :, 0] != ref["member_returns"][:, :, 1]).all()
        assert (ref["cvar"] <= ref["expected_returns"] + 1e-12).all() and (ref["cvar"] < ref["expected_returns"]).any()
    if M > 1 and H > 1 and not s["c"]["env"]["discrete"]:
        assert (ref["actions"][:, :, 0, 1:] != ref["actions"][:, :, 1, 1:]).any()  # a feedback law: the members' actions part
    assert np.array_equal(ref["best"], np.argmax(ref["score"], axis=1))


def test_ragged_shapes_are_what_the_gpu_test_needs():
    """7 farms, K M = 15 rows per farm: max_eval_farms = 32 gives chunks of 2 farms and a last one of 1, M C = 10 rows of a
    policy, fewer than a 16-row tile; max_eval_farms = 300 one chunk of 7, M C = 35 rows: three tiles, the last partial."""
    s = sr.case("ragged")
    rows = s["K"] * s["M"]
    assert (s["B"], rows) == (7, 15)
    C = min(32 // rows, s["B"])
    assert C == 2 and s["B"] % C == 1 and s["M"] * C == 10
    C = min(300 // rows, s["B"])
    assert C == 7 and s["M"] * C == 35 and 35 % 16 not in (0,) and -(-35 // 16) == 3
    e = sr.case("edge")
    assert (e["K"], e["M"], e["H"]) == (1, 1, 1)


@pytest.mark.parametrize("base", ("row3_central", "row3_discrete"))
def test_one_still_member_is_the_policy_rollout_under_the_wind_held(base):
    """M = 1 under a still process — every sigma, revert and the ramp 0 — is policy_ref.rollout(wind=None): the path is the
    current wind held and the mean of one member is that member."""
    c = policy_ref.case(base)
    got = sr.rollouts(c, c["ws"], c["wd"], 1, 1, 0.0, sr.STILL, sr.SEED)
    want = policy_ref.rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["params"], c["spec"], c["H"], c["env"], c["gamma"],
                              policy_ref.LOAD_COEF, wind=None)
    held = np.stack([c["ws"], c["wd"]], axis=1)[:, None, None]
    assert np.array_equal(got["wind_paths"], np.broadcast_to(held, got["wind_paths"].shape))
    for k in ("rewards", "farm_power", "actions", "observations", "final_yaw", "gated"):
        assert np.array_equal(got[k][:, :, 0], want[k]), k
    for k in ("member_returns", "expected_returns", "cvar", "score"):
        assert np.array_equal(got[k].reshape(want["returns"].shape), want["returns"]), k
    assert np.array_equal(got["best"], want["best"])
