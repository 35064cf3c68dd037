"""CPU: the policy extension (include/wfpolicy.h) — header, binding table, kernel metadata, the torch conversion — and the
properties of the reference and of the cases the GPU tests use (tests/policy_ref.py: the closed-loop rollouts of MLP policies
restated in NumPy over the float64 oracle)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

KERNELS = ("wf_policy_transpose_kernel", "wf_policy_begin_kernel", "wf_policy_advance_kernel", "wf_policy_reduce_kernel")
ENTRY_POINTS = {"wf_policy_" + n for n in ("create", "destroy", "config", "set_network", "run", "set_timing", "last_timing", "evaluator",
                                           "kernel_info", "last_error")}


def test_policy_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfpolicy.h")
    assert set(syms) == ENTRY_POINTS
    assert set(_lib.POLICY_ABI) == set(syms)
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert getattr(lib, s).argtypes == _lib.POLICY_ABI[s][1]  # bound by load()
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.ROLLOUT_ABI, _lib.ROLLSCEN_ABI, _lib.CALIB_ABI):
        assert not set(table) & set(_lib.POLICY_ABI)
    text = open(os.path.join(ROOT, "include", "wfpolicy.h")).read()
    assert "THE PROJECT'S OWN" in text and "PARITY UNPINNED" in text and "ON-THE-FLY" in text and "tests/policy_ref.py" in text
    for name, value in (("WF_POLICY_KERNELS", 4), ("WF_POLICY_MAX_H", 256), ("WF_POLICY_MAX_K", 64), ("WF_POLICY_MAX_LAYERS", 4),
                        ("WF_POLICY_MAX_WIDTH", 256)):
        assert re.search(r"^#define %s %d$" % (name, value), text, flags=re.M), name
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "_lib.py")).read()
    assert '"policy",' in src and '"wfpolicy.h",' in src and "POLICY_ABI," in src  # the sources that trigger a rebuild


def test_policy_kernels_have_no_private_segment(tmp_path):
    """The four glue kernels, compiled with the Makefile's flags: exactly these, no private segment (nothing is sized by N or
    by a width: at any N), no spilled register, no out-of-line call, all LDS sized at launch.  Metadata only.  The reward tile
    is the extensions' shared one."""
    mk = makefile()
    assert "POLICYOBJ = policy/wf_policy_kernels.o policy/wf_policy_abi.o" in mk and "$(POLICYOBJ): %.o: %.hip" in mk
    assert re.search(r"^POLICYHDRS = ", mk, flags=re.M)
    assert re.search(r"^\$\(OUT\):.*\$\(POLICYOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*policy/\*\.o", mk, flags=re.M)
    seen, text = compile_kernels("policy/wf_policy_kernels.hip", tmp_path)
    assert_no_private_segment(seen, KERNELS)
    assert "s_swappc_b64" not in text
    for m in seen.values():
        assert m["group_segment_fixed_size"] == 0
    src = open(os.path.join(ROOT, "wfcrl-env_amd", "csrc", "policy", "wf_policy_kernels.hip")).read()
    assert "wf_staged_row_rewards(" in src and "wf_env_transition(" in src and "atomicAdd(&ng" in src
    assert not re.search(r"atomicAdd\((?!&ng)", src)  # (the one atomic is the integer gate count in LDS)


def _sequential(widths, act, final, seed):
    import torch
    import torch.nn as nn

    torch.manual_seed(seed)
    mods = []
    acts = {"relu": nn.ReLU, "tanh": nn.Tanh, "softsign": nn.Softsign}
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(nn.Linear(a, b))
        if l < len(widths) - 2:
            mods.append(acts[act]())
    if final:
        mods.append(acts[final]())
    return nn.Sequential(*mods)


@pytest.mark.parametrize("act", ["relu", "tanh", "softsign"])
@pytest.mark.parametrize("widths", [(3 * 7 + 2, 5, 65, 7), (3 * 7 + 2, 7)])
def test_reference_mlp_agrees_with_torch(act, widths):
    """The reference's network against a float64 torch.nn.Sequential holding the same float32 parameters, on CPU: 1e-12
    relative on every output, hidden activation and final activation both `act` (relu: no final)."""
    import torch

    import policy_ref as pr
    from wfcrl_env_amd import policy as P

    final = None if act == "relu" else act
    net = _sequential(widths, act, final, seed=3)
    params, spec = P.policy_from_torch(net, "central")
    assert spec["widths"] == widths and spec["final"] == final and (len(widths) == 2 or spec["activation"] == act)
    obs = np.random.default_rng(4).uniform(-3.0, 3.0, (9, widths[0])).astype(np.float32)
    want = net.double()(torch.from_numpy(obs).double()).detach().numpy()
    got = pr.mlp(params[0], spec, obs)
    assert got.shape == want.shape and got.dtype == np.float64
    assert (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0)).all(), np.abs(got - want).max()
    # the normalisation: shift and scale are applied before the first layer
    spec2 = P.mlp_spec("central", widths, spec["activation"], final, shift=np.full(widths[0], 0.5), scale=np.full(widths[0], 2.0))
    want2 = net(torch.from_numpy((obs.astype(np.float64) - 0.5) * 2.0)).detach().numpy()
    assert (np.abs(pr.mlp(params[0], spec2, obs) - want2) <= 1e-12 * np.maximum(np.abs(want2), 1.0)).all()


def test_policy_from_torch_is_parameters_to_vector_and_refuses_by_name():
    import torch
    import torch.nn as nn

    from wfcrl_env_amd import policy as P

    nets = [_sequential((5, 8, 4, 1), "tanh", "softsign", seed=s) for s in (0, 1, 2)]
    params, spec = P.policy_from_torch(nets, "shared", out_scale=5.0, use_freewind=True)
    assert params.shape == (3, P.param_count((5, 8, 4, 1))) and params.dtype == np.float32
    for k, net in enumerate(nets):
        assert np.array_equal(params[k], nn.utils.parameters_to_vector(net.parameters()).detach().numpy())
    assert spec["kind"] == "shared" and spec["widths"] == (5, 8, 4, 1) and spec["activation"] == "tanh" and spec["final"] == "softsign"
    assert spec["out_scale"] == 5.0 and spec["use_freewind"] and (spec["shift"] == 0.0).all() and (spec["scale"] == 1.0).all()
    one, _ = P.policy_from_torch(nets[1], "shared", use_freewind=True)
    assert np.array_equal(one, params[1:2])
    with pytest.raises(ValueError, match="share one architecture"):
        P.policy_from_torch([nets[0], _sequential((5, 8, 1), "tanh", None, 0)], "shared", use_freewind=True)
    with pytest.raises(ValueError, match="unsupported module"):
        P.policy_from_torch(nn.Sequential(nn.Linear(3, 4), nn.Sigmoid(), nn.Linear(4, 1)), "shared")
    with pytest.raises(ValueError, match="share one activation"):
        P.policy_from_torch(nn.Sequential(nn.Linear(3, 4), nn.ReLU(), nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 1)), "shared")
    with pytest.raises(ValueError, match="two Linear layers follow each other"):
        P.policy_from_torch(nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 1)), "shared")
    with pytest.raises(ValueError, match="needs a bias"):
        P.policy_from_torch(nn.Sequential(nn.Linear(3, 1, bias=False)), "shared")
    with pytest.raises(ValueError, match="not ReLU"):
        P.policy_from_torch(nn.Sequential(nn.Linear(3, 1), nn.ReLU()), "shared")
    with pytest.raises(ValueError, match="input width is 3, or 5"):
        P.policy_from_torch(nn.Sequential(nn.Linear(4, 1)), "shared")
    with pytest.raises(ValueError, match="nn.Sequential"):
        P.policy_from_torch(nn.Linear(3, 1), "shared")
    with pytest.raises(ValueError, match="1..4 layers"):
        P.mlp_spec("central", (5, 4, 4, 4, 4, 2))
    with pytest.raises(ValueError, match="hidden width at most 256"):
        P.mlp_spec("central", (5, 257, 2))
    with pytest.raises(ValueError, match="unknown activation"):
        P.mlp_spec("central", (5, 2), activation="gelu")
    with pytest.raises(ValueError, match="must be finite"):
        P.mlp_spec("central", (5, 2), scale=np.array([1.0, np.inf, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match='"central" or "shared"'):
        P.mlp_spec("decentral", (5, 2))
    assert torch.is_tensor(next(nets[0].parameters()))  # (the modules are left as they were)


@pytest.mark.parametrize("discrete", [False, True])
def test_zero_weights_issue_the_constant_action_and_equal_the_lookahead(discrete):
    """Weights 0 and biases c: every action is float32(c) (discrete: the index of the largest bias), whatever is observed, and
    the rollout IS lookahead_ref's look-ahead of that constant sequence: rewards, farm power, returns, final yaw, exactly."""
    import lookahead_ref
    import policy_ref as pr
    from wfcrl_env_amd import policy as P

    c = pr.case("row3_central")
    N, B, H = c["N"], c["B"], 4
    per = 3 if discrete else 1
    widths = (3 * N + 2, 5, per * N)
    bias = np.array([0.1, 0.7, 0.3] * N, np.float32) if discrete else np.array([2.5, -1.25, 7.0], np.float32)
    vec = np.zeros(P.param_count(widths), np.float32)
    vec[-per * N:] = bias
    spec = P.mlp_spec("central", widths, "relu")
    env = dict(c["env"], discrete=discrete)
    r = pr.rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], vec[None], spec, H, env, 0.9, 0.1, wind=c["wind"][:, :H])
    const = np.full(N, 1.0, np.float32) if discrete else bias
    assert (r["actions"] == const).all()
    seq = np.broadcast_to(const, (B, 1, H, N)).astype(np.float32)
    la = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], seq, env, 0.9, 0.1, wind=c["wind"][:, :H])
    for k in ("returns", "rewards", "farm_power"):
        assert np.array_equal(r[k], la[k]), k
    assert np.array_equal(r["final_yaw"].view(np.uint32), la["final_yaw"].view(np.uint32))
    assert np.array_equal(r["gated"], la["gated"].sum(axis=(2, 3))) and np.array_equal(r["yaw"].view(np.uint32), la["yaw"].view(np.uint32))


@pytest.mark.parametrize("name", ["row3_central", "row3_shared", "row3_discrete", "abl_central", "abl_shared", "abl_linear", "horns_central"])
def test_cases_show_what_they_are_aimed_at(name):
    """Counts on the reference alone: the policies move the turbines and differ from each other; a gate closes inside the
    horizon; a turbine starts at the yaw bound; the per-step wind crosses 0 / 360; the observation of step h + 1 holds the
    yaw after step h; a discrete turbine's two best outputs are further apart than 1e-9 on EVERY turbine; the reference's
    trajectory is lookahead_ref's walk of its own actions."""
    import lookahead_ref
    import policy_ref as pr

    c, r = pr.case(name), pr.reference(name)
    B, N, K, H = c["B"], c["N"], c["K"], c["H"]
    hold = np.float32(1.0 if c["env"]["discrete"] else 0.0)
    assert (r["actions"] != hold).mean() > (0.25 if c["env"]["discrete"] else 0.5)  # (the policies move the turbines)
    yaw, gated, final = lookahead_ref.trajectories(c["state"], r["actions"], c["env"])
    assert np.array_equal(yaw.view(np.uint32), r["yaw"].view(np.uint32)) and np.array_equal(final["yaw"].view(np.uint32), r["final_yaw"].view(np.uint32))
    assert np.array_equal(gated.sum(axis=(2, 3)), r["gated"])
    assert (c["state"]["yaw"][:, 0] == 40.0).all()
    assert np.array_equal(r["observations"][:, :, 0, :N], np.broadcast_to(c["state"]["yaw"][:, None], (B, K, N)))
    if H > 1:
        assert np.array_equal(r["observations"][:, :, 1:, :N], r["yaw"][:, :, :-1])
        assert gated.any() and (~gated).any()
        if name != "row3_shared":  # (its softsign output moves three turbines too gently to fill a budget in five steps)
            assert (gated[:, :, 1:] & ~gated[:, :, :-1]).any(), "no gate closes inside the horizon"
    if K > 1:
        assert all((r["actions"][:, i] != r["actions"][:, j]).any() for i in range(K) for j in range(i + 1, K))
    if c["wind"] is not None:
        d = c["wind"][:, :, 1]
        assert ((d[:, 1:] < d[:, :-1]) & (d[:, :-1] > 350.0)).any(axis=1).all()  # every farm's direction wraps along the horizon
        assert np.array_equal(r["observations"][:, 0, 1:, 3 * N], c["wind"][:, :-1, 0].astype(np.float32))
    if c["env"]["discrete"]:
        assert set(np.unique(r["actions"]).tolist()) <= {0.0, 1.0, 2.0} and len(np.unique(r["actions"])) == 3
        print(f"{name}: smallest gap between a turbine's two best outputs: {r['margin'].min():.3e}")
        assert (r["margin"] > 1e-9).all()
    if name == "horns_central":
        assert N == 80 and c["spec"]["widths"][0] == 242 and B == 4


def test_layer_and_width_coverage():
    import policy_ref as pr

    specs = [pr.case(n)["spec"] for n in pr.NAMES]
    assert {len(s["widths"]) - 1 for s in specs} >= {1, 3} and {w for s in specs for w in s["widths"][1:-1]} == {5, 65}
    assert {pr.case(n)["K"] for n in pr.NAMES} == {1, 3} and {pr.case(n)["H"] for n in pr.NAMES} == {1, 5}
    assert {s["kind"] for s in specs} == {"central", "shared"} and {s["activation"] for s in specs} == {"relu", "softsign", "tanh"}
