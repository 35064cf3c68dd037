"""GPU: closed-loop rollouts of MLP policies on the device (include/wfpolicy.h) against tests/policy_ref.py.

A closed loop feeds every step's rounding back into the next observation, so the run as a whole is not compared with the
reference's run.  Instead EACH LINK of the loop is checked against the device's OWN upstream values, and no
feedback-sensitivity bound is needed:
  1. observations -> actions: policy_ref's network on the device's observations gives the device's actions bit for bit (relu,
     softsign) or within one float32 ulp (tanh: np.exp against the library's exp_lean, a few float64 ulp); the discrete argmax
     is equal, the reference's two best outputs being further apart than 1e-9 on every turbine (asserted);
  2. actions -> yaw: lookahead_ref's walk of the device's actions gives final_yaw, the yaw block of the observations and gated;
  3. actions -> rewards: lookahead_returns on the device, fed with the device's actions, returns the same bits;
  4. yaw -> local wind, reward (strict): within the step's contract (parity.TOL_F64, carried into the reward by credit_ref.bound
     as tests/test_lookahead_gpu.py carries it) of the oracle solved at the device's yaw of that step.
Cases (tests/policy_ref.py; tests/test_policy.py shows on the reference what each is aimed at): the row of three and
Ablaincourt in both kinds, HornsRev1 x 4 (N = 80, D = 242), hidden widths 5 and 65, 1 to 3 layers, K 1 and 3, H 1 and 5, a
start yaw at a bound, gates that close inside the horizon, a wind per step across 0 / 360, the discrete encoding."""
import functools

import numpy as np
import pytest

import credit_ref
import lookahead_ref
import parity
import policy_links as links
import policy_ref as pr

pytestmark = pytest.mark.gpu

WANT = ("returns", "rewards", "farm_power", "actions", "observations", "final_yaw", "gated", "best")
LA_WANT = links.LA_WANT
MODES = (True, False)
_bits, _same = links.bits, links.same  # (the link checks themselves are tests/policy_links.py's, shared with the wide cases)


def _handle(c, state=True, discrete=None):
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.set_wind(c["ws"], c["wd"])
    w.env_config(load_coef=pr.LOAD_COEF, discrete=c["env"]["discrete"] if discrete is None else discrete, dt=c["env"]["dt"])
    if state:
        w.env_reset()
        w.env_set_state(c["state"])
    return w


def _run(w, c, strict, **kw):
    kw.setdefault("want", WANT)
    kw.setdefault("wind", c["wind"])
    return w.policy_returns(c["params"], c["spec"], c["H"], gamma=c["gamma"], strict=strict, **kw)


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    """(the run, lookahead_returns of every policy's actions on the same handle, the env state before and after)."""
    c = pr.case(name)
    w = _handle(c)
    before = w.env_get_state()
    got = _run(w, c, strict)
    after = w.env_get_state()
    la = [w.lookahead_returns(np.ascontiguousarray(got["actions"][:, k:k + 1]), gamma=c["gamma"], wind=c["wind"], strict=strict, want=LA_WANT)
          for k in range(c["K"])]
    w.close()
    for v in got.values():
        v.setflags(write=False)
    return got, la, before, after


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("name", pr.NAMES)
def test_actions_are_the_network_of_the_observations(name, strict):
    """Link 1, and the shapes and dtypes of every output."""
    c = pr.case(name)
    got = _device(name, strict)[0]
    B, N, K, H = c["B"], c["N"], c["K"], c["H"]
    shapes = {"returns": ((B, K), np.float64), "rewards": ((B, K, H), np.float64), "farm_power": ((B, K, H), np.float64),
              "actions": ((B, K, H, N), np.float32), "observations": ((B, K, H, 3 * N + 2), np.float32),
              "final_yaw": ((B, K, N), np.float32), "gated": ((B, K), np.int32), "best": ((B,), np.int32)}
    for k, (s, d) in shapes.items():
        assert got[k].shape == s and got[k].dtype == d, k
    links.network_link(c, name, got["observations"], got["actions"])
    assert (got["actions"] != (1.0 if c["env"]["discrete"] else 0.0)).mean() > (0.25 if c["env"]["discrete"] else 0.5)  # (the policies move)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("name", pr.NAMES)
def test_yaw_and_gates_are_the_walk_of_the_actions(name, strict):
    """Link 2: lookahead_ref.trajectories of the device's actions gives final_yaw, the yaw block of the observations (step 0:
    the env state; step h: the yaw after step h - 1) and the closed-gate counts, bit for bit.  The free-wind block is the
    wind the row was solved under.  The env state is unchanged by the call."""
    c = pr.case(name)
    got, _, before, after = _device(name, strict)
    gated = links.walk_link(c, got)
    if c["H"] > 1 and name != "row3_shared":
        assert (gated[:, :, 1:] & ~gated[:, :, :-1]).any()  # a gate closes inside the horizon
    for k in before:
        assert np.array_equal(before[k], after[k]), k


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("name", pr.NAMES)
def test_lookahead_of_the_actions_gives_the_same_bits(name, strict):
    """Link 3, oracle-free: lookahead_returns fed with policy k's `actions` under the same wind, in the same mode, returns the
    bits of rewards, farm_power, returns and final_yaw; `best` is the argmax of the device's own returns, the lowest index
    among equals; the return is the discounted sum of the device's own rewards."""
    c = pr.case(name)
    got, la = _device(name, strict)[:2]
    assert len(la) == c["K"]
    links.lookahead_link(name, got, dict(enumerate(la)), strict)
    links.returns_link(c, got)


@pytest.mark.parametrize("name", pr.NAMES)
def test_strict_local_wind_and_rewards_against_the_oracle(name):
    """Link 4: every float64 solve within the step's contract of the oracle at the device's yaw of that step — the local wind
    blocks of the observations under parity.TOL_F64's wind_speed / wind_dir tolerances, every reward and farm power under
    the bound that follows from it."""
    links.oracle_link(pr.case(name), name, _device(name, True)[0])


@pytest.mark.parametrize("discrete", [False, True])
def test_zero_weights_equal_the_lookahead_of_the_constant_sequence(discrete):
    """Weights 0, biases c: the constant action, and the bits of lookahead_returns of that sequence, in both modes."""
    from wfcrl_env_amd import policy as P

    c = pr.case("abl_central")
    N, B, H = c["N"], c["B"], 4
    per = 3 if discrete else 1
    widths = (3 * N + 2, 5, per * N)
    bias = np.array([0.1, 0.7, 0.3] * N, np.float32) if discrete else np.linspace(-6.0, 6.0, N).astype(np.float32)
    vec = np.zeros((1, P.param_count(widths)), np.float32)
    vec[0, -per * N:] = bias
    spec = P.mlp_spec("central", widths, "relu")
    const = np.full(N, 1.0, np.float32) if discrete else bias
    seq = np.ascontiguousarray(np.broadcast_to(const, (B, 1, H, N)), dtype=np.float32)
    w = _handle(c, discrete=discrete)
    for strict in MODES:
        got = w.policy_returns(vec, spec, H, gamma=c["gamma"], wind=c["wind"][:, :H], strict=strict, want=WANT)
        la = w.lookahead_returns(seq, gamma=c["gamma"], wind=c["wind"][:, :H], strict=strict, want=LA_WANT)
        assert np.array_equal(got["actions"], seq)
        for key in LA_WANT:
            assert _same(got[key], la[key]), (discrete, strict, key)
    w.close()


def test_same_bits():
    """Strict: max_eval_farms = 3 K (7 farms in chunks of 3, 3 and a ragged 1) and K (a farm per chunk), a scrambled farm list,
    torch tensors in and out and a second run give all the bits of the whole NumPy run.  Two default-mode runs on one evaluator
    agree bit for bit.  The split timing adds up."""
    import torch

    name = "abl_central"
    c = pr.case(name)
    K = c["K"]
    whole = _device(name, True)[0]
    w = _handle(c)
    again = _run(w, c, True)
    chunks = _run(w, c, True, max_eval_farms=3 * K)
    single = _run(w, c, True, max_eval_farms=K)
    farms = np.array([5, 2, 6, 0], np.int32)
    sub = _run(w, c, True, farms=farms, wind=c["wind"][farms], max_eval_farms=3 * K)
    t = w.policy_returns(torch.from_numpy(c["params"].copy()).cuda(), c["spec"], c["H"], gamma=c["gamma"], wind=c["wind"], strict=True, want=WANT)
    d1, d2 = _run(w, c, False), _run(w, c, False)
    w.policy_timing(detail=True)
    _run(w, c, True, max_eval_farms=3 * K)
    timing = w.policy_timing()
    w.close()
    assert all(v.is_cuda for v in t.values()) and t["best"].dtype == torch.int32 and t["observations"].dtype == torch.float32
    for k in WANT:
        assert _same(again[k], whole[k]), k
        assert _same(chunks[k], whole[k]), k
        assert _same(single[k], whole[k]), k
        assert _same(sub[k], whole[k][farms]), k
        assert _same(t[k].cpu().numpy(), whole[k]), k
        assert _same(d1[k], d2[k]), k
    assert timing["total_ms"] > 0.0 and timing["step_ms"] > 0.0 and timing["glue_ms"] > 0.0
    assert timing["step_ms"] + timing["glue_ms"] <= timing["total_ms"] * 1.05


def test_pending_prev_wind_is_read_and_not_consumed():
    """K = 1 with a speed left by env_set_prev_wind: step 0's reward is normalised by it in two consecutive calls (the first
    did not consume it) — lookahead_returns, which reads the same speed, returns the same bits — and then by the env's own
    step, whose reward lies within the two bounds of rewards[:, 0, 0]; normalised by the current speed it would not."""
    c = pr.case("abl_shared")
    wr = c["ws"] * 1.1
    w = _handle(c)
    w.env_set_prev_wind(wr)
    a = _run(w, c, False)
    b = _run(w, c, False)
    la = w.lookahead_returns(np.ascontiguousarray(a["actions"]), gamma=c["gamma"], want=LA_WANT)
    paid = w.env_step(np.ascontiguousarray(a["actions"][:, 0, 0]), want=("reward",))["reward"].astype(np.float64)
    end = w.env_get_state()
    w.close()
    for k in WANT:
        assert _same(a[k], b[k]), k
    for k in LA_WANT:
        assert _same(a[k], la[k]), k
    ref = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], a["actions"], c["env"], c["gamma"], pr.LOAD_COEF, wr0=wr)
    bound = credit_ref.bound(ref["out"], ref["wr_rows"], pr.LOAD_COEF, parity.TOL)
    assert (np.abs(a["rewards"][:, 0, 0] - paid) <= 2.0 * bound + np.abs(paid) * 2.0 ** -23).all()
    other = credit_ref.reward(ref["out"], c["ws"], pr.LOAD_COEF)
    assert (np.abs(other - ref["rewards"][:, 0, 0]) > 10.0 * bound).all()
    assert np.array_equal(_bits(end["yaw"]), _bits(a["final_yaw"][:, 0]))


def test_series_keyword_on_a_generated_episode():
    """VecWindFarmEnv.policy_returns on a wind_process env: wind="series" equals the call with wind=wind_preview(H), a torch
    module is taken through policy_from_torch, held wind is refused by name, and the env is left as it was."""
    import torch.nn as nn

    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd import policy as P

    process = dict(ws_revert=0.1, ws_sigma=0.4, wd_revert=0.1, wd_sigma=3.0, wd_ramp=2.0, dist=dict(wd_mean=265.0, wd_std=10.0))
    env = envs.make("Ablaincourt_Floris", env_batch=5, max_num_steps=12, load_coef=pr.LOAD_COEF, return_torch=False, wind_process=process)
    N, H = env.num_turbines, 4
    env.reset(seed=11)
    env.step({"yaw": np.full((5, N), 2.0, np.float32)})
    import torch

    torch.manual_seed(5)
    nets = [nn.Sequential(nn.Linear(3, 5), nn.Tanh(), nn.Linear(5, 1), nn.Tanh()) for _ in range(3)]
    kw = dict(kind="shared", out_scale=5.0, shift=[0.0, 8.0, 270.0], scale=[0.05, 0.25, 0.02])
    before = env.get_state()
    preview, avail = env.wind_preview(H)
    assert avail == H and (preview[:, 1:] != preview[:, :-1]).any()
    a = env.policy_returns(nets, H, gamma=0.9, wind="series", want=WANT, **kw)
    b = env.policy_returns(nets, H, gamma=0.9, wind=preview, want=WANT, **kw)
    d = env.fi.policy_returns(*P.policy_from_torch(nets, **kw), H, gamma=0.9, wind=preview, want=WANT)
    sub = env.policy_returns(nets, H, gamma=0.9, wind="series", farms=[3, 1], strict=True, want=WANT, **kw)
    full = env.policy_returns(nets, H, gamma=0.9, wind="series", strict=True, want=WANT, **kw)
    for k in WANT:
        assert _same(a[k], b[k]) and _same(a[k], d[k]), k
        assert _same(sub[k], full[k][[3, 1]]), k
    assert a["returns"].shape == (5, 3) and np.isfinite(a["returns"]).all() and (a["actions"] != 0.0).any()
    with pytest.raises(NotImplementedError, match="time-series"):
        env.policy_returns(nets, H, **kw)
    with pytest.raises(ValueError, match="kind="):
        env.policy_returns(nets, H, wind="series")
    after = env.get_state()
    for k in before:
        x, y = before[k], after[k]
        if isinstance(x, dict):
            assert all(np.array_equal(np.asarray(x[j]), np.asarray(y[j])) for j in x), k
        else:
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), k
    env.close()


def test_vec_env_method_returns_torch():
    """VecWindFarmEnv.policy_returns on a held-wind env that returns torch: CUDA tensors of the stated dtypes with the bits of
    WfStep.policy_returns given NumPy arrays on the same state; a (params, spec) pair and a module give the same."""
    import torch
    import torch.nn as nn

    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd import policy as P

    B, H = 6, 3
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    N = env.num_turbines
    env.reset(seed=0)
    env.step({"yaw": torch.full((B, N), 3.0).cuda()})
    torch.manual_seed(2)
    net = nn.Sequential(nn.Linear(3 * N + 2, 5), nn.Softsign(), nn.Linear(5, N), nn.Softsign())
    kw = dict(kind="central", out_scale=5.0, scale=np.full(3 * N + 2, 0.01))
    r = env.policy_returns(net, H, gamma=0.95, want=WANT, **kw)
    params, spec = P.policy_from_torch(net, **kw)
    pair = env.policy_returns((params, spec), H, gamma=0.95, want=WANT)
    direct = env.fi.policy_returns(params, spec, H, gamma=0.95, want=WANT)
    env.close()
    assert all(v.is_cuda for v in r.values()) and r["returns"].dtype == torch.float64 and r["gated"].dtype == torch.int32
    assert tuple(r["actions"].shape) == (B, 1, H, N) and r["actions"].dtype == torch.float32
    for k in WANT:
        assert _same(r[k].cpu().numpy(), direct[k]) and _same(pair[k].cpu().numpy(), direct[k]), k
    assert (direct["actions"] != 0.0).any()


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd import policy as P
    from wfcrl_env_amd.backend import WfStep
    from yawopt_ref import ROW3

    x, y = ROW3
    N = 3
    spec = P.mlp_spec("shared", (3, 5, 1), "relu")
    vec = np.zeros((2, P.param_count((3, 5, 1))), np.float32)
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.policy_returns(vec, spec, 2)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.policy_returns(vec, spec, 2)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.policy_returns(vec, spec, 2)
    w.env_config()
    w.env_reset()
    w.set_model_sets([{}, {"ambient_ti": 0.1}], [0, 1])
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wake-model parameter sets"):
        w.policy_returns(vec, spec, 2)
    w.set_model_sets([{}], [0, 0])
    w.close()
    w = WfStep(x, y, env_batch=2)
    w.set_wind(8.0, 270.0)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*parameter vector of the wrong length"):
        w.policy_returns(vec[:, :-1], spec, 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..256"):
        w.policy_returns(vec, spec, 257)
    with pytest.raises(ValueError, match="WF_E_INVALID.*K must be in 1..64"):
        w.policy_returns(np.zeros((65, vec.shape[1]), np.float32), spec, 2)
    for gamma in (1.5, float("nan")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.policy_returns(vec, spec, 2, gamma=gamma)
    with pytest.raises(ValueError, match="WF_E_INVALID.*output width does not match"):
        w.policy_returns(np.zeros((2, P.param_count((3, 5, 3))), np.float32), P.mlp_spec("shared", (3, 5, 3), "relu"), 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*input width does not match"):
        w.policy_returns(np.zeros((2, P.param_count((10, 3))), np.float32), P.mlp_spec("central", (10, 3)), 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.policy_returns(vec, spec, 2, max_eval_farms=1)
    with pytest.raises(ValueError, match="farm index out of range"):
        w.policy_returns(vec, spec, 2, farms=[0, 2])
    with pytest.raises(ValueError, match=r"\(n_farms, H, 2\)"):
        w.policy_returns(vec, spec, 2, wind=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="want must name"):
        w.policy_returns(vec, spec, 2, want=("reward",))
    bad = dict(spec, activation="gelu")
    with pytest.raises(ValueError, match="unknown kind or activation"):
        w.policy_returns(vec, bad, 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*scale must be finite"):
        w.policy_returns(vec, dict(spec, scale=np.array([1.0, np.nan, 1.0])), 2)
    with pytest.raises(ValueError, match="WF_E_INVALID.*out_scale must be finite"):
        w.policy_returns(vec, dict(spec, out_scale=float("inf")), 2)
    with pytest.raises(ValueError, match="has not run yet"):
        w.policy_timing()
    r = w.policy_returns(vec, spec, 2, farms=[1], max_eval_farms=2, want=WANT)  # (the handle still serves)
    assert r["returns"].shape == (1, 2) and np.isfinite(r["returns"]).all() and r["best"].tolist() == [0]
    assert (r["actions"] == 0.0).all() and (r["final_yaw"] == 0.0).all()
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_kernel_info_shows_no_scratch_at_80_turbines():
    c = pr.case("horns_central")
    w = _handle(c, state=False)
    info = w.policy_kernel_info()
    w.close()
    assert set(info) == {"transpose", "begin", "advance", "reduce"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
