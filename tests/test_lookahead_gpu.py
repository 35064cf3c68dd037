"""GPU: multi-step look-ahead returns on the device (include/wflookahead.h) against tests/lookahead_ref.py — the same
trajectories, rows, rewards and returns in NumPy over the float64 oracle.

The bounds need no measured number.  The step's contract is per turbine (tests/parity.py), carried through the reward's
formula by credit_ref.bound / power_bound per ROW — TOL_F64 when every row is solved in float64 (strict), TOL in the handle's
default mode; a return is held to sum_h g_h bound_h, on EVERY entry; nothing is exempted.

Inputs: the row of three under four winds and 32 farms of three layouts (yawopt_ref.gpu_input), N = 3 to 16; K = 8 sequences
of H = 4 steps, gamma 0.9, load_coef 0.1 and 1.0; actions from default_rng(61), uniform in [-5, 5] (continuous) or integers
{0, 1, 2} (discrete), sequence 0 all-hold; the env state set with env_set_state: yaw uniform in [-20, 20], acc uniform in
[0, 30], moves in 1..5, under env_config(dt=180) (rate 0.3 deg/s, budget 0.1: the gate is closed where
acc >= 5.4 (moves + 1)), so gates are closed from step 0 on and open along the horizon as the counter grows.  Checked on
the CPU with the oracle (`_ref` and the tests assert what matters): closed gates on 8 % to 13 % of the (row, turbine)
entries (17 % to 31 % with the discrete actions), 17 % to 32 % at step 0; the spread of the returns within a farm (median 0.15 to 0.26) is hundreds of default-mode
bounds (about 1e-3) and tens of thousands of strict ones (about 5e-6), so a wrong order, discount, normaliser or
substitution cannot hide; in strict mode the top two returns of every farm are further apart than the sum of their bounds
(8 times at the least).  (Under the default dt of 60 s the same state closes 70 % of the gates, whole farms hold still in
every sequence and their returns tie: nothing to tell sequences apart by.)

Bit identity across chunk sizes and farm lists is asserted in STRICT mode, where every row is solved by the float64 kernel,
whose bits do not depend on the batch; in the default mode only two runs on the same evaluator are compared
(tests/test_credit_gpu.py: test_same_bits)."""
import functools

import numpy as np
import pytest

import credit_ref
import lookahead_ref
import parity
import yawopt_ref
from yawopt_ref import ROW3

pytestmark = pytest.mark.gpu

NAMES = ("row3", "Ablaincourt_", "Turb6_Row2_", "Turb16_Row5_")
COEFS = (0.1, 1.0)
WANT = ("returns", "rewards", "farm_power", "final_yaw", "best")
K, H, GAMMA = 8, 4, 0.9
PARAMS = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=180.0, budget=0.1)


def _freeze(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            elif isinstance(v, dict):
                _freeze(v)


@functools.lru_cache(maxsize=None)
def _case(name):
    """An input: layout, winds, env state, the continuous and the discrete actions."""
    x, y, ws, wd = yawopt_ref.gpu_input(name)
    B, N = len(ws), len(x)
    rng = np.random.default_rng(61)
    state = {"yaw": rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32), "acc": rng.uniform(0.0, 30.0, (B, N)).astype(np.float32),
             "moves": rng.integers(1, 6, B).astype(np.int32)}
    cont = rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
    cont[:, 0] = 0.0
    disc = rng.integers(0, 3, (B, K, H, N)).astype(np.float32)
    disc[:, 0] = 1.0
    actions = {False: cont, True: disc}
    _freeze(state, actions)
    return x, y, ws, wd, state, actions


@functools.lru_cache(maxsize=None)
def _ref(name, discrete, lc):
    x, y, ws, wd, state, actions = _case(name)
    r = lookahead_ref.lookahead(x, y, ws, wd, state, actions[discrete], dict(PARAMS, discrete=discrete), GAMMA, lc)
    g = r["gated"]
    assert 0.15 < g[:, :, 0].mean() < 0.5 and 0.05 < g.mean() < 0.6  # closed gates from step 0 on, and open ones
    _freeze(r)
    return r


def _handle(name, lc, discrete=False, state=True):
    from wfcrl_env_amd.backend import WfStep

    x, y, ws, wd, st = _case(name)[:5]
    w = WfStep(x, y, env_batch=len(ws))
    w.set_wind(ws, wd)
    w.env_config(load_coef=lc, discrete=discrete, dt=PARAMS["dt"])
    if state:
        w.env_reset()
        w.env_set_state(st)
    return w


@functools.lru_cache(maxsize=None)
def _device(name, strict, lc, discrete=False):
    w = _handle(name, lc, discrete)
    r = w.lookahead_returns(_case(name)[5][discrete], gamma=GAMMA, strict=strict, want=WANT)
    w.close()
    _freeze(r)
    return r


def _bounds(ref, lc, tol, gamma=GAMMA):
    """(reward bound (B, K, H), farm-power bound (B, K, H), return bound (B, K) = sum_h g_h bound_h)."""
    shape = ref["rewards"].shape
    b = credit_ref.bound(ref["out"], ref["wr_rows"], lc, tol).reshape(shape)
    pb = credit_ref.power_bound(ref["out"], tol).reshape(shape)
    return b, pb, (lookahead_ref.discounts(gamma, shape[2]) * b).sum(axis=2)


def _check(name, strict, tol):
    for lc in COEFS:
        ref, got = _ref(name, False, lc), _device(name, strict, lc)
        B, N = ref["final_yaw"].shape[0], ref["final_yaw"].shape[2]
        assert got["returns"].shape == (B, K) and got["returns"].dtype == np.float64
        assert got["rewards"].shape == (B, K, H) and got["rewards"].dtype == np.float64
        assert got["farm_power"].shape == (B, K, H) and got["farm_power"].dtype == np.float64
        assert got["final_yaw"].shape == (B, K, N) and got["final_yaw"].dtype == np.float32
        assert got["best"].shape == (B,) and got["best"].dtype == np.int32
        b, pb, rb = _bounds(ref, lc, tol)
        er, ep, et = (np.abs(got[k] - ref[k]) for k in ("rewards", "farm_power", "returns"))
        spread = np.median(ref["returns"].max(axis=1) - ref["returns"].min(axis=1))
        label = f"{name} {'strict' if strict else 'default mode'} load_coef {lc}"
        print(f"{label}: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}, return "
              f"{(et / rb).max():.3f}; median spread of the returns {spread:.2e}, median return bound {np.median(rb):.2e}")
        assert spread > 50.0 * np.median(rb)  # (what is checked is far larger than what is allowed)
        assert (er <= b).all(), (label, (er / b).max())
        assert (ep <= pb).all(), (label, (ep / pb).max())
        assert (et <= rb).all(), (label, (et / rb).max())
        # the return is the discounted sum of the device's OWN rewards, bit for bit
        assert np.array_equal(got["returns"], lookahead_ref.discounted(got["rewards"], GAMMA))


@pytest.mark.parametrize("name", NAMES)
def test_strict_against_the_reference(name):
    """Every row solved in float64: every row's reward and farm power and every return inside the bounds that follow from
    TOL_F64, with both load coefficients."""
    _check(name, True, parity.TOL_F64)


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_against_the_reference(name):
    """The handle's own resolve mode: the same inequalities from TOL.  Nothing is exempted."""
    _check(name, False, parity.TOL)


@pytest.mark.parametrize("discrete", [False, True])
def test_final_yaw_has_the_bits_of_the_reference(discrete):
    """The yaw after step H - 1 of every sequence: the bits of the reference's float32 trajectory in both encodings — the
    gate, the accumulator and the counter are visible here without any tolerance (a sequence whose gate state the device got
    wrong at any step ends elsewhere).  Sequence 0 holds: continuous control stays at the state; a closed gate turns the
    discrete hold into "down"."""
    for name in NAMES:
        ref, got = _ref(name, discrete, 0.1), _device(name, False, 0.1, discrete)
        assert np.array_equal(got["final_yaw"].view(np.uint32), ref["final_yaw"].view(np.uint32)), name
        state = _case(name)[4]
        moved = (ref["final_yaw"] != state["yaw"][:, None, :])
        assert moved[:, 1:].any()
        if discrete:
            assert np.array_equal(moved[:, 0], ref["gated"][:, 0].any(axis=1))
        else:
            assert not moved[:, 0].any()


@pytest.mark.parametrize("strict", [True, False])
def test_best(strict):
    """The reference return of the device's choice is no lower than the reference maximum minus the sum of the two sequences'
    bounds, on every farm; in strict mode, where the top two reference returns of every farm are further apart than the
    sum of their bounds (asserted), it IS the reference's argmax.  The device's choice is the argmax of its own returns."""
    tol = parity.TOL_F64 if strict else parity.TOL
    for name in NAMES:
        for lc in COEFS:
            ref, got = _ref(name, False, lc), _device(name, strict, lc)
            rb = _bounds(ref, lc, tol)[2]
            B = rb.shape[0]
            rows = np.arange(B)
            best, top = got["best"], ref["best"]
            assert ((best >= 0) & (best < K)).all()
            assert np.array_equal(best, np.argmax(got["returns"], axis=1))
            assert (ref["returns"][rows, best] >= ref["returns"][rows, top] - (rb[rows, best] + rb[rows, top])).all(), (name, lc)
            if strict:
                order = np.argsort(-ref["returns"], axis=1, kind="stable")
                first, second = order[:, 0], order[:, 1]
                gap = ref["returns"][rows, first] - ref["returns"][rows, second]
                assert (gap > rb[rows, first] + rb[rows, second]).all(), (name, lc)  # (the reference alone)
                assert np.array_equal(best, top), (name, lc)


def test_equal_sequences_the_lower_index_wins():
    """Three sequences per farm — hold, the reference's best, the reference's best AGAIN — in strict mode: sequences 1 and 2
    have the same returns bit for bit, and the choice is never 2; where the best beats holding by more than the bounds it is 1.
    All-equal sequences: 0."""
    name, lc = "Ablaincourt_", 0.1
    ref = _ref(name, False, lc)
    actions = _case(name)[5][False]
    B = actions.shape[0]
    rows = np.arange(B)
    top = actions[rows, ref["best"]]
    three = np.stack([actions[:, 0], top, top], axis=1)
    rb = _bounds(ref, lc, parity.TOL_F64)[2]
    w = _handle(name, lc)
    got = w.lookahead_returns(three, gamma=GAMMA, strict=True, want=("returns", "best"))
    same = w.lookahead_returns(np.stack([top] * 5, axis=1), gamma=GAMMA, strict=True, want=("returns", "best"))
    w.close()
    assert np.array_equal(got["returns"][:, 1], got["returns"][:, 2])
    assert (got["best"] != 2).all()
    clear = ref["returns"][rows, ref["best"]] - ref["returns"][:, 0] > rb[rows, ref["best"]] + rb[:, 0]
    assert clear.any() and (got["best"][clear] == 1).all() and (got["best"][ref["best"] == 0] == 0).all()
    assert (same["returns"] == same["returns"][:, :1]).all() and (same["best"] == 0).all()


@pytest.mark.parametrize("discrete", [False, True])
def test_one_sequence_is_what_the_env_then_does(discrete):
    """K = 1 under the held wind, with a speed left by env_set_prev_wind: the call leaves the state as it was
    (env_get_state before and after compare equal); then H real env_step calls on the same handle — final_yaw is the yaw
    state after them, bit for bit; rewards[h] is within the sum of the two bounds (the env's and the row's, both
    credit_ref.bound under TOL, plus the rounding of the env's float32 reward) of the reward the env paid at step h; step 0
    of both is normalised by the pending speed, which the look-ahead did not consume."""
    name, lc = "Turb6_Row2_", 0.1
    x, y, ws, wd, state, actions = _case(name)
    seq = actions[discrete][:, 3:4]  # (B, 1, H, N)
    wr = ws * 1.1
    ref = lookahead_ref.lookahead(x, y, ws, wd, state, seq, dict(PARAMS, discrete=discrete), GAMMA, lc, wr0=wr)
    b = _bounds(ref, lc, parity.TOL)[0][:, 0]
    w = _handle(name, lc, discrete)
    w.env_set_prev_wind(wr)
    before = w.env_get_state()
    got = w.lookahead_returns(seq, gamma=GAMMA, want=WANT)
    after = w.env_get_state()
    paid = []
    for h in range(H):
        paid.append(w.env_step(seq[:, 0, h].copy(), want=("reward",))["reward"].astype(np.float64))
    end = w.env_get_state()
    w.close()
    for k in before:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], np.asarray(state[k]).reshape(before[k].shape)), k
    assert np.array_equal(got["final_yaw"][:, 0].view(np.uint32), end["yaw"].view(np.uint32))
    assert np.array_equal(end["yaw"].view(np.uint32), ref["final_yaw"][:, 0].view(np.uint32))
    assert np.array_equal(end["acc"].view(np.uint32), ref["final"]["acc"][:, 0].view(np.uint32)) and (end["moves"] == state["moves"] + H).all()
    paid = np.stack(paid, axis=1)  # (B, H)
    err = np.abs(got["rewards"][:, 0] - paid)
    allow = 2.0 * b + np.abs(paid) * 2.0 ** -23
    print(f"discrete={discrete}: largest |look-ahead reward - env reward| / allowed: {(err / allow).max():.3f}")
    assert (err <= allow).all()
    assert (np.abs(got["rewards"][:, 0] - ref["rewards"][:, 0]) <= b).all()
    # the pending speed counts: normalised by the current speed, step 0's reward would be far outside the bound
    other = credit_ref.reward(ref["out"], np.repeat(ws, H), lc).reshape(-1, H)[:, 0]
    assert (np.abs(other - ref["rewards"][:, 0, 0]) > 10.0 * b[:, 0]).all()


def test_wind_per_step():
    """wind= equal to the held wind gives the bits of wind=None (strict); a horizon whose speed changes at h = 2 — and whose
    direction turns at h = 3 — agrees with the reference on every row, step 2 normalised by the speed of step 1 and step 3
    by the new one: with another normaliser those rewards are far outside the bound (asserted on the reference)."""
    name, lc = "Turb6_Row2_", 0.1
    x, y, ws, wd, state, actions = _case(name)
    act = actions[False]
    B = len(ws)
    held = np.stack([np.repeat(ws[:, None], H, axis=1), np.repeat(wd[:, None], H, axis=1)], axis=2)
    wind = held.copy()
    wind[:, 2:, 0] *= 1.2
    wind[:, 3, 1] += 4.0
    ref = lookahead_ref.lookahead(x, y, ws, wd, state, act, dict(PARAMS, discrete=False), GAMMA, lc, wind=wind)
    b, pb, rb = _bounds(ref, lc, parity.TOL_F64)
    w = _handle(name, lc)
    none = w.lookahead_returns(act, gamma=GAMMA, strict=True, want=WANT)
    same = w.lookahead_returns(act, gamma=GAMMA, wind=held, strict=True, want=WANT)
    got = w.lookahead_returns(act, gamma=GAMMA, wind=wind, strict=True, want=WANT)
    w.close()
    for k in WANT:
        assert np.array_equal(none[k], same[k]), k
        assert np.array_equal(none[k], _device(name, True, lc)[k]), k
    assert (np.abs(got["rewards"] - ref["rewards"]) <= b).all() and (np.abs(got["farm_power"] - ref["farm_power"]) <= pb).all()
    assert (np.abs(got["returns"] - ref["returns"]) <= rb).all()
    assert np.array_equal(got["final_yaw"], none["final_yaw"])  # (the transition does not see the wind)
    wrong = credit_ref.reward(ref["out"], np.repeat(wind[:, None, :, 0], K, axis=1).reshape(-1), lc).reshape(B, K, H)  # the step's OWN speed
    assert (np.abs(wrong - ref["rewards"])[:, :, 2] > 10.0 * b[:, :, 2]).all()
    assert np.array_equal(wrong[:, :, 3], ref["rewards"][:, :, 3])  # (step 3: the speed before it is its own)


def test_same_bits():
    """Strict: max_eval_farms = K H + 1 (a farm per chunk) and 3 K H + 1 (32 farms in chunks of 3 and a ragged 2), a shuffled
    sub-list of farms and torch tensors in and out give all the bits of the whole NumPy run.  Two default-mode runs on one evaluator agree bit for bit."""
    import torch

    name, lc = "Ablaincourt_", 0.1
    act = _case(name)[5][False]
    B = act.shape[0]
    whole = _device(name, True, lc)
    kw = dict(gamma=GAMMA, strict=True, want=WANT)
    w = _handle(name, lc)
    again = w.lookahead_returns(act, **kw)
    chunks = w.lookahead_returns(act, max_eval_farms=3 * K * H + 1, **kw)
    single = w.lookahead_returns(act, max_eval_farms=K * H + 1, **kw)
    farms = np.random.default_rng(5).permutation(B)[:13]
    sub = w.lookahead_returns(act[farms], farms=farms, **kw)
    t = w.lookahead_returns(torch.from_numpy(act.copy()).cuda(), **kw)
    out = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda")}
    t0 = w.lookahead_returns(torch.from_numpy(act.copy()).cuda(), gamma=GAMMA, strict=True, want="returns", out=out)
    d1, d2 = w.lookahead_returns(act, gamma=GAMMA, want=WANT), w.lookahead_returns(act, gamma=GAMMA, want=WANT)
    timing = w.lookahead_timing()
    w.close()
    assert all(v.is_cuda for v in t.values()) and t0["returns"] is out["returns"] and set(t0) == {"returns"}
    assert t["best"].dtype == torch.int32 and t["final_yaw"].dtype == torch.float32
    for k in WANT:
        assert np.array_equal(again[k], whole[k]), k
        assert np.array_equal(chunks[k], whole[k]), k
        assert np.array_equal(single[k], whole[k]), k
        assert np.array_equal(sub[k], whole[k][farms]), k
        assert np.array_equal(t[k].cpu().numpy(), whole[k]), k
        assert np.array_equal(d1[k], d2[k]), k
    assert np.array_equal(t0["returns"].cpu().numpy(), whole["returns"])
    assert timing["total_ms"] > 0.0


def test_refusals_name_their_cause():
    """Each refusal carries its code and a message, and nothing is launched: the handle still serves afterwards."""
    from wfcrl_env_amd.backend import WfStep

    x, y = ROW3
    N = 3
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts (set_layouts)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*several layouts"):
        w.lookahead_returns(np.zeros((2, 2, 2, N), np.float32))
    w.close()
    w = WfStep(x, y, env_batch=2)
    zero = np.zeros((2, 2, 2, N), np.float32)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no wind"):
        w.lookahead_returns(zero)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.lookahead_returns(zero)
    w.env_config()
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
        w.lookahead_returns(np.zeros((2, 1, 65, N), np.float32))
    with pytest.raises(ValueError, match="WF_E_INVALID.*K H <= 4096"):
        w.lookahead_returns(np.zeros((2, 4097, 1, N), np.float32))
    with pytest.raises(ValueError, match="WF_E_INVALID.*K H <= 4096"):
        w.lookahead_returns(np.zeros((2, 241, 17, N), np.float32))  # 4097 rows
    for gamma in (1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
            w.lookahead_returns(zero, gamma=gamma)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows"):
        w.lookahead_returns(zero, max_eval_farms=3)  # K H = 4
    with pytest.raises(ValueError, match="farm index out of range"):
        w.lookahead_returns(zero, farms=[0, 2])
    with pytest.raises(ValueError, match=r"\(n_farms, K, H, num_turbines\)"):
        w.lookahead_returns(zero[:1])
    with pytest.raises(ValueError, match=r"\(n_farms, K, H, num_turbines\)"):
        w.lookahead_returns(zero[:, :, :, :2])
    with pytest.raises(ValueError, match=r"\(n_farms, H, 2\)"):
        w.lookahead_returns(zero, wind=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="want must name"):
        w.lookahead_returns(zero, want=("reward",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.lookahead_timing()
    up = zero.copy()
    up[:, 1] = 5.0
    r = w.lookahead_returns(up[:1], farms=[1], max_eval_farms=4, want=WANT)  # (the handle still serves)
    assert r["returns"].shape == (1, 2) and np.isfinite(r["returns"]).all() and r["best"].tolist() in ([0], [1])
    # from the reset state: the first 5 deg pass, and fill the budget (5 / 0.3 / 2 / 60 = 0.14 >= 0.1): the second step is gated
    assert r["final_yaw"][0, 0].tolist() == [0.0] * N and r["final_yaw"][0, 1].tolist() == [5.0] * N
    full = w.lookahead_returns(np.zeros((2, 4096, 1, N), np.float32), strict=True, want=("best", "returns"))  # the largest K; every sequence holds
    assert full["best"].tolist() == [0, 0] and (full["returns"] == full["returns"][:, :1]).all()
    assert w.step(np.zeros((2, N), np.float32))["power"].shape == (2, N)
    w.close()


def test_vec_env_method():
    """VecWindFarmEnv.lookahead_returns after reset(seed=0) and two steps: shapes and dtypes, agreement with
    WfStep.lookahead_returns on the same state, a farm list, and the env left as it was."""
    import torch
    from wfcrl_env_amd import environments as envs

    B, Kv, Hv = 8, 5, 3
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20)
    N = env.num_turbines
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        env.step({"yaw": (torch.rand((B, N), generator=gen) * 10.0 - 5.0).cuda()})
    seqs = (torch.rand((B, Kv, Hv, N), generator=gen) * 10.0 - 5.0).cuda()
    before = env.get_state()
    r = env.lookahead_returns({"yaw": seqs}, gamma=0.95)
    assert set(r) == {"returns", "rewards", "final_yaw", "best"} and all(v.is_cuda for v in r.values())
    assert tuple(r["returns"].shape) == (B, Kv) and r["returns"].dtype == torch.float64
    assert tuple(r["rewards"].shape) == (B, Kv, Hv) and r["rewards"].dtype == torch.float64
    assert tuple(r["final_yaw"].shape) == (B, Kv, N) and r["final_yaw"].dtype == torch.float32
    assert tuple(r["best"].shape) == (B,) and r["best"].dtype == torch.int32
    direct = env.fi.lookahead_returns(seqs, gamma=0.95, want=("returns", "rewards", "final_yaw", "best"))
    for k in r:
        assert torch.equal(r[k], direct[k]), k
    assert torch.equal(r["best"].long(), r["returns"].argmax(dim=1))
    strict = env.lookahead_returns(seqs, gamma=0.95, strict=True)
    sub = env.lookahead_returns(seqs, gamma=0.95, farms=[5, 2], strict=True)
    for k in sub:
        assert torch.equal(sub[k], strict[k][[5, 2]]), k
    after = env.get_state()
    for k in before:
        a, b = before[k], after[k]
        assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), k
    with pytest.raises(ValueError, match=r"\(num_envs, K, H, num_turbines\)"):
        env.lookahead_returns(seqs[:, 0])
    env.close()


def test_kernel_info_shows_no_scratch():
    w = _handle("row3", 0.1, state=False)
    info = w.lookahead_kernel_info()
    w.close()
    assert set(info) == {"layout", "reduce"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0, (k, v)
