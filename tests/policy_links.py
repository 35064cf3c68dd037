"""TEST INFRASTRUCTURE — the link checks tests/test_policy_gpu.py, tests/test_polscen_gpu.py and
tests/test_policy_wide_gpu.py share.  A closed loop feeds every step's rounding back into the next observation, so a run is
never compared with the reference's run: each link of the loop is checked against the device's OWN upstream values
(tests/test_policy_gpu.py's docstring lists the four).  `c` is a policy case as policy_ref.build makes it, `got` what
policy_returns returned for it.  The tolerances are the project's own: bits, one float32 ulp where a tanh is involved
(np.exp against the library's exp_lean), parity.TOL_F64 carried into the reward by credit_ref.bound."""
import numpy as np

import credit_ref
import lookahead_ref
import parity
import policy_ref as pr

LA_WANT = ("returns", "rewards", "farm_power", "final_yaw")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def network_link(c, name, observations, actions):
    """Link 1: policy_ref's network on the device's observations (B, K, ..., 3 N + 2) gives the device's actions (B, K, ..., N)
    bit for bit (relu, softsign) or within one float32 ulp (tanh); the discrete argmax is equal, the reference's two best
    outputs being further apart than 1e-9 on every turbine (asserted)."""
    N, spec, discrete = c["N"], c["spec"], c["env"]["discrete"]
    for k in range(c["K"]):
        want, margin = pr.actions_from_observations(c["params"][k], spec, observations[:, k], N, discrete)
        dev = actions[:, k]
        if discrete:
            print(f"{name} policy {k}: smallest gap between a turbine's two best outputs {margin.min():.3e}")
            assert (margin > 1e-9).all()
            assert np.array_equal(dev, want)
        elif "tanh" in (spec["activation"] if len(spec["widths"]) > 2 else None, spec["final"]):
            ulp = np.spacing(np.abs(want)).astype(np.float32)
            print(f"{name} policy {k}: actions that differ from the reference's by one float32 ulp: {(dev != want).sum()} of {dev.size}")
            assert (np.abs(dev.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        else:
            assert np.array_equal(bits(dev), bits(want)), (name, k, np.abs(dev - want).max())


def walk_link(c, got):
    """Link 2: lookahead_ref.trajectories of the device's actions gives final_yaw, the yaw block of the observations (step 0:
    the env state; step h: the yaw after step h - 1) and the closed-gate counts, bit for bit.  The free-wind block is the
    wind the row was solved under.  Returns the walk's gates (B, K, H, N)."""
    N = c["N"]
    yaw, gated, final = lookahead_ref.trajectories(c["state"], got["actions"], c["env"])
    assert np.array_equal(bits(got["final_yaw"]), bits(final["yaw"]))
    prev = np.concatenate([np.broadcast_to(c["state"]["yaw"][:, None, None], yaw[:, :, :1].shape), yaw[:, :, :-1]], axis=2)
    assert np.array_equal(bits(got["observations"][..., :N]), bits(prev))
    assert np.array_equal(got["gated"], gated.sum(axis=(2, 3)))
    held = np.stack([c["ws"], c["wd"]], axis=1)[:, None]
    wind = np.repeat(held, c["H"], axis=1) if c["wind"] is None else c["wind"]
    seen = np.concatenate([held, wind[:, :-1]], axis=1).astype(np.float32)  # (B, H, 2): observation h holds wind h - 1
    assert np.array_equal(got["observations"][..., 3 * N:], np.broadcast_to(seen[:, None], got["observations"][..., 3 * N:].shape))
    return gated


def lookahead_link(name, got, la, strict):
    """Link 3, oracle-free: lookahead_returns fed with policy k's `actions` under the same wind, in the same mode — la: {k: its
    result} — returns the bits of rewards, farm_power, returns and final_yaw."""
    for k, r in la.items():
        for key in LA_WANT:
            assert same(got[key][:, k:k + 1], r[key]), (name, strict, k, key)


def returns_link(c, got):
    """`best` is the argmax of the device's own returns, the lowest index among equals; the return is the discounted sum of the
    device's own rewards."""
    assert np.array_equal(got["best"], np.argmax(got["returns"], axis=1))
    assert np.array_equal(got["returns"], lookahead_ref.discounted(got["rewards"], c["gamma"]))


def oracle_link(c, name, got):
    """Link 4 (strict): every float64 solve within the step's contract of the oracle at the device's yaw of that step — the
    local wind blocks of the observations under parity.TOL_F64's wind_speed / wind_dir tolerances, every reward and farm
    power under the bound that follows from it."""
    from oracle import c_oracle

    N, K, H = c["N"], c["K"], c["H"]
    ref = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], got["actions"], c["env"], c["gamma"], pr.LOAD_COEF, wind=c["wind"])
    shape = ref["rewards"].shape
    b = credit_ref.bound(ref["out"], ref["wr_rows"], pr.LOAD_COEF, parity.TOL_F64).reshape(shape)
    pb = credit_ref.power_bound(ref["out"], parity.TOL_F64).reshape(shape)
    er, ep = np.abs(got["rewards"] - ref["rewards"]), np.abs(got["farm_power"] - ref["farm_power"])
    print(f"{name}: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}")
    assert (er <= b).all() and (ep <= pb).all()
    # the local wind of observation h: the solve of the yaw it holds, under the wind it holds (in float64: not the float32 copy)
    obs = got["observations"]
    held = np.stack([c["ws"], c["wd"]], axis=1)[:, None]
    wind = np.repeat(held, H, axis=1) if c["wind"] is None else c["wind"]
    seen = np.repeat(np.concatenate([held, wind[:, :-1]], axis=1)[:, None], K, axis=1).reshape(-1, 2)
    out = c_oracle.farm_step_batch(c["x"], c["y"], seen[:, 0], seen[:, 1], obs[..., :N].reshape(-1, N).astype(np.float64), None)
    rws, rwd = np.asarray(out["wind_speed"], np.float64), np.asarray(out["wind_direction"], np.float64)
    ews = np.abs(obs[..., N:2 * N].reshape(-1, N) - rws) / parity._ws_scale(rws, rws.shape[0])
    ewd = np.abs(obs[..., 2 * N:3 * N].reshape(-1, N) - rwd)
    print(f"{name}: largest local wind error / tolerance: speed {ews.max() / parity.TOL_F64['ws']:.3f}, direction {ewd.max() / parity.TOL_F64['wd']:.3f}")
    assert (ews <= parity.TOL_F64["ws"]).all() and (ewd <= parity.TOL_F64["wd"]).all()
