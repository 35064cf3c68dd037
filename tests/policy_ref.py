"""TEST INFRASTRUCTURE — the reference for the closed-loop rollouts of MLP policies (include/wfpolicy.h): a plain NumPy
restatement over the float64 oracle (oracle.c_oracle.farm_step_batch), which it does not modify.

What is restated HERE is what the header adds: the network (input normalisation, layers in a fixed order, activations, the
action from the last layer), the observation's lay-out and the closed loop's order of events.  The transition, the gate, the
reward and the discounted sum are lookahead_ref's / credit_ref's: this file calls them and restates none of them.

  network     x_i = (float64(obs_i) - shift_i) scale_i;  z_o = float64(b_o), then for i ascending z_o = z_o + float64(W[o][i]) x_i
              (product and sum rounded separately: NumPy's float64 operators do that);  hidden activation relu (z > 0 ? z : 0),
              softsign z / (1 + |z|) or tanh 1 - 2 / (exp(2 c) + 1), c = z clipped to +-20 (np.exp here, the library's exp_lean on
              the device: a few ulp apart);  the last layer linear, then `final` and out_scale
  action      continuous: float32(out_scale f(z_t));  discrete: the index of the largest of f(z_{3t .. 3t+2}), the lowest among equals
  observation central lay-out (3 N + 2,) float32: yaw, local wind speed, local wind direction, free wind (speed, direction);
              a shared policy sees (yaw_t, ws_t, wd_t[, free speed, free direction]) per turbine
  closed loop round 0 solves the current yaw under the current wind: observation 0;  for h = 0 .. H - 1: action from
              observation h, lookahead_ref's transition, the row solved under wind h, credit_ref's reward normalised by wr0
              (h = 0) or the speed of wind h - 1, observation h + 1 = the new yaw, that solve's local wind, wind h
The oracle's local wind is float64; an observation holds it rounded to float32, as the device's does."""
import functools

import numpy as np

import credit_ref
import lookahead_ref
import yawopt_ref

LOAD_COEF = 0.1
GAMMA = 0.9


def split(vec, widths):
    """[(W (out, in), b (out,))] float32 views of a parameter vector laid out as parameters_to_vector lays it out."""
    vec = np.asarray(vec, np.float32)
    out, o = [], 0
    for a, b in zip(widths[:-1], widths[1:]):
        W = vec[o:o + a * b].reshape(b, a)
        o += a * b
        out.append((W, vec[o:o + b]))
        o += b
    assert o == vec.size, "a parameter vector of the wrong length"
    return out


def activation(name, z):
    if name in (None, "none"):
        return z
    if name == "relu":
        return np.where(z > 0.0, z, 0.0)
    if name == "softsign":
        return z / (1.0 + np.abs(z))
    if name == "tanh":
        c = np.minimum(np.maximum(z, -20.0), 20.0)
        return 1.0 - 2.0 / (np.exp(2.0 * c) + 1.0)
    raise ValueError(name)


def mlp(vec, spec, obs):
    """f(z) of the last layer, float64 (..., out), for inputs obs (..., D) — un-normalised, any float type."""
    widths = spec["widths"]
    x = (np.asarray(obs).astype(np.float64) - spec["shift"]) * spec["scale"]
    layers = split(vec, widths)
    for l, (W, b) in enumerate(layers):
        W64 = W.astype(np.float64)
        z = np.broadcast_to(b.astype(np.float64), x.shape[:-1] + (b.size,)).copy()
        for i in range(W.shape[1]):  # ascending input index; product and sum are two roundings
            z = z + W64[:, i] * x[..., i:i + 1]
        x = activation(spec["activation"] if l < len(layers) - 1 else spec["final"], z)
    return x


def shared_inputs(obs, N, use_freewind):
    """(..., N, D) per-turbine inputs of a shared policy from central observations (..., 3 N + 2)."""
    obs = np.asarray(obs)
    cols = [obs[..., 0:N], obs[..., N:2 * N], obs[..., 2 * N:3 * N]]
    if use_freewind:
        cols += [np.broadcast_to(obs[..., 3 * N:3 * N + 1], cols[0].shape), np.broadcast_to(obs[..., 3 * N + 1:3 * N + 2], cols[0].shape)]
    return np.stack(cols, axis=-1)


def actions_from_observations(vec, spec, obs, N, discrete):
    """(raw actions (..., N) float32, margin (..., N) float64) of observations (..., 3 N + 2): margin is the gap between the
    two largest of a turbine's three outputs (discrete; inf for continuous control)."""
    obs = np.asarray(obs)
    if spec["kind"] == "shared":
        out = mlp(vec, spec, shared_inputs(obs, N, spec["use_freewind"]))  # (..., N, 1 or 3)
    else:
        out = mlp(vec, spec, obs)
        out = out.reshape(out.shape[:-1] + (N, 3 if discrete else 1))
    if not discrete:
        return (np.float64(spec["out_scale"]) * out[..., 0]).astype(np.float32), np.full(out.shape[:-1], np.inf)
    top = np.sort(out, axis=-1)
    return np.argmax(out, axis=-1).astype(np.float32), top[..., 2] - top[..., 1]  # (argmax: the first of equal maxima)


def observation(yaw, lws, lwd, ws, wd):
    """(rows, 3 N + 2) float32 from yaw (rows, N) float32, local wind (rows, N) and free wind (rows,)."""
    return np.concatenate([np.asarray(yaw, np.float32), np.asarray(lws).astype(np.float32), np.asarray(lwd).astype(np.float32),
                           np.asarray(ws).astype(np.float32)[:, None], np.asarray(wd).astype(np.float32)[:, None]], axis=1)


def rollout(x, y, ws, wd, state, params, spec, H, env_params, gamma, load_coef, wind=None, wr0=None, p=None):
    """ws, wd (B,); state dict(yaw (B, N), acc (B, N), moves (B,)); params (K, P).  Returns dict(returns (B, K), rewards,
    farm_power (B, K, H), actions (B, K, H, N) float32, observations (B, K, H, 3 N + 2) float32, final_yaw (B, K, N), gated
    (B, K) counts, best (B,), margin (B, K, H, N), yaw (B, K, H, N) the yaw after every step)."""
    from oracle import c_oracle

    params = np.atleast_2d(np.asarray(params, np.float32))
    B, N, K = len(ws), len(x), params.shape[0]
    ws, wd = np.asarray(ws, np.float64), np.asarray(wd, np.float64)
    if wind is None:
        wind = np.stack([np.repeat(ws[:, None], H, axis=1), np.repeat(wd[:, None], H, axis=1)], axis=2)
    wind = np.asarray(wind, np.float64)
    wr0 = ws if wr0 is None else np.broadcast_to(np.asarray(wr0, np.float64), (B,))
    rep = lambda a: np.repeat(np.asarray(a)[:, None], K, axis=1).reshape((B * K,) + np.asarray(a).shape[1:])  # rows (b, k)
    yaw, acc, moves = rep(np.asarray(state["yaw"], np.float32)), rep(np.asarray(state["acc"], np.float32)), rep(state["moves"]).astype(np.int64)
    cws, cwd = rep(ws), rep(wd)  # the wind the rows were solved under
    out = c_oracle.farm_step_batch(x, y, cws, cwd, yaw.astype(np.float64), p)
    res = {k: np.empty(s, d) for k, (s, d) in dict(rewards=((B, K, H), np.float64), farm_power=((B, K, H), np.float64),
           actions=((B, K, H, N), np.float32), observations=((B, K, H, 3 * N + 2), np.float32), margin=((B, K, H, N), np.float64),
           yaw=((B, K, H, N), np.float32)).items()}
    gated = np.zeros((B, K), np.int64)
    for h in range(H):
        obs = observation(yaw, out["wind_speed"], out["wind_direction"], cws, cwd).reshape(B, K, -1)
        a = np.empty((B, K, N), np.float32)
        for k in range(K):
            a[:, k], res["margin"][:, k, h] = actions_from_observations(params[k], spec, obs[:, k], N, env_params["discrete"])
        a2 = a.reshape(B * K, N)
        _, g = lookahead_ref.increment(acc, moves, a2, env_params)
        new = credit_ref.transition(yaw, acc, moves, a2, env_params)
        da, _ = lookahead_ref.increment(acc, moves, a2, env_params)
        acc, moves, yaw = (acc + np.abs(da)).astype(np.float32), moves + 1, new
        gated += g.reshape(B, K, N).sum(axis=2)
        wr = rep(wr0 if h == 0 else wind[:, h - 1, 0])
        cws, cwd = rep(wind[:, h, 0]), rep(wind[:, h, 1])
        out = c_oracle.farm_step_batch(x, y, cws, cwd, yaw.astype(np.float64), p)
        res["rewards"][:, :, h] = credit_ref.reward(out, wr, load_coef).reshape(B, K)
        res["farm_power"][:, :, h] = credit_ref.sums(out)[0].reshape(B, K)
        res["actions"][:, :, h], res["observations"][:, :, h], res["yaw"][:, :, h] = a, obs, yaw.reshape(B, K, N)
    res["returns"] = lookahead_ref.discounted(res["rewards"], gamma)
    res["final_yaw"], res["gated"], res["best"] = yaw.reshape(B, K, N), gated, np.argmax(res["returns"], axis=1)
    return res


# ---- the cases tests/test_policy.py asserts the properties of and tests/test_policy_gpu.py runs on the device ---------------
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=120.0, budget=0.1)
# name: (layout, farms, kind, hidden widths, activation, final, use_freewind, discrete, K, H, per-step wind, seed)
CASES = {
    "row3_central": ("row3", 4, "central", (5,), "relu", "tanh", False, False, 3, 5, True, 11),
    "row3_shared": ("row3", 4, "shared", (65, 5), "softsign", "softsign", True, False, 3, 5, True, 12),
    "row3_discrete": ("row3", 4, "shared", (5,), "relu", None, False, True, 3, 5, False, 13),
    "abl_central": ("Ablaincourt_", 7, "central", (65, 5), "tanh", "tanh", False, False, 3, 5, True, 14),
    "abl_shared": ("Ablaincourt_", 7, "shared", (5,), "tanh", "tanh", False, False, 1, 1, False, 15),
    "abl_linear": ("Ablaincourt_", 7, "central", (), "relu", None, False, False, 3, 5, False, 16),
    "horns_central": ("HornsRev1_", 4, "central", (65, 5), "relu", "softsign", False, False, 3, 5, False, 17),
}
NAMES = tuple(CASES)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


def build(name, row, inputs=None):
    """The inputs of the case `row` describes (a row of CASES, or one of another module's table in the same format): layout,
    winds, env state (some turbines at the upper yaw bound, accumulators on both sides of the budget gate), the K parameter
    vectors (uniform, scaled by 1 / sqrt(in)), the spec with a normalisation that brings every input to order one, and — where
    the case has one — a wind per step whose direction crosses 0 / 360.  `inputs` = (x, y, ws, wd) replaces
    yawopt_ref.gpu_input(layout) where the row's layout is not one of its names."""
    from wfcrl_env_amd import policy as P

    layout, B, kind, hidden, act, final, fw, discrete, K, H, per_step, seed = row
    x, y, ws, wd = yawopt_ref.gpu_input(layout) if inputs is None else inputs
    assert len(ws) >= B and len(wd) >= B, "fewer winds than farms"
    ws, wd = np.array(ws[:B], np.float64), np.array(wd[:B], np.float64)
    N = len(x)
    rng = np.random.default_rng(seed)
    state = {"yaw": rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32), "acc": rng.uniform(0.0, 20.0, (B, N)).astype(np.float32),
             "moves": rng.integers(1, 6, B).astype(np.int32)}
    state["yaw"][:, 0] = np.float32(ENV["yaw_hi"])  # a start yaw at a bound
    D = 3 * N + 2 if kind == "central" else (5 if fw else 3)
    per = 3 if discrete else 1
    widths = (D,) + tuple(hidden) + ((per * N) if kind == "central" else per,)
    if kind == "central":
        shift = np.concatenate([np.zeros(N), np.full(N, 8.0), np.full(N, 180.0), [8.0, 180.0]])
        scale = np.concatenate([np.full(N, 1 / 20.0), np.full(N, 1 / 4.0), np.full(N, 1 / 180.0), [1 / 4.0, 1 / 180.0]])
    else:
        shift = np.array([0.0, 8.0, 180.0, 8.0, 180.0][:D])
        scale = np.array([1 / 20.0, 1 / 4.0, 1 / 180.0, 1 / 4.0, 1 / 180.0][:D])
    spec = P.mlp_spec(kind, widths, act, final, out_scale=1.0 if final is None else 6.0, shift=shift, scale=scale, use_freewind=fw)
    vecs = []
    for _ in range(K):
        parts = []
        for a, b in zip(widths[:-1], widths[1:]):
            parts += [rng.uniform(-1.0, 1.0, a * b) * (2.0 / np.sqrt(a)), rng.uniform(-0.5, 0.5, b)]
        vecs.append(np.concatenate(parts))
    params = np.ascontiguousarray(np.stack(vecs), dtype=np.float32)
    if final is None and not discrete:
        params *= np.float32(4.0)  # (a linear output of order one would hardly move a turbine)
    wind = None
    if per_step:
        wind = np.empty((B, H, 2))
        wind[:, :, 0] = ws[:, None] * (1.0 + 0.05 * np.arange(1, H + 1))
        wind[:, :, 1] = np.mod(356.0 + 2.5 * np.arange(H)[None, :] + 0.5 * np.arange(B)[:, None], 360.0)  # 356 .. 360 | 0 .. : across the seam
    return _freeze(dict(name=name, x=x, y=y, ws=ws, wd=wd, B=B, N=N, K=K, H=H, state=state, spec=spec, params=params, wind=wind,
                        env=dict(ENV, discrete=discrete), gamma=GAMMA, kind=kind))


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case of CASES: `build` of its row."""
    return build(name, CASES[name])


def reference_of(c):
    """The reference rollout of a case `build` made, frozen."""
    return _freeze(rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["params"], c["spec"], c["H"], c["env"], c["gamma"], LOAD_COEF,
                           wind=c["wind"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(case(name))
