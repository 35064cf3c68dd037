"""TEST INFRASTRUCTURE — the reference for the closed-loop rollouts of yaw-table controllers (include/wfrollout.h): a plain
NumPy restatement over the float64 oracle (oracle.c_oracle.farm_step_batch), which it does not modify, built from the
references of the pieces: rose_ref.lookup (the table), credit_ref.transition / lookahead_ref.increment (the env's transition),
credit_ref.reward / bound (the row reward and what the step's contract allows), lookahead_ref.discounted (the return).

The definition, as the header states it, for one farm of N turbines, K controllers (slot, alpha, deadband, lead), H steps:
  observations  obs[0] the wind the env holds, obs[j] the wind of step j - 1
  controller    for h = 0 .. H - 1: o = obs[min(h + lead, H)];  float64 filter fs += alpha (o_s - fs), fd += alpha wrap(o_d - fd),
                wrap(d) = d - 360 rint(d / 360), every product and sum one IEEE operation, alpha == 1 a copy;  target = the
                table of `slot` at (fs, fd), clipped to (yaw_lo, yaw_hi) in float32;  e = target - y in float32;  the RAW action:
                continuous 0 inside the deadband else e clipped to +-step, discrete 1 inside the deadband else 2 / 0 / 1 by
                half a step;  then the env's transition with the move counter moves + 1 + h and acc += |da|
  rows, rewards, returns, best   lookahead_ref's
It also defines the cases the CPU and GPU tests share (`CASES`, `case`, `reference`)."""
import functools

import numpy as np

import credit_ref
import lookahead_ref
import rose_ref
import yawopt_ref

ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1)  # env_config's defaults
FIELDS = ("slot", "alpha", "deadband", "lead")
MAX_LEAD = 16


def wrap(d):
    """d - 360 rint(d / 360) in float64: rint rounds ties to even."""
    d = np.float64(d)
    return d - np.float64(360.0) * np.rint(d / np.float64(360.0))


def filter_step(fs, fd, os_, od, alpha):
    """One step of the float64 filter; alpha == 1 copies the observation."""
    alpha = np.float64(alpha)
    if alpha == 1.0:
        return np.float64(os_), np.float64(od)
    fs = fs + alpha * (np.float64(os_) - fs)
    fd = fd + alpha * wrap(np.float64(od) - fd)
    return fs, fd


def raw_action(target, yaw, deadband, env_params):
    """(N,) float32 raw actions from float32 targets and yaws."""
    f = np.float32
    step = f(env_params["yaw_step"])
    e = (np.asarray(target, f) - np.asarray(yaw, f)).astype(f)
    inside = np.abs(e) <= f(deadband)
    if env_params["discrete"]:
        half = f(0.5) * step
        a = np.where(e >= half, 2.0, np.where(e <= -half, 0.0, 1.0)).astype(f)
        return np.where(inside, f(1.0), a).astype(f)
    return np.where(inside, f(0.0), np.minimum(np.maximum(e, -step), step)).astype(f)


def broadcast_controllers(controllers):
    """dict of (K,) arrays from scalars / sequences: slot and lead int, alpha float64, deadband float32."""
    kinds = {"slot": np.int64, "alpha": np.float64, "deadband": np.float32, "lead": np.int64}
    default = {"slot": 0, "alpha": 1.0, "deadband": 0.0, "lead": 0}
    cols = {k: np.atleast_1d(np.asarray(controllers.get(k, default[k]), kinds[k])) for k in FIELDS}
    K = max(c.size for c in cols.values())
    return {k: np.broadcast_to(c, (K,)).copy() for k, c in cols.items()}, K


def trajectories(state, ws, wd, wind, controllers, tables, env_params, filter0=None):
    """The closed loop without any farm solve.  state dict(yaw (B, N), acc (B, N), moves (B,)); ws, wd (B,) the wind the env
    holds; wind (B, H, 2); tables {slot: (table, twd, tws, interp)}; filter0 (B, K, 2) or None.  Returns dict(actions, yaw,
    gated (B, K, H, N), target (B, K, H, N) float32 clipped, filt (B, K, H, 2) the filter after every step, filter_final
    (B, K, 2), circular (B, K, H) bool — the table's last-to-first bracket was used —, obs_index (K, H), final: the state)."""
    f = np.float32
    ctl, K = broadcast_controllers(controllers)
    wind = np.asarray(wind, np.float64)
    B, H = wind.shape[:2]
    N = np.asarray(state["yaw"]).shape[1]
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    obs = np.concatenate([np.stack([ws, wd], axis=1)[:, None, :], wind], axis=1)  # (B, H + 1, 2)
    y = np.repeat(np.asarray(state["yaw"], f).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    acc = np.repeat(np.asarray(state["acc"], f).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    moves = np.repeat(np.asarray(state["moves"]).reshape(B, 1), K, axis=1).reshape(B * K).astype(np.int64)
    filt = np.empty((B, K, 2), np.float64)
    filt[:] = np.stack([ws, wd], axis=1)[:, None, :] if filter0 is None else np.asarray(filter0, np.float64)
    out = {k: np.empty((B, K, H, N), f) for k in ("actions", "yaw", "target")}
    out["gated"] = np.empty((B, K, H, N), bool)
    out["filt"] = np.empty((B, K, H, 2), np.float64)
    out["circular"] = np.zeros((B, K, H), bool)
    out["obs_index"] = np.empty((K, H), np.int64)
    lo, hi = f(env_params["yaw_lo"]), f(env_params["yaw_hi"])
    for h in range(H):
        a = np.empty((B * K, N), f)
        for b in range(B):
            for k in range(K):
                j = min(h + int(ctl["lead"][k]), H)
                out["obs_index"][k, h] = j
                fs, fd = filter_step(filt[b, k, 0], filt[b, k, 1], obs[b, j, 0], obs[b, j, 1], ctl["alpha"][k])
                filt[b, k] = (fs, fd)
                T, twd, tws, interp = tables[int(ctl["slot"][k])]
                tg = np.minimum(np.maximum(rose_ref.lookup(T, twd, tws, fs, fd, interp), lo), hi).astype(f)
                kb = rose_ref.bracket(twd, tws, fs, fd)
                out["circular"][b, k, h] = len(twd) > 1 and kb[0] == len(twd) - 1 and kb[1] == 0
                out["target"][b, k, h] = tg
                a[b * K + k] = raw_action(tg, y[b * K + k], ctl["deadband"][k], env_params)
        out["filt"][:, :, h] = filt
        y_new = credit_ref.transition(y, acc, moves, a, env_params)
        da, g = lookahead_ref.increment(acc, moves, a, env_params)
        acc = (acc + np.abs(da)).astype(f)
        moves = moves + 1
        y = y_new
        out["actions"][:, :, h] = a.reshape(B, K, N)
        out["yaw"][:, :, h] = y.reshape(B, K, N)
        out["gated"][:, :, h] = g.reshape(B, K, N)
    out["filter_final"] = filt.copy()
    out["final"] = {"yaw": y.reshape(B, K, N), "acc": acc.reshape(B, K, N), "moves": moves.reshape(B, K)}
    return out


def rollout(x, y, ws, wd, state, controllers, tables, H, env_params, gamma, load_coef, wind=None, wr0=None, filter0=None, p=None):
    """ws, wd (B,) the wind the env holds; wind (B, H, 2) per step (None: ws, wd held); wr0 (B,) the speed step 0 is
    normalised by (None: ws).  Returns trajectories' dict plus returns (B, K), rewards, farm_power (B, K, H), final_yaw
    (B, K, N) float32, gated_count (B, K), best (B,), out: the oracle's outputs of all B K H rows, wr_rows (B K H,)."""
    from oracle import c_oracle

    B, N = np.asarray(state["yaw"]).shape
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    if wind is None:
        wind = np.stack([np.repeat(ws[:, None], H, axis=1), np.repeat(wd[:, None], H, axis=1)], axis=2)
    wind = np.asarray(wind, np.float64)
    assert wind.shape == (B, H, 2)
    wr0 = ws if wr0 is None else np.broadcast_to(np.asarray(wr0, np.float64), (B,))
    r = trajectories(state, ws, wd, wind, controllers, tables, env_params, filter0)
    K = r["yaw"].shape[1]
    ws_rows = np.repeat(wind[:, None, :, 0], K, axis=1)
    wd_rows = np.repeat(wind[:, None, :, 1], K, axis=1)
    wr = np.concatenate([wr0[:, None], wind[:, :-1, 0]], axis=1)  # (B, H): the speed BEFORE step h
    wr_rows = np.repeat(wr[:, None, :], K, axis=1).reshape(-1)
    out = c_oracle.farm_step_batch(x, y, ws_rows.reshape(-1), wd_rows.reshape(-1), r["yaw"].reshape(B * K * H, N).astype(np.float64), p)
    out = {k: np.asarray(v) for k, v in out.items() if k in ("power", "load", "wind_speed", "wind_direction")}
    rewards = credit_ref.reward(out, wr_rows, load_coef).reshape(B, K, H)
    returns = lookahead_ref.discounted(rewards, gamma)
    r.update(returns=returns, rewards=rewards, farm_power=credit_ref.sums(out)[0].reshape(B, K, H), final_yaw=r["final"]["yaw"],
             gated_count=r["gated"].sum(axis=(2, 3)).astype(np.int32), best=np.argmax(returns, axis=1), out=out, wr_rows=wr_rows)
    return r


def bounds(ref, load_coef, tol, gamma):
    """(reward bound (B, K, H), farm-power bound (B, K, H), return bound (B, K) = sum_h g_h bound_h) of a `rollout` result."""
    shape = ref["rewards"].shape
    b = credit_ref.bound(ref["out"], ref["wr_rows"], load_coef, tol).reshape(shape)
    pb = credit_ref.power_bound(ref["out"], tol).reshape(shape)
    return b, pb, (lookahead_ref.discounts(gamma, shape[2]) * b).sum(axis=2)


# ---- the cases the CPU and GPU tests share: the smallest shapes at which the kernels can go wrong ---------------------------
def steering_table(x, twd, tws, centre, width, seed):
    """A synthetic wake-steering table (Dt, St, N) float32: per turbine an amplitude of 8 to 24 deg, an odd function of the
    misalignment around `centre` (one sine period over +-width, zero outside), shrinking with the speed.  What the look-up is
    given matters here, not whether it is an optimum."""
    rng = np.random.default_rng(seed)
    amp = rng.uniform(8.0, 24.0, len(x))
    d = (np.asarray(twd, np.float64) - centre + 180.0) % 360.0 - 180.0
    shape = np.where(np.abs(d) <= width, np.sin(np.pi * d / width), 0.0)
    speed = 1.0 - 0.25 * np.arange(len(tws)) / max(len(tws) - 1, 1)
    return (shape[:, None, None] * speed[None, :, None] * amp[None, None, :]).astype(np.float32)


def swing(rng, B, H, ws0, wd0, amp, noise):
    """(B, H, 2) winds: a slow swing of the direction around wd0 plus AR(1) noise, a slowly varying speed."""
    h = np.arange(1, H + 1)
    phase = rng.uniform(0.0, 2.0 * np.pi, (B, 1))
    ar = np.zeros((B, H))
    e = rng.normal(0.0, noise, (B, H))
    for i in range(1, H):
        ar[:, i] = 0.7 * ar[:, i - 1] + e[:, i]
    wdir = wd0[:, None] + amp * (np.sin(2.0 * np.pi * h[None, :] / max(H, 8) + phase) - np.sin(phase)) + ar
    wspd = ws0[:, None] * (1.0 + 0.03 * np.sin(2.0 * np.pi * h[None, :] / 11.0 + phase))
    return np.stack([wspd, wdir], axis=2)


# name: layout, farms, K controllers (alpha, deadband, lead, slot), H, discrete, direction the winds sit around, what it is aimed at.
# The seeds were chosen WITH THIS REFERENCE (a condition on the inputs, asserted in tests/test_rollout.py): on every farm the
# controllers' returns are pairwise further apart than the sum of their two default-mode bounds (4.9 times at the least), so
# `best` and the order of the returns can be compared.
CASES = {
    # the row of three: every controller feature at once, continuous control; slot 0 NEAREST on a 2.5 deg grid, slot 1 LINEAR
    "row3": dict(layout="row3", B=4, H=7, discrete=False, wd0=268.0, amp=9.0, noise=1.5, gamma=0.95, seed=19,
                 controllers=dict(alpha=[1.0, 0.5, 1.0, 0.25, 1.0], deadband=[0.0, 0.0, 4.0, 2.0, 0.0], lead=[0, 0, 1, 0, 16],
                                  slot=[0, 1, 0, 1, 1])),
    # the same under discrete control
    "row3_discrete": dict(layout="row3", B=4, H=7, discrete=True, wd0=268.0, amp=9.0, noise=1.5, gamma=0.95, seed=18,
                          controllers=dict(alpha=[1.0, 0.5, 1.0, 0.25, 1.0], deadband=[0.0, 3.0, 6.0, 1.0, 2.5], lead=[0, 1, 1, 0, 16],
                                           slot=[0, 1, 0, 1, 1])),
    # N = 7, five farms (farm lists, ragged chunks), winds around north: the filtered direction crosses 0 / 360 and the
    # table's circular bracket (its last node to its first) is used
    "Ablaincourt_": dict(layout="Ablaincourt_", B=5, H=6, discrete=False, wd0=359.0, amp=6.0, noise=1.0, gamma=1.0, seed=10,
                         controllers=dict(alpha=[1.0, 0.4, 0.7], deadband=[0.0, 1.0, 3.0], lead=[0, 2, 0], slot=[2, 2, 3])),
    # N = 80, K N = 320 trajectories (more than a block's 256 threads), 280 rows far past one LDS tile, H past lookahead's 64
    "HornsRev1_": dict(layout="HornsRev1_", B=2, H=70, discrete=False, wd0=270.0, amp=10.0, noise=1.5, gamma=0.99, seed=7,
                       controllers=dict(alpha=[1.0, 0.3, 1.0, 0.6], deadband=[0.0, 0.0, 5.0, 2.5], lead=[0, 0, 1, 2], slot=[0, 0, 1, 1])),
}
LOAD_COEF = 0.1


def _freeze(obj):
    if isinstance(obj, np.ndarray):
        obj.setflags(write=False)
    elif isinstance(obj, dict):
        for v in obj.values():
            _freeze(v)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            _freeze(v)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(x, y, ws, wd (B,), wind (B, H, 2), state, tables {slot: (T, twd, tws, interp)}, controllers, H, K, env, gamma) — read-only."""
    c = CASES[name]
    if c["layout"] == "row3":
        x, y = yawopt_ref.ROW3
    else:
        lay = yawopt_ref.layouts()[c["layout"]]
        x, y = np.asarray(lay["xcoords"], np.float64), np.asarray(lay["ycoords"], np.float64)
    B, H, N = c["B"], c["H"], len(x)
    rng = np.random.default_rng(c["seed"])
    ws = rng.uniform(7.0, 10.0, B)
    wd = c["wd0"] + rng.uniform(-3.0, 3.0, B)
    wind = swing(rng, B, H, ws, wd, c["amp"], c["noise"])
    moves = rng.integers(0, 4, B).astype(np.int32)
    # the gate closes at acc >= 1.8 (moves + 1): start below it, so that it closes along the horizon and opens again
    state = {"yaw": rng.uniform(-8.0, 8.0, (B, N)).astype(np.float32),
             "acc": (rng.uniform(0.0, 1.5, (B, N)) * (moves[:, None] + 1)).astype(np.float32), "moves": moves}
    near = np.arange(240.0, 300.1, 2.5)          # slots 0 / 1: a 2.5 deg grid around west
    ring = np.arange(5.0, 360.0, 10.0)           # slots 2 / 3: the whole circle, no node at 0: north lies in the circular bracket
    tws = np.array([6.0, 8.0, 10.0, 12.0])
    tables = {0: (steering_table(x, near, tws, 270.0, 20.0, 1), near, tws, "nearest"),
              1: (steering_table(x, near, tws, 270.0, 20.0, 2), near, tws, "linear"),
              2: (steering_table(x, ring, tws[:1], 0.0, 30.0, 3), ring, tws[:1], "linear"),
              3: (steering_table(x, ring, tws, 0.0, 30.0, 4), ring, tws, "nearest")}
    ctl, K = broadcast_controllers(c["controllers"])
    out = dict(x=x, y=y, ws=ws, wd=wd, wind=wind, state=state, tables=tables, controllers=ctl, H=H, K=K, B=B, N=N,
               env=dict(ENV, discrete=c["discrete"]), gamma=c["gamma"])
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, held=False):
    """`rollout` of a case under its per-step winds (held: under the held wind, wind=None), load_coef LOAD_COEF — read-only."""
    c = case(name)
    r = rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["controllers"], c["tables"], c["H"], c["env"], c["gamma"], LOAD_COEF,
                wind=None if held else c["wind"])
    _freeze(r)
    return r


# ---- the series-ahead case: a series that ends inside the horizon -----------------------------------------------------------
SERIES = dict(layout="Turb3_Row1_", env_id="Turb3_Row1_Floris", B=4, T=8, t=3, H=6, start=(0, 5, 7, 2), gamma=0.9,
              controllers=dict(alpha=[1.0, 0.5, 1.0], deadband=[0.0, 1.0, 2.0], lead=[0, 0, 1], slot=[0, 1, 1]))


@functools.lru_cache(maxsize=None)
def series_case():
    """dict(x, y, series (T, 2), start, t, ws, wd — the wind of tick t —, rows (B, H, 2) — the window (1, H) —, available, state,
    tables, controllers, H, K, env, gamma): T - t - 1 = 4 rows are left of a horizon of 6, the last one is held."""
    import series_cases
    import series_ref

    c = SERIES
    x, y = series_cases.layout(c["layout"])
    B, N, H = c["B"], len(x), c["H"]
    s = series_cases.series(c["T"])
    start = np.asarray(c["start"], np.int32)
    now = s[(start + c["t"]) % c["T"]]
    rows, avail = series_ref.window(s, start, c["t"], 1, H)
    rng = np.random.default_rng(23)
    state = {"yaw": rng.uniform(-8.0, 8.0, (B, N)).astype(np.float32), "acc": rng.uniform(0.0, 6.0, (B, N)).astype(np.float32),
             "moves": np.full(B, c["t"] - 1, np.int32)}
    near, tws = np.arange(240.0, 300.1, 2.5), np.array([6.0, 8.0, 10.0, 12.0])
    tables = {0: (steering_table(x, near, tws, 270.0, 20.0, 1), near, tws, "nearest"),
              1: (steering_table(x, near, tws, 270.0, 20.0, 2), near, tws, "linear")}
    ctl, K = broadcast_controllers(c["controllers"])
    out = dict(x=x, y=y, series=s, start=start, t=c["t"], T=c["T"], ws=now[:, 0].copy(), wd=now[:, 1].copy(), rows=rows, available=avail,
               state=state, tables=tables, controllers=ctl, H=H, K=K, B=B, N=N, env=dict(ENV, discrete=False), gamma=c["gamma"])
    _freeze(out)
    return out


@functools.lru_cache(maxsize=None)
def series_reference():
    """`rollout` of the series case: row h under window entry h, step 0 normalised by the CURRENT speed — read-only."""
    c = series_case()
    r = rollout(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["controllers"], c["tables"], c["H"], c["env"], c["gamma"], LOAD_COEF,
                wind=c["rows"], wr0=c["ws"])
    _freeze(r)
    return r
