"""TEST INFRASTRUCTURE — the reference for the multi-step look-ahead returns (include/wflookahead.h): a plain NumPy
restatement over the float64 oracle (oracle.c_oracle.farm_step_batch), which it does not modify.

The definition, as the header states it, for one farm of N turbines, K action sequences of H steps:
  trajectory  sequence k starts at the farm's env state (yaw, acc, moves); step h applies the fused env step's transition
              (credit_ref.transition: gate, increment, clip, in float32) and then acc += |a| — a the increment the gate and
              the clip left — and moves += 1
  rows        R = K H: row k H + h holds the yaw after step h of sequence k, under wind h (the farm's wind held, or wind[h])
  row reward  credit_ref.reward: psum / N / 1e6 * 1e3 / wr^3 - load_coef lsum / (4 N), float64, left to right; wr is the
              free-stream speed BEFORE the step: wr0 (None: the farm's current speed) for h = 0, the speed of wind h - 1 after
  return      g_0 = 1, g_h = g_{h-1} gamma; ret = sum_h g_h r_h added in ascending h from 0.0, product and sum rounded
              separately
  best        the sequence of the largest return, the lowest index among equal maxima
P and the loads are the oracle's float64 values (the device's are the step's float32 outputs: credit_ref.bound says how far
the two may be apart)."""
import numpy as np

import credit_ref


def increment(acc, moves, action, env_params):
    """(a, gated): the float32 increment the gate and the clip leave of `action` (B, N) on acc (B, N), moves (B,) — the
    counter BEFORE the step — and where the gate was closed.  The operations of credit_ref.transition."""
    f = np.float32
    e = env_params
    a = np.array(action, dtype=f)
    mv = (np.asarray(moves).reshape(-1, 1) + 1).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = ((np.asarray(acc, f) / f(e["actuator_rate"])) / mv) / f(e["dt"])
    gated = frac >= f(e["budget"])
    a = np.where(gated, f(0.0), a).astype(f)
    step = f(e["yaw_step"])
    a = ((a - f(1.0)) * step).astype(f) if e["discrete"] else np.minimum(np.maximum(a, -step), step)
    return a.astype(f), gated


def trajectories(state, actions, env_params):
    """(yaw (B, K, H, N) float32 — the yaw after every step —, gated (B, K, H, N) bool, final state dict(yaw, acc (B, K, N),
    moves (B, K))) of actions (B, K, H, N) from state dict(yaw (B, N), acc (B, N), moves (B,))."""
    actions = np.asarray(actions, np.float32)
    B, K, H, N = actions.shape
    y = np.repeat(np.asarray(state["yaw"], np.float32).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    acc = np.repeat(np.asarray(state["acc"], np.float32).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    moves = np.repeat(np.asarray(state["moves"]).reshape(B, 1), K, axis=1).reshape(B * K).astype(np.int64)
    yaw = np.empty((B, K, H, N), np.float32)
    gated = np.empty((B, K, H, N), bool)
    for h in range(H):
        a = actions[:, :, h, :].reshape(B * K, N)
        y = credit_ref.transition(y, acc, moves, a, env_params)
        da, g = increment(acc, moves, a, env_params)
        acc = (acc + np.abs(da)).astype(np.float32)
        moves = moves + 1
        yaw[:, :, h, :] = y.reshape(B, K, N)
        gated[:, :, h, :] = g.reshape(B, K, N)
    return yaw, gated, {"yaw": y.reshape(B, K, N), "acc": acc.reshape(B, K, N), "moves": moves.reshape(B, K)}


def discounts(gamma, H):
    """[g_0 .. g_{H-1}] float64: g_0 = 1, g_h = g_{h-1} gamma."""
    g = np.empty(H, np.float64)
    v = np.float64(1.0)
    for h in range(H):
        g[h] = v
        v = v * np.float64(gamma)
    return g


def discounted(rewards, gamma):
    """(...,) float64 returns of rewards (..., H): sum_h g_h r_h added in ascending h from 0.0."""
    rewards = np.asarray(rewards, np.float64)
    g = discounts(gamma, rewards.shape[-1])
    ret = np.zeros(rewards.shape[:-1], np.float64)
    for h in range(rewards.shape[-1]):
        ret = ret + g[h] * rewards[..., h]
    return ret


def lookahead(x, y, ws, wd, state, actions, env_params, gamma, load_coef, wind=None, wr0=None, p=None):
    """ws, wd (B,) a wind per farm; state dict(yaw (B, N), acc (B, N), moves (B,)); actions (B, K, H, N) in the env's
    encoding; wind (B, H, 2) (speed, direction) per step (None: ws, wd held); wr0 (B,) the speed step 0 is normalised by
    (None: ws).  Returns dict(returns (B, K), rewards (B, K, H), farm_power (B, K, H), final_yaw (B, K, N) float32, best (B,),
    yaw (B, K, H, N), gated (B, K, H, N), out: the oracle's outputs of all B K H rows, wr_rows (B K H,))."""
    from oracle import c_oracle

    actions = np.asarray(actions, np.float32)
    B, K, H, N = actions.shape
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    if wind is None:
        wind = np.stack([np.repeat(ws[:, None], H, axis=1), np.repeat(wd[:, None], H, axis=1)], axis=2)
    wind = np.asarray(wind, np.float64)
    assert wind.shape == (B, H, 2)
    wr0 = ws if wr0 is None else np.broadcast_to(np.asarray(wr0, np.float64), (B,))
    yaw, gated, final = trajectories(state, actions, env_params)
    ws_rows = np.repeat(wind[:, None, :, 0], K, axis=1)  # (B, K, H)
    wd_rows = np.repeat(wind[:, None, :, 1], K, axis=1)
    wr = np.concatenate([wr0[:, None], wind[:, :-1, 0]], axis=1)  # (B, H): the speed BEFORE step h
    wr_rows = np.repeat(wr[:, None, :], K, axis=1).reshape(-1)
    out = c_oracle.farm_step_batch(x, y, ws_rows.reshape(-1), wd_rows.reshape(-1), yaw.reshape(B * K * H, N).astype(np.float64), p)
    out = {k: np.asarray(v) for k, v in out.items() if k in ("power", "load", "wind_speed", "wind_direction")}
    rewards = credit_ref.reward(out, wr_rows, load_coef).reshape(B, K, H)
    fp = credit_ref.sums(out)[0].reshape(B, K, H)
    returns = discounted(rewards, gamma)
    return {"returns": returns, "rewards": rewards, "farm_power": fp, "final_yaw": final["yaw"], "best": np.argmax(returns, axis=1),
            "yaw": yaw, "gated": gated, "final": final, "out": out, "wr_rows": wr_rows}
