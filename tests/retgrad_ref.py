"""TEST INFRASTRUCTURE — the reference for the gradient of look-ahead returns with respect to the action sequences
(include/wfretgrad.h): a plain NumPy restatement over the float64 oracle (oracle.c_oracle.farm_step_batch), which it does not
modify.  It is built from the references of the extensions it chains: lookahead_ref (the walk, the gate, the discounts, the
returns), credit_ref (row rewards and their bounds) and grad_ref (the perturbed yaws).

The definition, as the header states it, for one farm of N turbines, K CONTINUOUS action sequences of H steps:
  trajectory  lookahead_ref.trajectories' walk, with two pass flags per (k, h, i): t = the clip to [lo, hi] returned y + a
              unchanged; s = the gate was open and the clip to +-yaw_step returned the action unchanged, and t.  The rule: the
              derivative of an operation is 1 where it returned its input unchanged, else 0.  Later gates' dependence on acc
              is piecewise constant: derivative 0.
  rows        W = 2 N + 1 per (k, h), grad_ref.rows of the yaw after step h with the ENV's bounds and step delta, all under
              wind h: row 0 the yaw, row 2 i + 1 / 2 i + 2 entry i moved to y+ / y-; d = float64(y+) - float64(y-)
  row reward  credit_ref.reward; all W rows of step h normalised by the speed BEFORE the step (lookahead_ref)
  quotient    q[h][i] = (r(row 2 i + 1) - r(row 2 i + 2)) / d, exactly 0 where d <= 0
  sweep       per (k, i), float64, every product and sum rounded on its own: lam = terminal (or 0); for h = H-1 .. 0:
              lam = g_h q[h][i] + lam; action_gradient[h][i] = s ? lam : 0; lam = t ? lam : 0; state_gradient[i] = lam at the end
  base        returns, rewards, farm_power, final_yaw, best: lookahead_ref.lookahead's, from rows 0"""
import numpy as np

import credit_ref
import grad_ref
import lookahead_ref


def walk(state, actions, env_params):
    """(yaw (B, K, H, N) float32, mask (B, K, H, N) uint8: bit 0 = s, bit 1 = t, final state) of CONTINUOUS actions
    (B, K, H, N): lookahead_ref.trajectories' walk with the pass flags."""
    assert not env_params["discrete"]
    f = np.float32
    actions = np.asarray(actions, f)
    B, K, H, N = actions.shape
    y = np.repeat(np.asarray(state["yaw"], f).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    acc = np.repeat(np.asarray(state["acc"], f).reshape(B, 1, N), K, axis=1).reshape(B * K, N)
    moves = np.repeat(np.asarray(state["moves"]).reshape(B, 1), K, axis=1).reshape(B * K).astype(np.int64)
    yaw = np.empty((B, K, H, N), f)
    mask = np.empty((B, K, H, N), np.uint8)
    for h in range(H):
        a = actions[:, :, h, :].reshape(B * K, N)
        da, gated = lookahead_ref.increment(acc, moves, a, env_params)
        yn = credit_ref.transition(y, acc, moves, a, env_params)
        t = yn == (y + da).astype(f)
        s = (~gated) & (da == a) & t
        acc = (acc + np.abs(da)).astype(f)
        moves = moves + 1
        y = yn
        yaw[:, :, h, :] = y.reshape(B, K, N)
        mask[:, :, h, :] = (s.astype(np.uint8) | (t.astype(np.uint8) << 1)).reshape(B, K, N)
    ref_yaw, _, final = lookahead_ref.trajectories(state, actions, env_params)
    assert np.array_equal(ref_yaw.view(np.uint32), yaw.view(np.uint32))
    return yaw, mask, final


def sweep(q, mask, gamma, terminal=None):
    """(action_gradient (..., H, N), state_gradient (..., N)) float64 of q (..., H, N), mask (..., H, N) and terminal (..., N):
    the backward sweep, every product and sum rounded on its own."""
    q = np.asarray(q, np.float64)
    H = q.shape[-2]
    g = lookahead_ref.discounts(gamma, H)
    s, t = (np.asarray(mask) & 1) != 0, (np.asarray(mask) & 2) != 0
    lam = np.zeros(q.shape[:-2] + q.shape[-1:]) if terminal is None else np.array(terminal, np.float64)
    ag = np.zeros(q.shape)
    for h in range(H - 1, -1, -1):
        lam = g[h] * q[..., h, :] + lam
        ag[..., h, :] = np.where(s[..., h, :], lam, 0.0)
        lam = np.where(t[..., h, :], lam, 0.0)
    return ag, lam


def quotient_bound(row_bound, d):
    """(B, K, H, N): (bound(row 2 i + 1) + bound(row 2 i + 2)) / d from row bounds (B, K, H, W); 0 where d <= 0."""
    live = d > 0.0
    return np.where(live, (row_bound[..., 1::2] + row_bound[..., 2::2]) / np.where(live, d, 1.0), 0.0)


def sweep_bound(qb, q, mask, gamma, terminal=None):
    """(bound on |action_gradient error| (..., H, N), on |state_gradient error| (..., N)): the quotient bounds qb carried
    through the sweep with the reference's flags and discounts — the sweep is linear in q — plus the float64 rounding of its
    2 H products and sums: 2 H 2^-52 of the largest magnitude the sweep can reach (the terminal contribution is exact up to
    that rounding)."""
    H = q.shape[-2]
    g = lookahead_ref.discounts(gamma, H)
    mag = (g[:, None] * (np.abs(q) + qb)).sum(axis=-2) + (0.0 if terminal is None else np.abs(np.asarray(terminal, np.float64)))
    agb, sgb = sweep(qb, mask, gamma)
    slack = 2.0 * H * 2.0 ** -52 * mag
    return agb + slack[..., None, :], sgb + slack


def return_gradient(x, y, ws, wd, state, actions, env_params, gamma, load_coef, wind=None, wr0=None, terminal=None, delta=1.0,
                    p=None):
    """ws, wd (B,) a wind per farm; state dict(yaw (B, N), acc (B, N), moves (B,)); actions (B, K, H, N) continuous;
    wind (B, H, 2) per step (None: ws, wd held); wr0 (B,) the speed step 0 is normalised by (None: ws); terminal (B, K, N).
    Returns lookahead_ref.lookahead's base outputs (returns, rewards, farm_power, final_yaw, best) and action_gradient,
    reward_gradient (B, K, H, N), state_gradient (B, K, N), yaw, pass_mask, d (B, K, H, N), row_reward (B, K, H, W),
    out: the oracle's outputs of all B K H W rows, wr_rows (B K H W,)."""
    from oracle import c_oracle

    actions = np.asarray(actions, np.float32)
    B, K, H, N = actions.shape
    W = 2 * N + 1
    ws = np.broadcast_to(np.asarray(ws, np.float64), (B,))
    wd = np.broadcast_to(np.asarray(wd, np.float64), (B,))
    if wind is None:
        wind = np.stack([np.repeat(ws[:, None], H, axis=1), np.repeat(wd[:, None], H, axis=1)], axis=2)
    wind = np.asarray(wind, np.float64)
    assert wind.shape == (B, H, 2)
    wr0 = ws if wr0 is None else np.broadcast_to(np.asarray(wr0, np.float64), (B,))
    yaw, mask, final = walk(state, actions, env_params)
    bounds = (float(np.float32(env_params["yaw_lo"])), float(np.float32(env_params["yaw_hi"])))
    blk = grad_ref.rows(yaw.reshape(B * K * H, N), delta, bounds)  # (B K H, W, N)
    d = grad_ref.perturbed(yaw, delta, bounds)[2]  # (B, K, H, N)
    shape = (B, K, H, W)
    ws_rows = np.broadcast_to(wind[:, None, :, None, 0], shape).reshape(-1)
    wd_rows = np.broadcast_to(wind[:, None, :, None, 1], shape).reshape(-1)
    wr = np.concatenate([wr0[:, None], wind[:, :-1, 0]], axis=1)  # (B, H): the speed BEFORE step h
    wr_rows = np.broadcast_to(wr[:, None, :, None], shape).reshape(-1)
    out = c_oracle.farm_step_batch(x, y, ws_rows, wd_rows, blk.reshape(-1, N).astype(np.float64), p)
    out = {k: np.asarray(v) for k, v in out.items() if k in ("power", "load", "wind_speed", "wind_direction")}
    rr = credit_ref.reward(out, wr_rows, load_coef).reshape(shape)
    fp = credit_ref.sums(out)[0].reshape(shape)[..., 0]
    live = d > 0.0
    q = np.where(live, (rr[..., 1::2] - rr[..., 2::2]) / np.where(live, d, 1.0), 0.0)
    ag, sg = sweep(q, mask, gamma, terminal)
    rewards = rr[..., 0].copy()
    returns = lookahead_ref.discounted(rewards, gamma)
    return {"returns": returns, "rewards": rewards, "farm_power": fp.copy(), "final_yaw": final["yaw"], "best": np.argmax(returns, axis=1),
            "action_gradient": ag, "reward_gradient": q, "state_gradient": sg, "yaw": yaw, "pass_mask": mask, "d": d,
            "row_reward": rr, "out": out, "wr_rows": wr_rows}
