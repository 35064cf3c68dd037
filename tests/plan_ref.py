"""TEST INFRASTRUCTURE — the reference for the receding-horizon planner (include/wfplan.h): the cross-entropy method over
action sequences restated in NumPy over the float64 oracle, reusing tests/lookahead_ref.py (trajectories, lookahead,
discounts) for the scoring.  It modifies nothing of either.

The definition, as the header states it, for one farm b of N turbines, K candidates of H steps, E elites, iterations
i = 0 .. I - 1 with widths sigma[i]:
  candidates  k = 0 the best sequence so far (iteration 0: zeros), k = 1 the mean mu (mean0, or zeros, before iteration 0),
              k >= 2, element e = h N + t:  (float32) clip((double)mu[e] + sigma[i] z, -yaw_step, +yaw_step)
  deviate     z = ((double)S 2^-32 - 2.0) 1.7320508075688772, S the 64-bit sum of the four words of
              philox4x32_10(seed, ((uint64)b << 32) | (uint32)(k H N + e), stream = i), b the farm's index in the PARENT
  scoring     lookahead_ref.lookahead: the env's transition from the state, row rewards, discounted returns
  update      rank_k = #{j: ret_j > ret_k or (ret_j == ret_k and j < k)}; elites rank < E;
              mu[e] = (float32)((sum over the elites in ascending k of (double)a_k[e]) / E);
              winner = the largest return, the lowest index among equals; a winner other than 0 becomes the best sequence
Philox4x32-10 is restated from the device code (csrc/wf_philox.h) line by line: two 32 x 32 -> 64 bit products per round,
the keys bumped by the Weyl constants after every round, ten rounds.

MARGIN.  The device's returns are the step's float32 (or, strict, float64) outputs through the same formula; each is within
`bound` of the reference's — the return bound tests/test_lookahead_gpu.py derives from credit_ref.bound, sum_h g_h bound_h.
An order of two returns is the same on both sides when they are further apart than the sum of their two bounds; rows of
identical yaw trajectories have identical returns on both sides and the lowest index wins on both.  Per farm and iteration
the elite set is decided between every elite and every non-elite, the winner between the winner and everyone else — the
closest of these are (last elite, first non-elite) and (winner, runner-up); the farm's margin is the smallest
|ret_a - ret_b| - (bound_a + bound_b) over those pairs with differing trajectories and over all iterations, and the farm is
SAFE when it is positive: the device then has the reference's bits in plan, mean, first_action and final_yaw."""
import numpy as np

import credit_ref
import lookahead_ref
import parity

MASK = np.uint64(0xFFFFFFFF)
SQRT3 = 1.7320508075688772


def philox4x32_10(seed, ctr, stream):
    """The four 32-bit words (..., 4) uint32 of Philox4x32-10 keyed by the 64-bit `seed`, for 64-bit counters `ctr` (any
    shape) and the 32-bit `stream`: counter words (ctr lo, ctr hi, stream, 0), key words (seed lo, seed hi)."""
    ctr = np.asarray(ctr, np.uint64)
    c0, c1 = ctr & MASK, ctr >> np.uint64(32)
    c2 = np.full(ctr.shape, int(stream) & 0xFFFFFFFF, np.uint64)
    c3 = np.zeros(ctr.shape, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0  # (both factors below 2^32: the product is exact in 64 bits)
        p1 = np.uint64(0xCD9E8D57) * c2
        n0, n1 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK
        n2, n3 = (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def deviate(seed, farm, index, stream):
    """z float64 of farm index `farm` and element index `index` (arrays broadcast): mean 0, variance 1, |z| <= 2 sqrt 3."""
    ctr = (np.asarray(farm, np.uint64) << np.uint64(32)) | (np.asarray(index, np.uint64) & MASK)
    s = philox4x32_10(seed, ctr, stream).astype(np.uint64).sum(axis=-1, dtype=np.uint64)
    return (s.astype(np.float64) * 2.0 ** -32 - 2.0) * SQRT3


def candidates(mu, best, sigma_i, seed, farm_index, i, K, yaw_step):
    """(B, K, H, N) float32 raw actions of iteration i from mu, best (B, H, N) float32; farm_index (B,) indices in the parent."""
    B, H, N = mu.shape
    lim = float(np.float32(yaw_step))
    a = np.empty((B, K, H, N), np.float32)
    a[:, 0], a[:, 1] = best, mu
    if K > 2:
        idx = np.arange(2 * H * N, K * H * N, dtype=np.uint64).reshape(1, K - 2, H, N)
        z = deviate(seed, np.asarray(farm_index, np.uint64).reshape(B, 1, 1, 1), idx, i)
        prod = np.float64(sigma_i) * z
        a[:, 2:] = np.clip(mu[:, None].astype(np.float64) + prod, -lim, lim).astype(np.float32)
    return a


def ranks(ret):
    """rank_k = #{j: ret_j > ret_k or (ret_j == ret_k and j < k)} along the last axis."""
    K = ret.shape[-1]
    j, k = np.arange(K)[:, None], np.arange(K)[None, :]
    rj, rk = ret[..., :, None], ret[..., None, :]
    return ((rj > rk) | ((rj == rk) & (j < k))).sum(axis=-2)


def elite_mean(a, elite, E):
    """(B, H, N) float32: the float64 sum of a (B, K, H, N) over the elite rows in ascending k, one division by E."""
    s = np.zeros(a.shape[:1] + a.shape[2:], np.float64)
    for k in range(a.shape[1]):
        s = np.where(elite[:, k, None, None], s + a[:, k].astype(np.float64), s)
    return (s / np.float64(E)).astype(np.float32)


def _margin(ret, rb, yaw, elite, winner):
    """Per farm: the smallest |ret_a - ret_b| - (rb_a + rb_b) over (elite, non-elite) and (winner, other) pairs whose yaw
    trajectories differ (inf when there is none)."""
    B, K = ret.shape
    m = np.full(B, np.inf)
    for b in range(B):
        for a in range(K):
            for c in range(K):
                decides = (elite[b, a] and not elite[b, c]) or (a == winner[b] and c != a)
                if decides and not np.array_equal(yaw[b, a], yaw[b, c]):
                    m[b] = min(m[b], abs(ret[b, a] - ret[b, c]) - (rb[b, a] + rb[b, c]))
    return m


def plan(x, y, ws, wd, state, env_params, H, K, E, sigma, seed, gamma, load_coef, wind=None, mean0=None, wr0=None,
         farm_index=None, tol=None, p=None):
    """The plans of B farms: ws, wd (B,), state dict(yaw (B, N), acc (B, N), moves (B,)), sigma (I,), wind (B, H, 2) or None,
    mean0 (B, H, N) or None, farm_index (B,) the farms' indices in the parent (None: 0 .. B - 1); tol: the per-turbine
    tolerance the bounds follow from (None: parity.TOL_F64, the strict mode).  Returns dict(plan, mean (B, H, N) float32,
    first_action, final_yaw (B, N) float32, plan_return, hold_return (B,), plan_bound, hold_bound (B,) — their return bounds —,
    margin (B,), safe (B,) bool, winners (I, B))."""
    tol = parity.TOL_F64 if tol is None else tol
    B, N = np.asarray(state["yaw"]).shape
    farm_index = np.arange(B) if farm_index is None else np.asarray(farm_index)
    mu = np.zeros((B, H, N), np.float32) if mean0 is None else np.array(mean0, np.float32).reshape(B, H, N)
    best = np.zeros((B, H, N), np.float32)
    g = lookahead_ref.discounts(gamma, H)
    rows = np.arange(B)
    margin = np.full(B, np.inf)
    winners = []
    hold_return = hold_bound = None
    for i, s in enumerate(np.asarray(sigma, np.float64).reshape(-1)):
        a = candidates(mu, best, s, seed, farm_index, i, K, env_params["yaw_step"])
        la = lookahead_ref.lookahead(x, y, ws, wd, state, a, dict(env_params, discrete=False), gamma, load_coef, wind=wind, wr0=wr0, p=p)
        ret = la["returns"]
        rb = (g * credit_ref.bound(la["out"], la["wr_rows"], load_coef, tol).reshape(B, K, H)).sum(axis=2)
        elite = ranks(ret) < E
        assert (elite.sum(axis=1) == E).all()
        w = np.argmax(ret, axis=1)  # (the first of equal maxima)
        margin = np.minimum(margin, _margin(ret, rb, la["yaw"], elite, w))
        if i == 0:
            hold_return, hold_bound = ret[:, 0].copy(), rb[:, 0].copy()
        mu = elite_mean(a, elite, E)
        best = a[rows, w].copy()  # (candidate 0 is the best so far: w == 0 keeps it)
        plan_return, plan_bound = ret[rows, w], rb[rows, w]
        winners.append(w)
    final = lookahead_ref.trajectories(state, best[:, None], dict(env_params, discrete=False))[2]["yaw"][:, 0]
    return {"plan": best, "mean": mu, "first_action": best[:, 0].copy(), "final_yaw": final, "plan_return": plan_return,
            "hold_return": hold_return, "plan_bound": plan_bound, "hold_bound": hold_bound, "margin": margin, "safe": margin > 0.0,
            "winners": np.stack(winners)}
