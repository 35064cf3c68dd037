"""TEST INFRASTRUCTURE — the reference for the scenario planner (include/wfscenplan.h): the cross-entropy method over action
sequences, every candidate scored over an ensemble of wind futures, in NumPy over the float64 oracle.  It is COMPOSED and
restates none of its parts: the candidates, the ranks over the scores and the elite mean are plan_ref's; the member paths, the
rows, the member returns, the statistics and the bound carry are scenario_ref's (over lookahead_ref); it modifies none of them.

  iteration i  a = plan_ref.candidates(mu, best, sigma[i], seed, farm index, i, K, yaw_step)
               s = scenario_ref.scenario(..., a, ..., M, process, scenario_seed, tail, lam, anchor, bounds, farms): the paths are
               keyed by scenario_seed and the farm's index alone, so every iteration draws the same ones
               elites = plan_ref.ranks(score) < E;  mu = plan_ref.elite_mean(a, elites, E);  winner = the first maximum of the score;
               best = the winner's sequence (candidate 0 is the best so far: a winner 0 keeps it)

MARGIN.  A candidate's score carries scenario_ref.carry's bound: (1 - lam) x the mean of its member bounds + lam x the
largest member bound.  An order of two scores is the same on the device when they are further apart than the sum of their
bounds; candidates of identical yaw trajectories have identical rows under identical winds, so identical scores on both
sides, and the lowest index wins on both.  Per farm and iteration the elite set is decided between every elite and every
non-elite — the closest such pair is (last elite, first non-elite) —, the winner between the winner and every other
candidate; the farm's margin is the smallest |s_a - s_b| - (bound_a + bound_b) over those pairs with differing trajectories and
over all iterations, and the farm is SAFE when it is positive: the device then has the reference's bits in plan, mean,
first_action and final_yaw.  A rank flip among the members inside one candidate moves cvar within its bound only."""
import numpy as np

import lookahead_ref
import parity
import plan_ref
import scenario_ref

MAX_ITERATIONS = 16


def margin(score, bound, yaw, elite, winner):
    """(B,): the smallest |s_a - s_c| - (bound_a + bound_c) over (elite a, non-elite c) and (winner a, other c) pairs whose yaw
    trajectories (B, K, H, N) differ; inf where there is none."""
    B, K = score.shape
    out = np.full(B, np.inf)
    for b in range(B):
        ident = np.unique(yaw[b].reshape(K, -1), axis=0, return_inverse=True)[1].reshape(-1)  # equal trajectories, equal id
        differ = ident[:, None] != ident[None, :]
        decides = elite[b][:, None] & ~elite[b][None, :]
        decides[winner[b], :] = True
        decides[winner[b], winner[b]] = False
        pairs = decides & differ
        if pairs.any():
            gap = np.abs(score[b][:, None] - score[b][None, :]) - (bound[b][:, None] + bound[b][None, :])
            out[b] = gap[pairs].min()
    return out


def plan(x, y, ws, wd, state, env_params, H, K, E, sigma, seed, gamma, load_coef, M, process, scenario_seed, tail=None, lam=0.0,
         anchor=None, bounds=(3.0, 28.0), mean0=None, farm_index=None, tol=None, p=None):
    """The plans of B farms: ws, wd (B,), state dict(yaw (B, N), acc (B, N), moves (B,)), sigma (I,), mean0 (B, H, N) or None,
    anchor (B, 2) or None, farm_index (B,) the farms' indices in the parent (None: 0 .. B - 1); tol: the per-turbine tolerance the
    bounds follow from (None: parity.TOL_F64, the strict mode).  Returns the outputs — plan, mean (B, H, N) float32, first_action,
    final_yaw (B, N) float32, plan_score, plan_expected, plan_cvar, hold_score (B,), plan_member_returns (B, M), wind_paths
    (B, M, H, 2) — plus winners (I, B), scores (I, B, K), score_bounds (I, B, K), zero_scores (I, B) — candidate 0's —, the
    winner's bounds plan_bound dict(score, expected, cvar (B,), member_returns (B, M)), hold_bound (B,), margin (B,), safe (B,)."""
    tol = parity.TOL_F64 if tol is None else tol
    B, N = np.asarray(state["yaw"]).shape
    sigma = np.asarray(sigma, np.float64).reshape(-1)
    assert 1 <= sigma.size <= MAX_ITERATIONS and K >= 3 and 1 <= E <= K
    farm_index = np.arange(B) if farm_index is None else np.asarray(farm_index)
    q = M if tail is None else int(tail)
    params = dict(env_params, discrete=False)
    mu = np.zeros((B, H, N), np.float32) if mean0 is None else np.array(mean0, np.float32).reshape(B, H, N)
    best = np.zeros((B, H, N), np.float32)
    rows = np.arange(B)
    worst = np.full(B, np.inf)
    winners, scores, sbounds = [], [], []
    hold_score = hold_bound = None
    for i, s in enumerate(sigma):
        a = plan_ref.candidates(mu, best, s, seed, farm_index, i, K, env_params["yaw_step"])
        sc = scenario_ref.scenario(x, y, ws, wd, state, a, params, gamma, load_coef, M, process, scenario_seed, q, lam, anchor, bounds,
                                   farm_index, p=p)
        c = scenario_ref.carry(sc, load_coef, tol, gamma, lam)
        score = sc["score"]
        elite = plan_ref.ranks(score) < E
        assert (elite.sum(axis=1) == E).all()
        w = np.argmax(score, axis=1)  # (the first of equal maxima)
        worst = np.minimum(worst, margin(score, c["score"], sc["members"][0]["yaw"], elite, w))
        if i == 0:
            hold_score, hold_bound = score[:, 0].copy(), c["score"][:, 0].copy()
        mu = plan_ref.elite_mean(a, elite, E)
        best = a[rows, w].copy()  # (candidate 0 is the best so far: w == 0 keeps it)
        winners.append(w); scores.append(score); sbounds.append(c["score"])
        last = {"plan_score": score[rows, w], "plan_expected": sc["expected_returns"][rows, w], "plan_cvar": sc["cvar"][rows, w],
                "plan_member_returns": sc["member_returns"][rows, w], "wind_paths": sc["wind_paths"]}
        plan_bound = {"score": c["score"][rows, w], "expected": c["expected_returns"][rows, w], "cvar": c["cvar"][rows, w],
                      "member_returns": c["member_returns"][rows, w]}
    final = lookahead_ref.trajectories(state, best[:, None], params)[2]["yaw"][:, 0]
    scores = np.stack(scores)
    return dict(last, plan=best, mean=mu, first_action=best[:, 0].copy(), final_yaw=final, hold_score=hold_score,
                hold_bound=hold_bound, plan_bound=plan_bound, winners=np.stack(winners), scores=scores,
                score_bounds=np.stack(sbounds), zero_scores=scores[:, :, 0], margin=worst, safe=worst > 0.0)
