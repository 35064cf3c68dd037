"""TEST INFRASTRUCTURE — the reference for policy search on the device (include/wfpolsearch.h): the header's definition restated
in NumPy and nothing else.  candidates: rows 0 and 1 are copies, row k >= 2 is (float)((double)mean + (double)sigma z) with
plan_ref.deviate(seed, k, p, i); aggregate: the farm scores added inside tiles of 256 list positions, then over the tiles, one
division; refit: plan_ref.ranks with every non-finite fitness as -inf, the winner, the elite mean and width per weight; search:
the loop over a scorer, which is policy_ref.rollout's returns (held wind or a wind per step) or polscen_ref.rollouts' score
(members)."""
import functools

import numpy as np

import plan_ref
import policy_ref
import polscen_ref

TILE = 256

# the search every test runs on the policy_ref cases: (K, E, I); the start is params[0]
SIGMA0, SIGMA_MIN, SEED = 0.3, 0.01, 7
CASES = {"row3_shared": (8, 2, 3), "row3_central": (8, 2, 3), "abl_central": (6, 2, 2), "row3_discrete": (8, 2, 3)}
NAMES = tuple(CASES)


def candidates(mean, sigma, incumbent, seed, i, K):
    """C_i (K, P) float32 from mean, sigma, incumbent (P,) float32."""
    mean, sigma = np.asarray(mean, np.float32), np.asarray(sigma, np.float32)
    P = mean.size
    c = np.empty((K, P), np.float32)
    c[0], c[1] = np.asarray(incumbent, np.float32), mean
    if K > 2:
        z = plan_ref.deviate(seed, np.arange(2, K, dtype=np.uint64)[:, None], np.arange(P, dtype=np.uint64)[None, :], i)
        prod = sigma.astype(np.float64)[None, :] * z
        c[2:] = (mean.astype(np.float64)[None, :] + prod).astype(np.float32)
    return c


def aggregate(farm_scores):
    """F (K,) float64 from farm scores (n, K) float64 in list order."""
    s = np.asarray(farm_scores, np.float64)
    n, K = s.shape
    total = np.zeros(K, np.float64)
    for first in range(0, n, TILE):
        t = np.zeros(K, np.float64)
        for b in range(first, min(first + TILE, n)):
            t = t + s[b]
        total = total + t
    return total / np.float64(n)


def refit(C, F, E, sigma_min):
    """(winner, mean (P,) float32, sigma (P,) float32, elite (K,) bool) of candidates C (K, P) float32 with fitness F (K,)."""
    C, F = np.asarray(C, np.float32), np.asarray(F, np.float64)
    g = np.where(np.isfinite(F), F, -np.inf)
    rank = plan_ref.ranks(g)
    winner = int(np.flatnonzero(rank == 0)[0])
    elite = rank < E
    s = np.zeros(C.shape[1], np.float64)
    for k in range(C.shape[0]):
        if elite[k]:
            s = s + C[k].astype(np.float64)
    m = s / np.float64(E)
    q = np.zeros(C.shape[1], np.float64)
    for k in range(C.shape[0]):
        if elite[k]:
            d = C[k].astype(np.float64) - m
            q = q + d * d
    v = q / np.float64(E)
    return winner, m.astype(np.float32), (np.sqrt(v) + np.float64(sigma_min)).astype(np.float32), elite


def search(scorer, mean0, sigma0, K, E, I, sigma_min, seed):
    """The loop over `scorer`: (K, P) float32 -> (n, K) float64 farm scores.  dict(best_params, best_fitness, init_fitness, mean,
    sigma, fitness (I, K), winner (I,), candidates (I, K, P), sigma_history (I, P), farm_scores (I, n, K), elite (I, K))."""
    mean = np.array(mean0, np.float32)
    sigma = np.broadcast_to(np.asarray(sigma0, np.float32), mean.shape).copy()
    inc = mean.copy()
    out = {k: [] for k in ("fitness", "winner", "candidates", "sigma_history", "farm_scores", "elite")}
    best = None
    for i in range(I):
        C = candidates(mean, sigma, inc, seed, i, K)
        fs = np.asarray(scorer(C), np.float64)
        F = aggregate(fs)
        out["sigma_history"].append(sigma)
        w, mean, sigma, elite = refit(C, F, E, sigma_min)
        inc, best = C[w].copy(), F[w]
        for k, v in (("fitness", F), ("winner", w), ("candidates", C), ("farm_scores", fs), ("elite", elite)):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    res["winner"] = res["winner"].astype(np.int32)
    res.update(best_params=inc, best_fitness=np.float64(best), init_fitness=res["fitness"][0, 0], mean=mean, sigma=sigma)
    return res


def policy_scorer(c, farms=None, wind="case"):
    """policy_ref.rollout's returns of the case `c` on the listed farms (all), under the case's wind per step (or `wind`)."""
    sel = np.arange(c["B"]) if farms is None else np.asarray(farms)
    wind = c["wind"] if isinstance(wind, str) else wind
    state = {k: np.asarray(v)[sel] for k, v in c["state"].items()}

    def score(C):
        return policy_ref.rollout(c["x"], c["y"], c["ws"][sel], c["wd"][sel], state, C, c["spec"], c["H"], c["env"], c["gamma"],
                                  policy_ref.LOAD_COEF, wind=None if wind is None else wind[sel])["returns"]
    return score


def polscen_scorer(s, scenario_seed):
    """polscen_ref.rollouts' score of the ensemble case `s` (polscen_ref.build's dict): the same scenario_seed in every iteration."""
    def score(C):
        c = dict(s["c"], params=C)
        return polscen_ref.rollouts(c, s["ws"], s["wd"], s["M"], s["tail"], s["lam"], s["process"], scenario_seed, None, s["bounds"])["score"]
    return score


@functools.lru_cache(maxsize=None)
def reference(name):
    """The search of CASES[name] over policy_ref's case of that name, frozen."""
    c = policy_ref.case(name)
    K, E, I = CASES[name]
    return policy_ref._freeze(search(policy_scorer(c), c["params"][0], SIGMA0, K, E, I, SIGMA_MIN, SEED))
