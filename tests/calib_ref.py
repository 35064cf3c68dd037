"""TEST INFRASTRUCTURE — the reference for wake-model calibration (include/wfcalib.h): the loss of candidate parameter sets
against measured powers and the cross-entropy fit over the eighteen fields, restated in NumPy over the unchanged float64
oracle (one call per set, `ModelParams(**set)`, as tests/test_modelset_gpu.py: _oracle_by_set), with the deviate of
tests/plan_ref.py.  It modifies nothing of either.

The definition, as the header states it, for one problem g of C conditions and N turbines, S candidates, E elites,
iterations i = 0 .. I - 1 with widths sigma[i] (fractions of hi - lo):
  loss        L_s = sum_c ( sum_t w[c][t] * ((P_s[c][t] - P[c][t]) / scale)^2 ), float64, every operation rounded once, the
              inner sum in ascending t from 0.0, the outer one in ascending c from 0.0
  candidates  s = 0 the best set so far (iteration 0: init), s = 1 the mean mu (init before iteration 0),
              s >= 2, field f:  clip(mu_f + (sigma[i] * (hi_f - lo_f)) * z, lo_f, hi_f); lo_f == hi_f: lo_f exactly
  deviate     z = plan_ref.deviate(seed, g, s * 18 + f, stream = i)
  validity    ambient_ti, alpha, defl_alpha, ka * ambient_ti + kb, defl_ka * ambient_ti + defl_kb, ch_constant all > 0;
              an invalid candidate's loss is +inf and it is counted
  masking     an entry of weight 0 adds +0 whatever stands there (a NaN power too); a loss that is not finite is +inf
  update      rank_s = #{j: L_j < L_s or (L_j == L_s and j < s)}; elites rank < E;
              mu_f = (sum over the elites in ascending s of field f) / E;
              winner = the lowest loss, the lowest index among equals; a winner other than 0 becomes the best set

BOUND.  A device power is the float64 kernels' float32 output, inside parity.TOL_F64's power tolerance of the oracle's as
parity.within applies it to the reference power: delta[c][t] = TOL_F64["power"] * max(P_ref, 1 kW).  With e the reference's
residual, ((e + d)^2 - e^2) <= 2 |e| delta + delta^2 for |d| <= delta, so a loss is within
    bound = sum w * (2 |e| delta + delta^2) / scale^2
of the reference's.  An order of two losses is the same on both sides when they are further apart than the sum of their two
bounds; candidates with identical fields have identical losses on both sides (the lowest index wins on both), and so have two
invalid ones.  A problem's margin is the smallest |L_a - L_b| - (bound_a + bound_b) over every (elite, non-elite) pair and
every (winner, other) pair of differing candidates, over all iterations; the problem is SAFE when it is positive: the device
then has the reference's bits in best_set, mean and n_invalid."""
import functools

import numpy as np

import parity
import plan_ref

FIELDS = ("ambient_ti", "shear", "veer", "alpha", "beta", "ka", "kb", "ad", "bd", "dm", "ch_initial", "ch_constant", "ch_ai",
          "ch_downstream", "defl_alpha", "defl_beta", "defl_ka", "defl_kb")
NF = len(FIELDS)
# the library's default model as a set (include/wfstep.h: wf_default_model; tests/test_calib.py holds it against the oracle's)
DEFAULT = {"ambient_ti": 0.06, "shear": 0.12, "veer": 0.0, "alpha": 0.58, "beta": 0.077, "ka": 0.38, "kb": 0.004, "ad": 0.0,
           "bd": 0.0, "dm": 1.0, "ch_initial": 0.1, "ch_constant": 0.5, "ch_ai": 0.8, "ch_downstream": -0.32, "defl_alpha": 0.58,
           "defl_beta": 0.077, "defl_ka": 0.38, "defl_kb": 0.004}
RATED = 5.0e6  # the scale the tests pass, watts (nrel_5MW's plateau; any fixed positive number serves)


def as_array(sets):
    """(..., 18) float64 of a dict of fields (scalars or arrays) or a list of dicts; missing fields are DEFAULT's."""
    if isinstance(sets, dict):
        cols = [np.asarray(sets.get(f, DEFAULT[f]), np.float64) for f in FIELDS]
        shape = np.broadcast_shapes(*[c.shape for c in cols])
        return np.stack([np.broadcast_to(c, shape) for c in cols], axis=-1).copy()
    return np.stack([as_array(d) for d in sets])


def as_dict(a):
    """{field: array(...)} of an (..., 18) array: what WfStep.set_model_sets and model_loss accept."""
    a = np.asarray(a, np.float64)
    return {f: a[..., j].copy() for j, f in enumerate(FIELDS)}


def valid(a):
    """(...,) bool of (..., 18) sets: what wf_set_model_sets asks, with its roundings (product, then sum)."""
    a = np.asarray(a, np.float64)
    g = lambda f: a[..., FIELDS.index(f)]  # noqa: E731
    return ((g("ambient_ti") > 0.0) & (g("alpha") > 0.0) & (g("defl_alpha") > 0.0) & (g("ka") * g("ambient_ti") + g("kb") > 0.0)
            & (g("defl_ka") * g("ambient_ti") + g("defl_kb") > 0.0) & (g("ch_constant") > 0.0))


def powers(x, y, ws, wd, yaw, sets):
    """(S, C, N) float64: the oracle's powers of C conditions (ws, wd (C,), yaw (C, N)) under each of the (S, 18) sets."""
    from oracle import c_oracle
    from oracle.floris_gch_numpy import ModelParams

    sets = np.asarray(sets, np.float64).reshape(-1, NF)
    ws, wd = np.asarray(ws, np.float64), np.asarray(wd, np.float64)
    yaw = np.asarray(yaw, np.float64)
    out = np.empty((sets.shape[0],) + yaw.shape)
    for s, row in enumerate(sets):
        out[s] = c_oracle.farm_step_batch(x, y, ws, wd, yaw, ModelParams(**dict(zip(FIELDS, map(float, row)))))["power"]
    return out


def delta(pref):
    """The power tolerance of the float64 contract at the reference powers, watts (parity.within on parity.errors' scale)."""
    return parity.TOL_F64["power"] * np.maximum(pref, 1e3)


def loss(p, obs, weight=None, scale=RATED):
    """(L, bound), each (...,): p (..., C, N) powers, obs and weight (C, N); the header's order of operations."""
    p = np.asarray(p, np.float64)
    obs = np.asarray(obs, np.float64)
    w = np.ones(obs.shape) if weight is None else np.asarray(weight, np.float64)
    sc = np.float64(scale)
    e = p - obs
    q = e / sc
    term = np.where(w == 0.0, 0.0, w * (q * q))  # (a masked entry adds +0 whatever stands there, a NaN power too)
    C, N = obs.shape
    L = np.zeros(p.shape[:-2])
    for c in range(C):
        row = np.zeros(p.shape[:-2])
        for t in range(N):
            row = row + term[..., c, t]
        L = L + row
    d = delta(p)
    bound = np.where(w == 0.0, 0.0, w * (2.0 * np.abs(e) * d + d * d)).sum(axis=(-2, -1)) / (sc * sc)
    # a loss that is not finite (a NaN observation under a positive weight) counts as +inf, as an invalid candidate's does: a NaN
    # would compare false with everything, rank first and leave no winner.  All +inf: candidate 0 wins, the lowest index
    bad = ~np.isfinite(L)
    return np.where(bad, np.inf, L), np.where(bad, 0.0, bound)


def score(x, y, ws, wd, yaw, obs, sets, weight=None, scale=RATED):
    """One problem: dict(loss, bound (S,), best int, power (S, C, N)) of the (S, 18) valid sets."""
    p = powers(x, y, ws, wd, yaw, sets)
    L, b = loss(p, obs, weight, scale)
    return {"loss": L, "bound": b, "best": int(np.argmin(L)), "power": p}


def candidates(mu, best, lo, hi, sigma_i, seed, g, i, S):
    """(S, 18) float64 candidates of iteration i of problem g from mu, best (18,)."""
    a = np.empty((S, NF))
    a[0], a[1] = best, mu
    if S > 2:
        idx = np.arange(2 * NF, S * NF, dtype=np.uint64).reshape(S - 2, NF)
        z = plan_ref.deviate(seed, np.uint64(g), idx, i)
        width = np.float64(sigma_i) * (hi - lo)
        a[2:] = np.clip(mu + width * z, lo, hi)
        a[2:] = np.where(lo == hi, lo, a[2:])
    return a


def ranks(L):
    """rank_s = #{j: L_j < L_s or (L_j == L_s and j < s)} along the last axis."""
    S = L.shape[-1]
    j, s = np.arange(S)[:, None], np.arange(S)[None, :]
    lj, ls = L[..., :, None], L[..., None, :]
    return ((lj < ls) | ((lj == ls) & (j < s))).sum(axis=-2)


def elite_mean(a, elite, E):
    """(18,): the sum of a (S, 18) over the elite rows in ascending s, one division by E."""
    s = np.zeros(a.shape[1])
    for k in range(a.shape[0]):
        if elite[k]:
            s = s + a[k]
    return s / np.float64(E)


def _margin(L, b, a, elite, w):
    m = np.inf
    S = L.shape[0]
    for p in range(S):
        for q in range(S):
            decides = (elite[p] and not elite[q]) or (p == w and q != p)
            if not decides or np.array_equal(a[p], a[q]) or (np.isinf(L[p]) and np.isinf(L[q])):
                continue
            m = min(m, abs(L[p] - L[q]) - (b[p] + b[q]))
    return m


def fit(x, y, ws, wd, yaw, obs, lo, hi, init, S, E, sigma, seed, weight=None, scale=RATED, problem_index=None):
    """G problems: ws, wd (G, C), yaw, obs, weight (G, C, N), lo, hi (18,), init (G, 18) or (18,).  Returns dict(best_set, mean
    (G, 18), best_loss, init_loss, best_bound, init_bound (G,), history, history_bound (G, I), fit_power (G, C, N) float64,
    n_invalid (G,) int, margin (G,), safe (G,) bool, winners (G, I))."""
    ws, wd = np.atleast_2d(np.asarray(ws, np.float64)), np.atleast_2d(np.asarray(wd, np.float64))
    G = ws.shape[0]
    yaw, obs = np.asarray(yaw, np.float64).reshape(G, ws.shape[1], -1), np.asarray(obs, np.float64).reshape(G, ws.shape[1], -1)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    init = np.broadcast_to(np.asarray(init, np.float64), (G, NF))
    sigma = np.asarray(sigma, np.float64).reshape(-1)
    idx = np.arange(G) if problem_index is None else np.asarray(problem_index)
    out = {k: [] for k in ("best_set", "mean", "best_loss", "init_loss", "best_bound", "init_bound", "history", "history_bound",
                           "fit_power", "n_invalid", "margin", "winners")}
    for g in range(G):
        assert valid(init[g]) and (init[g] >= lo).all() and (init[g] <= hi).all()
        wg = None if weight is None else np.asarray(weight, np.float64)[g]
        mu, best = init[g].copy(), init[g].copy()
        margin, n_invalid, hist, hb, wins = np.inf, 0, [], [], []
        for i, sg in enumerate(sigma):
            a = candidates(mu, best, lo, hi, sg, seed, idx[g], i, S)
            ok = valid(a)
            n_invalid += int((~ok).sum())
            L, b = np.full(S, np.inf), np.zeros(S)
            p = np.zeros((S,) + yaw[g].shape)
            p[ok] = powers(x, y, ws[g], wd[g], yaw[g], a[ok])
            L[ok], b[ok] = loss(p[ok], obs[g], wg, scale)
            elite = ranks(L) < E
            assert elite.sum() == E
            w = int(np.argmin(L))  # (the first of equal minima)
            margin = min(margin, _margin(L, b, a, elite, w))
            if i == 0:
                init_loss, init_bound = L[0], b[0]
            mu = elite_mean(a, elite, E)
            if w != 0 or i == 0:
                best, best_loss, best_bound, fit_power = a[w].copy(), L[w], b[w], p[w].copy()
            hist.append(L[w]); hb.append(b[w]); wins.append(w)
        for k, v in (("best_set", best), ("mean", mu), ("best_loss", best_loss), ("init_loss", init_loss), ("best_bound", best_bound),
                     ("init_bound", init_bound), ("history", hist), ("history_bound", hb), ("fit_power", fit_power),
                     ("n_invalid", n_invalid), ("margin", margin), ("winners", wins)):
            out[k].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    out["safe"] = out["margin"] > 0.0
    return out


# ---- the cases the GPU tests run, with their references computed once (tests/test_calib.py asserts they are safe) ----
ROW3 = (np.array([0.0, 630.0, 1260.0]), np.array([0.0, 0.0, 0.0]))  # three turbines in a row, 5 D apart
FIT_FREE = {"ambient_ti": (0.03, 0.15), "ka": (0.2, 0.6), "alpha": (0.3, 0.9)}
FIT_TRUTH = ({"ambient_ti": 0.08, "ka": 0.3, "alpha": 0.7}, {"ambient_ti": 0.05, "ka": 0.45, "alpha": 0.5})
FIT = dict(S=16, E=4, sigma=(0.25, 0.12, 0.06), G=2, C=4)
FIT_SEEDS = {"row3": 1, "Ablaincourt_": 1}
# bounds that let ka * ambient_ti + kb go non-positive: ka below -kb / TI = -0.0667
INVALID_FREE = {"ka": (-0.6, 0.5), "ambient_ti": (0.04, 0.1)}
INVALID = dict(S=24, E=4, sigma=(0.6, 0.4), G=1, C=2, seed=3)


def layout(name):
    import json
    import os

    if name == "row3":
        return ROW3
    from conftest import ROOT

    with open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")) as f:
        l = json.load(f)[name]
    return np.asarray(l["xcoords"], np.float64), np.asarray(l["ycoords"], np.float64)


def conditions(name, G, C, seed=0):
    """(ws, wd (G, C), yaw (G, C, N) float32): winds about the layout's wake directions and yaws a controller would hold."""
    import zlib

    N = layout(name)[0].size
    rng = np.random.default_rng(zlib.crc32(f"calib/{name}/{G}/{C}/{seed}".encode()))
    ws = rng.uniform(7.0, 10.5, (G, C))
    wd = 270.0 + rng.uniform(-12.0, 12.0, (G, C))
    yaw = rng.uniform(-20.0, 20.0, (G, C, N)).astype(np.float32)
    return ws, wd, yaw


def bounds_arrays(free, init=None):
    """(lo, hi, init) (18,) each: the free fields' bounds, every other field fixed at init (None: DEFAULT)."""
    init = as_array(DEFAULT if init is None else init)
    lo, hi = init.copy(), init.copy()
    for f, (a, b) in free.items():
        lo[FIELDS.index(f)], hi[FIELDS.index(f)] = a, b
    return lo, hi, init


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """The twin problem on `name`: G problems with different truths, measurements from the oracle at the truth."""
    x, y = layout(name)
    G, C = FIT["G"], FIT["C"]
    ws, wd, yaw = conditions(name, G, C)
    truth = as_array(list(FIT_TRUTH))
    obs = np.stack([powers(x, y, ws[g], wd[g], yaw[g], truth[g:g + 1])[0] for g in range(G)])
    lo, hi, init = bounds_arrays(FIT_FREE)
    return dict(x=x, y=y, ws=ws, wd=wd, yaw=yaw, obs=obs, truth=truth, lo=lo, hi=hi, init=init, seed=FIT_SEEDS[name], **FIT)


@functools.lru_cache(maxsize=None)
def fit_reference(name, seed=None):
    c = fit_case(name)
    return fit(c["x"], c["y"], c["ws"], c["wd"], c["yaw"], c["obs"], c["lo"], c["hi"], c["init"], c["S"], c["E"], c["sigma"],
               c["seed"] if seed is None else seed)


@functools.lru_cache(maxsize=None)
def invalid_case():
    x, y = layout("row3")
    G, C = INVALID["G"], INVALID["C"]
    ws, wd, yaw = conditions("row3", G, C, seed=1)
    obs = np.stack([powers(x, y, ws[g], wd[g], yaw[g], as_array(FIT_TRUTH[0])[None])[0] for g in range(G)])
    lo, hi, init = bounds_arrays(INVALID_FREE)
    ref = fit(x, y, ws, wd, yaw, obs, lo, hi, init, INVALID["S"], INVALID["E"], INVALID["sigma"], INVALID["seed"])
    return dict(x=x, y=y, ws=ws, wd=wd, yaw=yaw, obs=obs, lo=lo, hi=hi, init=init, ref=ref, **INVALID)
