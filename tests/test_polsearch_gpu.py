"""GPU: policy search on the device (include/wfpolsearch.h) against tests/search_ref.py's parts.

A closed loop — and a search around it — is never compared run against run.  As in tests/policy_links.py EACH LINK is checked
against the device's OWN upstream values, so no closeness-to-a-decision condition is needed:
  1. candidates: search_ref.candidates of the device's mean (candidates[i][1]), sigma_history[i] and incumbent (candidates[i][0])
     reproduces candidates[i], bit for bit;
  2. scorer: policy_returns(candidates[i]) — with members policy_scenarios(...)["score"] — on the same handle, same strict, same
     max_eval_farms, same farms returns farm_scores[i], bit for bit, in both modes;
  3. aggregate: search_ref.aggregate(farm_scores[i]) is fitness[i], bits;
  4. refit: search_ref.refit(candidates[i], fitness[i]) gives winner[i] and the next mean (bits) and the next sigma (one float32
     ulp; the count of entries that differ is printed, bits are expected); the next incumbent is the winner's row;
  5. invariants: fitness[i][0] has the bits of max fitness[i - 1]; the start is improved by more than 1e-2 on the four cases;
     env state and wind unchanged; two runs, host and device arrays the same bits; a warm start runs.
Then the shapes at which each kernel takes another path, the refusals by name, kernel_info and the VecWindFarmEnv method."""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_links as links
import policy_ref as pr
import polscen_ref
import search_ref as sr
import yawopt_ref

pytestmark = pytest.mark.gpu

WANT = ("best_params", "best_fitness", "init_fitness", "mean", "sigma", "fitness", "winner", "candidates", "sigma_history", "farm_scores")
MODES = (True, False)
KEYS = ("ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp")
PROCESS = dict(zip(KEYS, polscen_ref.PROCESS))

_bits, _same = links.bits, links.same


def _handle(c, ws=None, wd=None):
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["B"])
    w.set_wind(c["ws"] if ws is None else ws, c["wd"] if wd is None else wd)
    w.env_config(load_coef=pr.LOAD_COEF, discrete=c["env"]["discrete"], dt=c["env"]["dt"])
    w.env_reset()
    w.env_set_state(c["state"])
    return w


def _search(w, c, strict, K, E, I, **kw):
    kw.setdefault("want", WANT)
    kw.setdefault("sigma", sr.SIGMA0)
    kw.setdefault("sigma_min", sr.SIGMA_MIN)
    kw.setdefault("seed", sr.SEED)
    kw.setdefault("wind", c["wind"])
    kw.setdefault("mean", c["params"][0])
    mean = kw.pop("mean")
    return w.search_policy(mean, c["spec"], c["H"], candidates=K, elites=E, iterations=I, gamma=c["gamma"], strict=strict, **kw)


def _rescore(w, c, got, strict, **kw):
    """policy_returns of every iteration's candidates on the same handle: (I, n, K)."""
    kw.setdefault("wind", c["wind"])
    return np.stack([w.policy_returns(got["candidates"][i], c["spec"], c["H"], gamma=c["gamma"], strict=strict, want=("returns",), **kw)["returns"]
                     for i in range(got["candidates"].shape[0])])


def _check_links(got, rescored, mean0, sigma0, K, E, I, sigma_min, seed, n):
    """Links 1 to 4 and the bit invariants of 5 on one run's outputs; `rescored` (I, n, K) is the scorer's own answer to the
    device's candidates."""
    P = np.asarray(mean0).size
    f8, f4, i4 = np.float64, np.float32, np.int32
    shapes = {"best_params": ((P,), f4), "best_fitness": ((), f8), "init_fitness": ((), f8), "mean": ((P,), f4), "sigma": ((P,), f4),
              "fitness": ((I, K), f8), "winner": ((I,), i4), "candidates": ((I, K, P), f4), "sigma_history": ((I, P), f4),
              "farm_scores": ((I, n, K), f8)}
    for k, (shape, d) in shapes.items():
        assert got[k].shape == shape and got[k].dtype == d, k
    cand, hist, fit, win = got["candidates"], got["sigma_history"], got["fitness"], got["winner"]
    sigma0 = np.broadcast_to(np.asarray(sigma0, np.float32), (P,))
    assert _same(cand[0, 0], np.asarray(mean0, np.float32)) and _same(cand[0, 1], np.asarray(mean0, np.float32))
    assert _same(hist[0], np.ascontiguousarray(sigma0))
    off = 0
    for i in range(I):
        assert _same(sr.candidates(cand[i, 1], hist[i], cand[i, 0], seed, i, K), cand[i]), ("candidates", i)  # link 1
        assert _same(rescored[i], got["farm_scores"][i]), ("scorer", i)                                       # link 2
        assert _same(sr.aggregate(got["farm_scores"][i]), fit[i]), ("aggregate", i)                           # link 3
        w, mean, sigma, _ = sr.refit(cand[i], fit[i], E, sigma_min)                                           # link 4
        assert w == win[i], ("winner", i)
        nxt_mean, nxt_sigma, nxt_inc = (cand[i + 1, 1], hist[i + 1], cand[i + 1, 0]) if i + 1 < I else (got["mean"], got["sigma"], got["best_params"])
        assert _same(mean, nxt_mean), ("mean", i)
        ulp = np.abs(_bits(sigma).astype(np.int64) - _bits(nxt_sigma).astype(np.int64))
        off += int((ulp != 0).sum())
        assert ulp.max() <= 1, ("sigma", i)
        assert _same(cand[i, win[i]], nxt_inc), ("incumbent", i)
        if i > 0:
            assert _bits(fit[i, 0]) == _bits(fit[i - 1].max()), ("F_i[0]", i)                                  # 5
    print("sigma entries that differ from the reference's by one ulp:", off)
    assert _bits(got["best_fitness"]) == _bits(fit[-1, win[-1]]) and _bits(got["best_fitness"]) == _bits(fit.max())
    assert _bits(got["init_fitness"]) == _bits(fit[0, 0]) and got["best_fitness"] >= got["init_fitness"]


@functools.lru_cache(maxsize=None)
def _device(name, strict):
    c = pr.case(name)
    K, E, I = sr.CASES[name]
    w = _handle(c)
    before, wind_before = w.env_get_state(), w.get_wind()
    got = _search(w, c, strict, K, E, I)
    after, wind_after = w.env_get_state(), w.get_wind()
    again = _search(w, c, strict, K, E, I)
    rescored = _rescore(w, c, got, strict)
    w.close()
    for v in got.values():
        v.setflags(write=False)
    return got, rescored, again, (before, after, wind_before, wind_after)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("name", sr.NAMES)
def test_every_link_on_the_four_cases(name, strict):
    """Links 1 to 5 on the cases of the reference's prototype: P = 726, 78, 1932 (eight workgroups along p, no multiple
    of 64) and 38 (the discrete encoding)."""
    c = pr.case(name)
    K, E, I = sr.CASES[name]
    got, rescored, again, (before, after, wind_before, wind_after) = _device(name, strict)
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, K, E, I, sr.SIGMA_MIN, sr.SEED, c["B"])
    print(name, strict, "init_fitness -> best_fitness", float(got["init_fitness"]), float(got["best_fitness"]))
    assert got["best_fitness"] > got["init_fitness"] + 1e-2
    for k in before:  # the env state and the wind are read, never written
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(wind_before[0], wind_after[0]) and np.array_equal(wind_before[1], wind_after[1])
    for k in WANT:  # two runs give the same bits
        assert _same(got[k], again[k]), k
    # the draws are the reference's own (they depend on seed, k, p, i only), so iteration 0's candidates are its bits
    assert _same(got["candidates"][0], sr.reference(name)["candidates"][0])


@pytest.mark.parametrize("strict", MODES)
def test_host_and_device_arrays_and_a_warm_start(strict):
    import torch

    name = "row3_central"
    c = pr.case(name)
    K, E, I = sr.CASES[name]
    got = _device(name, strict)[0]
    w = _handle(c)
    dev = _search(w, c, strict, K, E, I, mean=torch.as_tensor(np.array(c["params"][0])).cuda(), wind=torch.as_tensor(np.array(c["wind"])).cuda())
    for k in WANT:
        assert dev[k].is_cuda and _same(dev[k].cpu().numpy(), got[k]), k
    short = _search(w, c, strict, K, E, I, want=("best_fitness",))  # only one output asked for: the same search
    assert set(short) == {"best_fitness"} and _bits(short["best_fitness"]) == _bits(got["best_fitness"])
    warm = _search(w, c, strict, K, E, 2, mean=got["mean"], sigma=got["sigma"], seed=sr.SEED + 1)
    rescored = _rescore(w, c, warm, strict)
    w.close()
    _check_links(warm, rescored, got["mean"], got["sigma"], K, E, 2, sr.SIGMA_MIN, sr.SEED + 1, c["B"])
    assert warm["init_fitness"] <= warm["best_fitness"]
    assert not _same(warm["candidates"][0, 2:], got["candidates"][0, 2:])


# ---- the shapes at which each kernel takes another path: the row of three, 2 farms, H = 2 ----------------------------------
def _small(B=2, K=3, hidden=(5,), kind="shared", discrete=False, seed=31, inputs=None):
    row = ("row3", B, kind, hidden, "relu", None if discrete else "tanh", False, discrete, K, 2, False, seed)
    return pr.build("small", row, inputs=inputs)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("K,E,I", [(3, 1, 1), (3, 3, 16), (64, 1, 2), (64, 64, 2), (64, 7, 1)])
def test_limits_of_K_E_and_I(K, E, I, strict):
    """P = 26 (shared 3-5-1), K = 3 and 64, E = 1 and K, I = 1 and 16; E = 1 gives sigma = sigma_min from the first refit on."""
    c = _small()
    assert c["params"].shape[1] == 26
    w = _handle(c)
    got = _search(w, c, strict, K, E, I)
    rescored = _rescore(w, c, got, strict)
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, K, E, I, sr.SIGMA_MIN, sr.SEED, 2)
    if E == 1:
        assert (got["sigma_history"][1:] == np.float32(sr.SIGMA_MIN)).all() and (got["sigma"] == np.float32(sr.SIGMA_MIN)).all()
        assert _same(got["mean"], got["best_params"])


@pytest.mark.parametrize("strict", MODES)
def test_a_vector_longer_than_one_pass(strict):
    """P = 8705 (shared 3-64-128-1): more than the 8192 elements the advance's 32 workgroups along p cover in one pass, and no
    multiple of 64; K = 11: two slices of candidate rows, the second partial."""
    c = _small(hidden=(64, 128))
    assert c["params"].shape[1] == 8705
    w = _handle(c)
    got = _search(w, c, strict, 11, 3, 2)
    rescored = _rescore(w, c, got, strict)
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, 11, 3, 2, sr.SIGMA_MIN, sr.SEED, 2)


@pytest.mark.parametrize("strict", MODES)
def test_one_farm_and_two_tiles(strict):
    """n = 1; and n = 300 farms of the row of three with K = 3, H = 2: two tiles of list positions, the second partial."""
    c = _small(B=1)
    w = _handle(c)
    got = _search(w, c, strict, 3, 2, 2)
    rescored = _rescore(w, c, got, strict)
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, 3, 2, 2, sr.SIGMA_MIN, sr.SEED, 1)
    assert _same(got["fitness"], got["farm_scores"][:, 0])  # one farm: its score is the fitness
    rng = np.random.default_rng(8)
    x, y = yawopt_ref.gpu_input("row3")[:2]
    c = _small(B=300, inputs=(x, y, rng.uniform(6.0, 11.0, 300), rng.uniform(0.0, 360.0, 300)))
    w = _handle(c)
    got = _search(w, c, strict, 3, 2, 2)
    rescored = _rescore(w, c, got, strict)
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, 3, 2, 2, sr.SIGMA_MIN, sr.SEED, 300)
    one_walk = got["farm_scores"][0].sum(axis=0) / 300.0
    assert np.allclose(got["fitness"][0], one_walk, rtol=1e-12)


def test_three_chunks_of_the_scorer_give_the_one_chunk_fitness():
    """7 farms, K = 3: max_eval_farms = 9 makes the scorer run chunks of 3, 3 and 1 farms.  In strict mode the fitness bits are
    the one-chunk run's; the links hold under the same max_eval_farms."""
    c = pr.case("abl_central")
    w = _handle(c)
    whole = _search(w, c, True, 3, 2, 2)
    parts = _search(w, c, True, 3, 2, 2, max_eval_farms=9)
    rescored = _rescore(w, c, parts, True, max_eval_farms=9)
    w.close()
    for k in WANT:
        assert _same(whole[k], parts[k]), k
    _check_links(parts, rescored, c["params"][0], sr.SIGMA0, 3, 2, 2, sr.SIGMA_MIN, sr.SEED, 7)


@pytest.mark.parametrize("strict", MODES)
def test_a_farm_list_is_followed_in_its_order(strict):
    """A permuted subset: farm_scores and fitness follow the list's order; the draws do not depend on the list."""
    c = pr.case("abl_central")
    farms = [5, 0, 3]
    w = _handle(c)
    got = _search(w, c, strict, 4, 2, 2, farms=farms, wind=np.ascontiguousarray(c["wind"][farms]))
    rescored = _rescore(w, c, got, strict, farms=farms, wind=np.ascontiguousarray(c["wind"][farms]))
    alone = np.stack([w.policy_returns(got["candidates"][0], c["spec"], c["H"], gamma=c["gamma"], strict=True, farms=[f],
                                       wind=np.ascontiguousarray(c["wind"][[f]]), want=("returns",))["returns"][0] for f in farms])
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, 4, 2, 2, sr.SIGMA_MIN, sr.SEED, 3)
    if strict:
        assert _same(alone, got["farm_scores"][0])
    assert _same(got["candidates"][0], _device("abl_central", strict)[0]["candidates"][0][:4])  # (nor on K)


@pytest.mark.parametrize("strict", MODES)
def test_a_weight_without_width_never_moves(strict):
    c = _small(discrete=True, K=3)
    mean0 = c["params"][0]
    sigma0 = np.full(mean0.size, 0.4, np.float32)
    frozen = np.array([0, 7, mean0.size - 1])
    sigma0[frozen] = 0.0
    w = _handle(c)
    got = _search(w, c, strict, 6, 3, 4, sigma=sigma0, sigma_min=0.0)
    rescored = _rescore(w, c, got, strict)
    w.close()
    _check_links(got, rescored, mean0, sigma0, 6, 3, 4, 0.0, sr.SEED, 2)
    held = got["candidates"][:, :, frozen]
    assert np.array_equal(_bits(held), np.broadcast_to(_bits(mean0[frozen]), held.shape))
    assert _same(got["mean"][frozen], mean0[frozen]) and _same(got["best_params"][frozen], mean0[frozen])
    assert (got["sigma"][frozen] == 0.0).all() and (got["sigma_history"][:, frozen] == 0.0).all()


@pytest.mark.parametrize("strict", MODES)
def test_members_score_through_policy_scenarios(strict):
    """members = 2, tail = 1: the farm scores are policy_scenarios' score of the candidates on the same handle, under the same
    scenario_seed in every iteration."""
    s = polscen_ref.case("row3_central")
    c = s["c"]
    K, E, I = 4, 2, 2
    kw = dict(members=2, process=PROCESS, scenario_seed=polscen_ref.SEED, tail=1, risk_weight=0.5, bounds=s["bounds"])
    w = _handle(c, s["ws"], s["wd"])
    before = w.env_get_state()
    got = _search(w, c, strict, K, E, I, wind=None, **kw)
    after = w.env_get_state()
    rescored = np.stack([w.policy_scenarios(got["candidates"][i], c["spec"], c["H"], 2, PROCESS, seed=polscen_ref.SEED, gamma=c["gamma"],
                                            tail=1, risk_weight=0.5, bounds=s["bounds"], strict=strict, want=("score",))["score"]
                         for i in range(I)])
    held = _search(w, c, strict, K, E, I, wind=None, want=("farm_scores",))["farm_scores"]
    w.close()
    _check_links(got, rescored, c["params"][0], sr.SIGMA0, K, E, I, sr.SIGMA_MIN, sr.SEED, c["B"])
    assert not _same(held, got["farm_scores"])  # (the ensemble is not the held wind)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_refusals_by_name():
    from wfcrl_env_amd import _lib
    from wfcrl_env_amd import policy as P
    from wfcrl_env_amd.backend import WfStep

    c = _small()
    spec, mean = c["spec"], c["params"][0]
    w = _handle(c)

    def run(**kw):
        a = dict(mean=mean, spec=spec, H=2, K=4, E=2, I=2)
        a.update(kw)
        m, sp, H, K, E, I = (a.pop(k) for k in ("mean", "spec", "H", "K", "E", "I"))
        return w.search_policy(m, sp, H, candidates=K, elites=E, iterations=I, **a)

    for K in (2, 65):
        with pytest.raises(ValueError, match="WF_E_INVALID.*candidates K must be in 3..64"):
            run(K=K)
    for E in (0, 5):
        with pytest.raises(ValueError, match="WF_E_INVALID.*elites E must be in 1..K"):
            run(E=E)
    for I in (0, 17):
        with pytest.raises(ValueError, match="WF_E_INVALID.*iterations I must be in 1..16"):
            run(I=I)
    for bad in (np.nan, np.inf):
        m = mean.copy()
        m[3] = bad
        with pytest.raises(ValueError, match="WF_E_INVALID.*mean0 must be finite"):
            run(mean=m)
    for bad in (-0.1, np.nan, np.inf):
        sg = np.full(mean.size, 0.3, np.float32)
        sg[5] = bad
        with pytest.raises(ValueError, match="WF_E_INVALID.*sigma0 must be finite and >= 0"):
            run(sigma=sg)
        with pytest.raises(ValueError, match="WF_E_INVALID.*sigma_min must be finite and >= 0"):
            run(sigma_min=bad)
    with pytest.raises(ValueError, match="WF_E_INVALID.*parameter vector of the wrong length"):  # the scorer's own message
        run(mean=mean[:-1])
    with pytest.raises(ValueError, match="sigma must be a scalar or"):
        run(sigma=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..256"):
        run(H=0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*H must be in 1..64"):
        run(H=65, members=2, process=PROCESS)
    with pytest.raises(ValueError, match="WF_E_INVALID.*M must be in 1..64"):
        run(members=65, process=PROCESS)
    with pytest.raises(ValueError, match="WF_E_INVALID.*tail must be in 1..M"):
        run(members=2, tail=3, process=PROCESS)
    with pytest.raises(ValueError, match="WF_E_INVALID.*anchor's speed"):
        run(members=2, process=PROCESS, anchor=np.array([[8.0, 270.0], [0.0, 270.0]]))
    with pytest.raises(ValueError, match="WF_E_INVALID.*gamma"):
        run(gamma=1.5)
    with pytest.raises(ValueError, match="WF_E_INVALID.*max_eval_farms must hold one farm's rows: at least K"):
        run(max_eval_farms=3)
    with pytest.raises(ValueError, match="WF_E_INVALID.*output width does not match"):
        run(mean=np.zeros(P.param_count((3, 5, 3)), np.float32), spec=P.mlp_spec("shared", (3, 5, 3), "relu"))
    with pytest.raises(ValueError, match="farm index out of range"):
        run(farms=[0, 2])
    with pytest.raises(ValueError, match="wind and members exclude each other"):
        run(members=2, process=PROCESS, wind=np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="members must be >= 1"):
        run(members=0, process=PROCESS)
    with pytest.raises(ValueError, match="want must name"):
        run(want=("returns",))
    with pytest.raises(ValueError, match="has not run yet"):
        w.search_policy_timing()
    r = run(farms=[1])  # (the handle still serves)
    assert np.isfinite(r["best_fitness"]) and r["best_params"].shape == mean.shape
    w.close()

    # the C entry points themselves: an object created without a polscen object, and policy objects that hold no network
    w = _handle(c)
    lib = w._lib
    obj = C.c_void_p()
    assert lib.wf_polsearch_create(w._h, None, None, C.byref(obj)) == -1  # WF_E_INVALID: the policy object is NULL
    pol = w._policy()
    assert lib.wf_polsearch_create(w._h, pol._r, None, C.byref(obj)) == 0
    sg = np.full(mean.size, 0.3, np.float32)
    proc = _lib.WindProcess(**PROCESS)

    def raw(M):
        return lib.wf_polsearch_run(obj, mean.ctypes.data, sg.ctypes.data, mean.size, 4, 2, 2, 0.0, C.c_ulonglong(1), 2, 1.0, None, M,
                                    C.byref(proc), 3.0, 28.0, C.c_ulonglong(0), 1, 0.0, None, 2, None, *([None] * 10), 0)

    assert raw(2) == -1 and b"created without a polscen object" in lib.wf_polsearch_last_error(obj)
    assert raw(0) == -1 and b"no network: wf_policy_set_network comes first" in lib.wf_polsearch_last_error(obj)
    pol._set_network(spec)
    assert raw(0) == 0  # (with a network the same call serves)
    assert lib.wf_polsearch_destroy(obj) == 0
    w.close()
    w = WfStep(c["x"], c["y"], env_batch=2)  # no env state: the scorer's refusal
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="WF_E_INVALID.*no env state"):
        w.search_policy(mean, spec, 2, candidates=4, elites=2, iterations=1)
    w.close()


def test_kernel_info_and_timing():
    c = _small()
    w = _handle(c)
    info = w.search_policy_kernel_info()
    assert set(info) == {"tiles", "advance"}
    for k, v in info.items():
        assert v["scratch_bytes"] == 0 and v["vgprs"] > 0 and v["lds_bytes"] == 0, (k, v)
    w.search_policy_timing(detail=True)
    _search(w, c, False, 8, 2, 3, want=("best_fitness",))
    t = w.search_policy_timing()
    w.close()
    assert t["total_ms"] > 0.0 and t["step_ms"] > 0.0 and t["glue_ms"] > 0.0
    assert t["step_ms"] + t["glue_ms"] <= t["total_ms"] * 1.01 + 1e-3


def test_vec_env_method_returns_torch():
    """VecWindFarmEnv.search_policy on an env that returns torch: CUDA tensors, an nn.Sequential taken through
    policy_from_torch, the bits of WfStep.search_policy given NumPy arrays on the same state; with members the env's
    wind_process and bounds; a shaped reward is refused; the env is left as it was."""
    import torch
    import torch.nn as nn

    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd import policy as P

    B, H = 3, 2
    process = dict(ws_revert=0.1, ws_sigma=0.4, wd_revert=0.1, wd_sigma=3.0, wd_ramp=2.0, dist=dict(wd_mean=265.0, wd_std=10.0))
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=12, load_coef=pr.LOAD_COEF, wind_process=process)
    N = env.num_turbines
    env.reset(seed=11)
    env.step({"yaw": torch.full((B, N), 2.0).cuda()})
    torch.manual_seed(2)
    net = nn.Sequential(nn.Linear(3, 5), nn.Softsign(), nn.Linear(5, 1), nn.Softsign())
    kw = dict(kind="shared", out_scale=5.0, scale=np.full(3, 0.01))
    before = env.fi.env_get_state()
    want = ("best_params", "best_fitness", "init_fitness", "fitness")
    r = env.search_policy(net, H, sigma=0.2, candidates=4, elites=2, iterations=2, seed=3, members=2, scenario_seed=5, tail=1, want=want, **kw)
    after = env.fi.env_get_state()
    params, spec = P.policy_from_torch(net, **kw)
    proc = {k: process[k] for k in KEYS}
    bounds = (float(env._wind_dist.get("ws_lo", 3.0)), float(env._wind_dist.get("ws_hi", 28.0))) if env._wind_dist is not None else (3.0, 28.0)
    direct = env.fi.search_policy(np.asarray(params)[0], spec, H, sigma=0.2, candidates=4, elites=2, iterations=2, seed=3, members=2,
                                  process=proc, scenario_seed=5, tail=1, bounds=bounds, want=want)
    env.close()
    for k in want:
        assert r[k].is_cuda and _same(r[k].cpu().numpy(), direct[k]), k
    assert tuple(r["fitness"].shape) == (2, 4) and r["best_fitness"] >= r["init_fitness"]
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    env = envs.make("Ablaincourt_Floris", env_batch=2, max_num_steps=5, return_torch=False)  # no wind_process
    env.reset(seed=0)
    start = (np.zeros((1, P.param_count((3, 1))), np.float32), P.mlp_spec("shared", (3, 1)))
    with pytest.raises(ValueError, match="built without wind_process"):
        env.search_policy(start, 2, candidates=3, elites=1, iterations=1, members=2)
    r = env.search_policy(start, 2, candidates=3, elites=1, iterations=1)
    assert isinstance(r["best_params"], np.ndarray) and r["best_params"].shape == (4,)
    env.reward_shaper = type("Shaped", (), {})()
    with pytest.raises(ValueError, match="search_policy needs the plain reward"):
        env.search_policy(start, 2, candidates=3, elites=1, iterations=1)
    env.close()
