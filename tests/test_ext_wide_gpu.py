"""GPU: the extensions' glue kernels past one wave, one LDS tile and one pass of their strided loops, against the references
the extensions already have (grad_ref, credit_ref, lookahead_ref, plan_ref, yawopt_ref, robust_ref over the float64 oracle) on
the cases of tests/ext_wide_cases.py: N = 65 and 256, K = 300 and 1537.  tests/test_ext_wide.py shows on the CPU that every
case reaches the branch it is for — the tile loops of wf_staged_row_rewards and wf_grad_reduce_kernel with their offsets
and ragged last tiles, the 256-thread launch of wf_plan_advance_kernel, K beyond the threads of a block, the even reward
stride, the `t += 64` loops of the search kernels — and that the references decide clearly.

No tolerance is new.  Rewards, farm powers, differences and returns are held to credit_ref.bound / power_bound and
lookahead_ref.discounts (parity.TOL_F64 strict, parity.TOL in the default mode), the sensitivities to the bound of
tests/test_grad_gpu.py, the searches to MARGIN, YAW_TOL and POW_TOL of tests/test_yawopt_gpu.py through its (and
tests/test_robust_gpu.py's) _check_against_reference, and bits wherever the small-shape tests assert bits.  Every test prints
its largest error / bound before it asserts.  A handle per case, closed in `finally`."""
import numpy as np
import pytest

import credit_ref
import ext_wide_cases as wc
import lookahead_ref
import parity
import robust_ref
import yawopt_ref
from ext_wide_cases import GAMMA, GRAD_BOUNDS, LOAD_COEF, PASSES
from test_lookahead import PARAMS
from test_robust_gpu import _check_against_reference as _check_robust_search
from test_yawopt_gpu import POW_TOL, _check_against_reference as _check_search

pytestmark = pytest.mark.gpu


def _open(c, env=False):
    from wfcrl_env_amd.backend import WfStep

    w = WfStep(c["x"], c["y"], env_batch=c["farms"])
    w.set_wind(c["ws"], c["wd"])
    if env:
        w.env_config(load_coef=LOAD_COEF, discrete=False, dt=PARAMS["dt"])
        if "state" in c:
            w.env_reset()
            w.env_set_state(c["state"])
    return w


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view))


# ---- grad -------------------------------------------------------------------------------------------------------------------
GRAD_KEYS = ("power", "gradient", "jacobian")


def _check_grad(name, one, rnd, tol, mode):
    """The inequalities of tests/test_grad_gpu.py: _check — |J_dev - J_ref|[i][j] <= tol (max(P+_j, 1e3) + max(P-_j, 1e3)) / d_i,
    |G_dev - G_ref|[i] <= sum_j |c_j| x that, the forward power inside tol — with c = 1 and with the case's cotangent, and
    of test_gradient_is_the_jacobian_contracted: G against the device's own J within 1e-12 sum_j |c_j J[i][j]|."""
    c, ref = wc.case(name), wc.reference(name)
    B, N = c["yaw"].shape
    assert one["power"].shape == (B, N) and one["power"].dtype == np.float32
    assert one["gradient"].shape == (B, N) and one["gradient"].dtype == np.float64 and one["jacobian"].shape == (B, N, N)
    assert (ref["d"] >= 1.0).all() and (ref["d"] < 1.9).any()  # (one-sided quotients next to the bounds; none is dead)
    jb = tol * (np.maximum(ref["p_plus"], 1e3) + np.maximum(ref["p_minus"], 1e3)) / ref["d"][:, :, None]  # [b, i, j]
    for tag, got, cc, g_ref in (("c = 1", one, np.ones((B, N)), ref["gradient"]), ("random c", rnd, c["cot"].astype(np.float64), ref["g_c"])):
        ej = np.abs(got["jacobian"] - ref["jacobian"])
        gb = (np.abs(cc)[:, None, :] * jb).sum(axis=2)
        eg = np.abs(got["gradient"] - g_ref)
        ep = np.abs(got["power"].astype(np.float64) - ref["power"]) / np.maximum(ref["power"], 1e3)
        terms = cc[:, None, :] * got["jacobian"]
        ec = np.abs(got["gradient"] - terms.sum(axis=2))
        print(f"{name} {mode}, {tag}: largest error / bound: Jacobian {(ej / jb).max():.3f}, gradient {(eg / gb).max():.3f}, power "
              f"{ep.max() / tol:.3f}; G against its own J {(ec / (1e-12 * np.abs(terms).sum(axis=2))).max():.3f}")
        assert (ej <= jb).all(), (name, mode, tag, (ej / jb).max())
        assert (eg <= gb).all(), (name, mode, tag, (eg / gb).max())
        assert ep.max() <= tol, (name, mode, tag, ep.max())
        assert (ec <= 1e-12 * np.abs(terms).sum(axis=2)).all(), (name, mode, tag)
    assert np.array_equal(one["jacobian"], rnd["jacobian"]) and np.array_equal(one["power"], rnd["power"])  # c plays no part in them
    assert (one["gradient"] != rnd["gradient"]).any()
    # what is checked is larger than what is allowed: in every tile of every farm some |J| exceeds ten strict bounds
    big = np.abs(ref["jacobian"]) > 10.0 * jb
    print(f"{name} {mode}: {big.mean():.1%} of the Jacobian entries exceed ten bounds")
    i0 = 0
    for nt in wc.REACHES[name]["tiles"]:
        assert tol != parity.TOL_F64["power"] or big[:, i0:i0 + nt].any(axis=(1, 2)).all(), (name, i0)
        i0 += nt


def test_grad_two_tiles():
    """G65: tiles of 63 and 2 turbines, lane loops past 64.  Strict and default mode against the reference; strict chunks of
    2 + 1 farms and the farm list [2, 0, 0] give the bits of the whole run."""
    name = "G65"
    c = wc.case(name)
    yaw, cot, N = c["yaw"], c["cot"], c["N"]
    kw = dict(bounds=GRAD_BOUNDS, jacobian=True)
    w = _open(c)
    try:
        one = w.yaw_gradient(yaw, strict=True, **kw)
        rnd = w.yaw_gradient(yaw, cot, strict=True, **kw)
        chunks = w.yaw_gradient(yaw, cot, strict=True, max_eval_farms=2 * (2 * N + 1) + 1, **kw)
        farms = [2, 0, 0]
        sub = w.yaw_gradient(yaw[farms], cot[farms], farms=farms, strict=True, **kw)
        d_one = w.yaw_gradient(yaw, **kw)
        d_rnd = w.yaw_gradient(yaw, cot, **kw)
    finally:
        w.close()
    _check_grad(name, one, rnd, parity.TOL_F64["power"], "strict")
    _check_grad(name, d_one, d_rnd, parity.TOL["power"], "default mode")
    for k in GRAD_KEYS:
        assert _bits(chunks[k], rnd[k]), k
        assert _bits(sub[k], rnd[k][farms]), k


def test_grad_largest_farm():
    """G256: 18 tiles of 15 turbines, the last of 1; LDS rows of 257 floats."""
    name = "G256"
    c = wc.case(name)
    w = _open(c)
    try:
        one = w.yaw_gradient(c["yaw"], bounds=GRAD_BOUNDS, strict=True, jacobian=True)
        rnd = w.yaw_gradient(c["yaw"], c["cot"], bounds=GRAD_BOUNDS, strict=True, jacobian=True)
    finally:
        w.close()
    _check_grad(name, one, rnd, parity.TOL_F64["power"], "strict")


# ---- credit -----------------------------------------------------------------------------------------------------------------
CREDIT_WANT = ("reward", "farm_power", "difference")


def _check_credit(name, got, tol, mode):
    """The inequalities of tests/test_credit_gpu.py: _check and test_exact_zeros_and_copied_rows, on every row."""
    ref = wc.reference(name)
    B, N, K = ref["same"].shape
    R = 1 + N * K
    assert got["reward"].shape == (B, R) and got["reward"].dtype == np.float64
    assert got["farm_power"].shape == (B, R) and got["difference"].shape == (B, N, K) and got["difference"].dtype == np.float64
    b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, tol).reshape(B, R)
    pb = credit_ref.power_bound(ref["out"], tol).reshape(B, R)
    same = ref["same"]
    srow = same.reshape(B, N * K)
    db = (b[:, :1] + b[:, 1:]).reshape(B, N, K)
    b[:, 1:] = np.where(srow, b[:, :1], b[:, 1:])  # (a row that copies row 0 has row 0's bounds)
    pb[:, 1:] = np.where(srow, pb[:, :1], pb[:, 1:])
    er, ep, ed = (np.abs(got[k] - ref[k]) for k in CREDIT_WANT)
    live = ~same
    print(f"{name} {mode}: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}, difference "
          f"{(ed[live] / db[live]).max():.3f}; median |D| {np.median(np.abs(ref['difference'][live])):.2e}, median bound {np.median(db[live]):.2e}")
    assert (er <= b).all(), (name, mode, (er / b).max())
    assert (ep <= pb).all(), (name, mode, (ep / pb).max())
    assert (ed <= db).all(), (name, mode, (ed / db).max())
    # the copies: exactly 0.0, the reward and the farm power row 0's bits; everywhere else reward[0] - reward[row], bit for bit
    assert same.sum() == len(wc.CASES[name]["copies"])
    assert (got["difference"][same] == 0.0).all() and not np.signbit(got["difference"][same]).any()
    for k in ("reward", "farm_power"):
        assert _bits(got[k][:, 1:][srow], np.broadcast_to(got[k][:, :1], srow.shape)[srow]), k
    d = (got["reward"][:, :1] - got["reward"][:, 1:]).reshape(B, N, K)
    assert _bits(got["difference"][live], d[live])
    clear = live & (np.abs(ref["difference"]) > db)
    assert clear.any() and (got["difference"][clear] != 0.0).all()  # (a reference |D| beyond its bound cannot come out as 0)


def test_credit_eight_tiles():
    """C65: 131 rows in 8 tiles of 18, the last of 5; a copied alternative per farm in the last tile.  Strict and default mode
    against the reference; strict chunks of 2 + 1 farms and the farm list [2, 0, 0] give the bits of the whole run."""
    name = "C65"
    c = wc.case(name)
    yaw, alt = c["yaw"], c["alt"]
    R = 1 + c["N"] * c["K"]
    w = _open(c)
    try:
        w.env_config(load_coef=LOAD_COEF)
        whole = w.counterfactual_rewards(yaw, alt, strict=True, want=CREDIT_WANT)
        chunks = w.counterfactual_rewards(yaw, alt, strict=True, max_eval_farms=2 * R + 1, want=CREDIT_WANT)
        farms = [2, 0, 0]
        sub = w.counterfactual_rewards(yaw[farms], alt[farms], farms=farms, strict=True, want=CREDIT_WANT)
        default = w.counterfactual_rewards(yaw, alt, want=CREDIT_WANT)
    finally:
        w.close()
    _check_credit(name, whole, parity.TOL_F64, "strict")
    _check_credit(name, default, parity.TOL, "default mode")
    for k in CREDIT_WANT:
        assert _bits(chunks[k], whole[k]), k
        assert _bits(sub[k], whole[k][farms]), k


def test_credit_largest_farm():
    """C256: 257 rows in 65 tiles of 4, the last of 1; the copied alternative in tile 32."""
    name = "C256"
    c = wc.case(name)
    w = _open(c)
    try:
        w.env_config(load_coef=LOAD_COEF)
        got = w.counterfactual_rewards(c["yaw"], c["alt"], strict=True, want=CREDIT_WANT)
    finally:
        w.close()
    _check_credit(name, got, parity.TOL_F64, "strict")


# ---- lookahead --------------------------------------------------------------------------------------------------------------
LA_WANT = ("returns", "rewards", "farm_power", "final_yaw", "best")


def _check_lookahead(name, got, tol, mode):
    """The checks of tests/test_lookahead_gpu.py: _check, test_final_yaw_has_the_bits_of_the_reference and test_best."""
    c, ref = wc.case(name), wc.reference(name)
    B, K, H, N = c["actions"].shape
    strict = tol is parity.TOL_F64
    assert got["returns"].shape == (B, K) and got["returns"].dtype == np.float64
    assert got["rewards"].shape == (B, K, H) and got["rewards"].dtype == np.float64
    assert got["farm_power"].shape == (B, K, H) and got["farm_power"].dtype == np.float64
    assert got["final_yaw"].shape == (B, K, N) and got["final_yaw"].dtype == np.float32
    assert got["best"].shape == (B,) and got["best"].dtype == np.int32
    b, pb, rb = wc.lookahead_bounds(ref, tol)
    er, ep, et = (np.abs(got[k] - ref[k]) for k in ("rewards", "farm_power", "returns"))
    spread = np.median(ref["returns"].max(axis=1) - ref["returns"].min(axis=1))
    print(f"{name} {mode}: largest error / bound: reward {(er / b).max():.3f}, farm power {(ep / pb).max():.3f}, return "
          f"{(et / rb).max():.3f}; median spread of the returns {spread:.2e}, median return bound {np.median(rb):.2e}")
    if strict:
        assert spread > 50.0 * np.median(rb)  # (what is checked is far larger than what is allowed)
    assert (er <= b).all(), (name, mode, (er / b).max())
    assert (ep <= pb).all(), (name, mode, (ep / pb).max())
    assert (et <= rb).all(), (name, mode, (et / rb).max())
    # the return is the discounted sum of the device's OWN rewards, bit for bit
    assert _bits(got["returns"], lookahead_ref.discounted(got["rewards"], GAMMA))
    assert _bits(got["final_yaw"], ref["final_yaw"])
    assert (ref["final_yaw"] != c["state"]["yaw"][:, None, :])[:, 1:].any() and _bits(got["final_yaw"][:, 0], c["state"]["yaw"])
    rows = np.arange(B)
    best, top = got["best"], ref["best"]
    assert np.array_equal(best, np.argmax(got["returns"], axis=1))
    assert (ref["returns"][rows, best] >= ref["returns"][rows, top] - (rb[rows, best] + rb[rows, top])).all()
    if strict:  # (tests/test_ext_wide.py: the top two reference returns are further apart than the sum of their bounds)
        assert np.array_equal(best, top), (name, best, top)


def _lookahead(w, c, actions=None, **kw):
    return w.lookahead_returns(c["actions"] if actions is None else actions, gamma=GAMMA, wind=c["wind"], want=LA_WANT, **kw)


def test_lookahead_two_tiles():
    """L65: 35 rows in tiles of 18 + 17, a wind per step, 455 trajectories on 256 threads.  Strict and default mode against
    the reference; strict chunks of 2 + 1 farms give the bits of the whole run."""
    name = "L65"
    c = wc.case(name)
    w = _open(c, env=True)
    try:
        whole = _lookahead(w, c, strict=True)
        chunks = _lookahead(w, c, strict=True, max_eval_farms=2 * c["K"] * c["H"] + 1)
        default = _lookahead(w, c)
    finally:
        w.close()
    _check_lookahead(name, whole, parity.TOL_F64, "strict")
    _check_lookahead(name, default, parity.TOL, "default mode")
    for k in LA_WANT:
        assert _bits(chunks[k], whole[k]), k


@pytest.mark.parametrize("name", ["L256", "LE"])
def test_lookahead_strict(name):
    """L256: 9 rows in tiles of 4, 4, 1.  LE: K = 1537 — the even reward stride Hs = H, 13 tiles of which the last holds 2
    rows, seven trips of the return loop."""
    c = wc.case(name)
    w = _open(c, env=True)
    try:
        got = _lookahead(w, c, strict=True)
    finally:
        w.close()
    _check_lookahead(name, got, parity.TOL_F64, "strict")


def test_lookahead_more_sequences_than_threads():
    """LK: K = 300 on 256 threads.  Against the reference; then ties: the reference's best sequence k* of every farm copied to
    (k* + 256) % 300 — below 44 the same thread's second sequence, else another thread's — and to 299: the returns of the
    copies have the bits of k*'s, and `best` is the lowest of the equal indices."""
    name = "LK"
    c, ref = wc.case(name), wc.reference(name)
    K = c["K"]
    tied = c["actions"].copy()
    want = []
    for b, k in enumerate(ref["best"]):
        same = sorted({int(k), (int(k) + 256) % K, K - 1})
        assert len(same) >= 2
        for j in same:
            tied[b, j] = c["actions"][b, k]
        want.append(same)
    w = _open(c, env=True)
    try:
        got = _lookahead(w, c, strict=True)
        ties = _lookahead(w, c, actions=tied, strict=True)
    finally:
        w.close()
    _check_lookahead(name, got, parity.TOL_F64, "strict")
    for b, same in enumerate(want):
        print(f"LK farm {b}: equal sequences {same}, best {ties['best'][b]}")
        assert _bits(ties["returns"][b, same], np.repeat(got["returns"][b, ref["best"][b]], len(same)))
        assert ties["best"][b] == same[0], (b, same, ties["best"][b])
        untouched = np.setdiff1d(np.arange(K), same)
        assert _bits(ties["returns"][b, untouched], got["returns"][b, untouched])


# ---- plan -------------------------------------------------------------------------------------------------------------------
PLAN_WANT = ("plan", "plan_return", "hold_return", "first_action", "final_yaw", "mean")
PLAN_BITS = ("plan", "mean", "first_action", "final_yaw")


def _plan(w, c, **kw):
    return w.plan_actions(c["H"], candidates=c["K"], elites=c["E"], sigma=c["sigma"], seed=c["seed"], gamma=GAMMA, want=PLAN_WANT, **kw)


def _check_plan(name, got):
    """tests/test_plan_gpu.py: test_strict_against_the_reference, with every farm safe."""
    c, ref = wc.case(name), wc.reference(name)
    B, H, N = c["farms"], c["H"], c["N"]
    shapes = {"plan": (B, H, N), "mean": (B, H, N), "first_action": (B, N), "final_yaw": (B, N), "plan_return": (B,), "hold_return": (B,)}
    for k, s in shapes.items():
        assert got[k].shape == s and got[k].dtype == (np.float64 if k.endswith("return") else np.float32), k
    eh, ep = np.abs(got["hold_return"] - ref["hold_return"]), np.abs(got["plan_return"] - ref["plan_return"])
    print(f"case {name}: smallest margin {ref['margin'].min():.2e}; largest error / bound: hold_return {(eh / ref['hold_bound']).max():.3f}, "
          f"plan_return {(ep / ref['plan_bound']).max():.3f}")
    assert ref["safe"].all()
    for k in PLAN_BITS:
        assert _bits(got[k], ref[k]), k
    assert (eh <= ref["hold_bound"]).all() and (ep <= ref["plan_bound"]).all()
    assert np.array_equal(got["first_action"], got["plan"][:, 0])
    assert (got["plan"] != 0.0).any() and (got["plan_return"] > got["hold_return"]).all()  # (the search moved)


def test_plan_256_threads():
    """PC: N = 65 — the 256-thread launch of the advance kernel, 24 rows in tiles of 18 + 6.  Strict against the reference;
    a second strict run and a farm per chunk give the same bits; the default mode holds the conditions of
    tests/test_plan_gpu.py: test_default_mode."""
    name = "PC"
    c = wc.case(name)
    w = _open(c, env=True)
    try:
        got = _plan(w, c, strict=True)
        again = _plan(w, c, strict=True)
        single = _plan(w, c, strict=True, max_eval_farms=c["K"] * c["H"])
        default = _plan(w, c)
        la = w.lookahead_returns(default["plan"][:, None].copy(), gamma=GAMMA, want=("returns", "final_yaw"))
    finally:
        w.close()
    _check_plan(name, got)
    for k in PLAN_WANT:
        assert _bits(again[k], got[k]), k
        assert _bits(single[k], got[k]), k
    assert (default["plan_return"] >= default["hold_return"]).all()
    ref = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], default["plan"][:, None], dict(PARAMS, discrete=False), GAMMA,
                                  LOAD_COEF)
    b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, parity.TOL).reshape(c["farms"], c["H"])
    rb = (lookahead_ref.discounts(GAMMA, c["H"]) * b).sum(axis=1)
    err = np.abs(default["plan_return"] - la["returns"][:, 0])
    eo = np.abs(default["plan_return"] - ref["returns"][:, 0])
    print(f"case {name}, default mode: largest |plan_return - lookahead return| / (2 bounds) {(err / (2.0 * rb)).max():.3f}, "
          f"|plan_return - oracle return| / bound {(eo / rb).max():.3f}")
    assert (err <= 2.0 * rb).all()
    assert (eo <= rb).all()  # (and the oracle's return of that plan)
    assert _bits(default["final_yaw"], la["final_yaw"][:, 0])
    assert _bits(default["final_yaw"], ref["final_yaw"][:, 0])


@pytest.mark.parametrize("name", ["PD", "PE"])
def test_plan_more_candidates_than_threads(name):
    """PD: K = 300 on 256 threads — the ranks by counting, the elite flags, the argmax over strided k, the mean of 30 elites.
    PE: K = 1537 — the even reward stride in the plan launcher, 100 elites."""
    c = wc.case(name)
    w = _open(c, env=True)
    try:
        got = _plan(w, c, strict=True)
    finally:
        w.close()
    _check_plan(name, got)


# ---- yawopt and robust ------------------------------------------------------------------------------------------------------
def test_yawopt_past_a_wave():
    """Y65: the visit order on two waves, the `t += 64` phases of the advance kernel.  Strict: the reference's decisions on
    every kept farm.  Default mode: the farm power never decreases, and the reported power is the oracle's at the returned yaw
    within the project's 1e-4."""
    c, ref = wc.case("Y65"), wc.reference("Y65")
    x, y, ws, wd = c["x"], c["y"], c["ws"], c["wd"]
    w = _open(c)
    try:
        strict = w.optimize_yaw(strict=True, passes=PASSES)
        default = w.optimize_yaw(passes=PASSES)
    finally:
        w.close()
    assert strict["yaw"].shape == (c["farms"], c["N"]) and strict["power"].shape == (c["farms"],)
    safe = _check_search(x, y, ws, wd, strict, ref, "Y65")
    assert safe.all() and (strict["yaw"] != 0.0).any()
    assert (default["power"] >= default["power_initial"]).all()
    e = np.abs(default["power"] / yawopt_ref.farm_power(x, y, ws, wd, default["yaw"]) - 1.0)
    print(f"Y65 default mode: power vs oracle at its yaw {e.max():.2e} (tol 1e-4)")
    assert e.max() <= 1e-4


def test_robust_past_a_wave():
    """R65: uncertain_power (strict) against robust_ref.expected_power at a random yaw within +-20 deg, under POW_TOL as
    tests/test_robust_gpu.py: test_uncertain_power; the robust search (strict) against robust_ref.optimize on every kept farm."""
    c, ref = wc.case("R65"), wc.reference("R65")
    x, y, ws, wd = c["x"], c["y"], c["ws"], c["wd"]
    B, N = c["farms"], c["N"]
    delta, wgt = wc.members()
    unc = dict(delta=wc.MEMBERS[0], weight=wc.MEMBERS[1], frame="fixed")
    yaw = np.random.default_rng(7).uniform(-20.0, 20.0, (B, N)).astype(np.float32)
    E, pm, Et = robust_ref.expected_power(x, y, ws, wd, yaw, delta, wgt, "fixed")
    w = _open(c)
    try:
        got = w.uncertain_power(yaw, wd_uncertainty=unc, strict=True)
        search = w.optimize_yaw(strict=True, passes=PASSES, wd_uncertainty=unc)
    finally:
        w.close()
    assert got["expected_power"].shape == (B,) and got["turbine_expected_power"].shape == (B, N) and got["member_power"].shape == (B, 3)
    assert np.array_equal(got["delta"], delta) and np.array_equal(got["weight"], wgt)
    for k, r in {"expected_power": E, "turbine_expected_power": Et, "member_power": pm}.items():
        e = np.abs(got[k] / r - 1.0).max()
        print(f"R65 {k}: strict {e:.2e} (tol {POW_TOL:g})")
        assert e <= POW_TOL, k
    safe = _check_robust_search(x, y, ws, wd, search, ref, "fixed", "R65", (delta, wgt))
    assert safe.all() and (search["yaw"] != 0.0).any()
