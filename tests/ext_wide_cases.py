"""TEST INFRASTRUCTURE — the cases tests/test_ext_wide.py (CPU: the cases and the references alone) and
tests/test_ext_wide_gpu.py (the device against the references) share: the extensions' glue kernels (csrc/ext, grad, credit,
lookahead, plan, yawopt, robust) past one wave, one LDS tile and one pass of their strided loops.  The other extension
tests stay at N <= 16, K = 8, H <= 4, where every glue kernel runs its simplest path; here every case names the branch it is
for, and `launch` restates the launchers' arithmetic so that a case that no longer reaches its branch fails on the CPU.

Layout: `wide_layout(N)`, a jittered grid in the style of tests/test_hip_parity.py: test_max_turbines_and_ragged_batch —
column pitch 700 m, row pitch 600 m, +-50 m jitter (default_rng(2)), ceil(sqrt(N)) turbines per grid row — at N = 65 (the
smallest farm past a wave) and N = 256 (WF_MAX_TURBINES); the row of three (yawopt_ref.ROW3) where K is what matters.

Env: test_lookahead.PARAMS (+-40 deg, 5 deg a step, 0.3 deg/s, 60 s steps, budget 0.1), the state of test_lookahead._state
(open and closed gates), load_coef 0.1, gamma 0.9.  Winds: grad, credit, yawopt and robust as yawopt_ref.gpu_case draws
them (6-12 m/s, any direction); lookahead and plan as plan_cases draws them (6-12 m/s, 255-285 deg: along the grid's rows),
a wind per step as plan_cases' case B (the speed drifts by 2 % a step, the direction turns by 1.5 deg a step).

  G65   grad       N 65, 3 farms, yaw uniform in +-20, a random cotangent: 2 tiles (63 + 2 turbines), lane loops past 64
  G256  grad       N 256, 1 farm: 18 tiles of 15 turbines, the last of 1; LDS row stride 257
                   (both under the bounds +-20: the entries within a degree of a bound have divisors between 1 and 2, so that
                   a divisor read at the wrong turbine shows)
  C65   credit     N 65, K 2, 3 farms, alternatives uniform in +-20, one per farm — in the LAST tile — a copy of the base
                   entry's bits: 8 tiles of 18 rows, the last of 5; the exact 0.0 beyond tile 0
  C256  credit     N 256, K 1, 1 farm, the copy in tile 32: 65 tiles of 4 rows, the last of 1
  L65   lookahead  N 65, K 7, H 5, 3 farms, a wind per step: 35 rows in tiles of 18 + 17; K N = 455 trajectories: a second
                   trip of the layout's loop
  L256  lookahead  N 256, K 3, H 3, 1 farm: 9 rows in tiles of 4, 4, 1
  LK    lookahead  row of three, K 300, H 2, 2 farms: K > 256 threads — the strided return loop, the argmax across threads —;
                   600 rows in tiles of 256, 256, 88
  LE    lookahead  row of three, K 1537, H 2, 1 farm: K (H | 1) > 4608, the even reward stride Hs = H; 13 tiles, the last of 2
  PC    plan       N 65, K 8, H 3, E 3, sigma (5, 2.5), 2 farms: 256 threads, 24 rows in tiles of 18 + 6
  PD    plan       row of three, K 300, H 2, E 30, sigma (5, 2.5), 2 farms: K > 256 — ranks, elite flags, argmax over strided k
  PE    plan       row of three, K 1537, H 2, E 100, sigma (5, 2.5), 1 farm: Hs = H in the plan launcher
  Y65   yawopt     N 65, passes (3,), 6 farms: the visit order on two waves, the `t += 64` phases of the advance kernel
  R65   robust     N 65, passes (3,), members (-3, 0, 3) deg with weights (1, 2, 1), 4 farms: the robust advance and the row
                   sums at N > 64; uncertain_power on the same farms

What was chosen, with the inputs and the references ALONE (tests/test_ext_wide.py asserts what the choices are for):
  grad   G65's generator is default_rng(74), of 71, 72, .. the first that gives a turbine of the SECOND tile a divisor other
         than that of the turbine at the same place in the first tile (farm 0); G256 has five such turbines as drawn (72).
  plan   the state generator is default_rng(3); of the planner seeds 1..3 the one with the widest smallest margin (the method
         of series_cases.PLAN): PC seed 1 (4.4e-4; seeds 2 and 3: 4.4e-5, 3.5e-4), PD seed 2 (3.1e-4; seeds 1 and 3: 3.7e-5,
         7.8e-5), PE seed 3 (1.1e-4; seeds 1 and 2: 2.3e-5, 2.1e-6).  Every farm of the three is safe under the strict bounds.
  yawopt / robust   32 winds from default_rng(40) (yawopt_ref.gpu_case); the reference margins of all 32 farms with
         passes (3,); kept: the first 6 (yawopt) / 4 (robust) farms whose margin is >= 1e-5 (test_yawopt_gpu.MARGIN) —
         Y65 farms 0 .. 5 (smallest margin 1.2e-5), R65 farms 0 .. 3 (1.4e-5); on this layout all 32 farms
         (yawopt) and 30 of 32 (robust) are at or above it.  With the default passes (5, 4) every farm of this size has a
         near-tie among its 130 visits, so they cannot be used for a yaw comparison.
  lookahead   the generator is default_rng(3), for L256 default_rng(6) (with 3, 5, 7 and 8 the hold is the best of its three
         sequences; of 4 and 6 the wider top-two gap — the best is the last sequence, whose rows end in the last tile): in
         strict bounds the top two returns of every farm are further apart than the sum of their return bounds (300 times at
         the least), and no farm's best sequence is the hold."""
import functools
import math

import numpy as np

import credit_ref
import grad_ref
import lookahead_ref
import parity
import plan_ref
import robust_ref
import yawopt_ref
from test_lookahead import PARAMS, _state

LOAD_COEF, GAMMA = 0.1, 0.9
GRAD_BOUNDS = (-20.0, 20.0)  # the yaws are uniform in +-20: an entry within a degree of a bound has a divisor 1 <= d < 2
PASSES = (3,)
MEMBERS = (np.array([-3.0, 0.0, 3.0]), np.array([1.0, 2.0, 1.0]))
N_WINDS = 32  # the farms Y65 / R65 are picked from

CASES = {
    "G65": dict(ext="grad", N=65, farms=3, rng=74),
    "G256": dict(ext="grad", N=256, farms=1, rng=72),
    "C65": dict(ext="credit", N=65, farms=3, K=2, rng=73, copies=((0, 64, 1), (1, 63, 0), (2, 62, 1))),  # (farm, turbine, alternative)
    "C256": dict(ext="credit", N=256, farms=1, K=1, rng=74, copies=((0, 129, 0),)),
    "L65": dict(ext="lookahead", N=65, farms=3, K=7, H=5, rng=3, wind_per_step=True),
    "L256": dict(ext="lookahead", N=256, farms=1, K=3, H=3, rng=6, wind_per_step=False),
    "LK": dict(ext="lookahead", N=3, farms=2, K=300, H=2, rng=3, wind_per_step=False),
    "LE": dict(ext="lookahead", N=3, farms=1, K=1537, H=2, rng=3, wind_per_step=False),
    "PC": dict(ext="plan", N=65, farms=2, K=8, H=3, E=3, sigma=(5.0, 2.5), rng=3, seed=1),
    "PD": dict(ext="plan", N=3, farms=2, K=300, H=2, E=30, sigma=(5.0, 2.5), rng=3, seed=2),
    "PE": dict(ext="plan", N=3, farms=1, K=1537, H=2, E=100, sigma=(5.0, 2.5), rng=3, seed=3),
    "Y65": dict(ext="yawopt", N=65, keep=(0, 1, 2, 3, 4, 5)),
    "R65": dict(ext="robust", N=65, keep=(0, 1, 2, 3)),
}

# what every case is for, in the terms of `launch`: asserted by tests/test_ext_wide.py
REACHES = {
    "G65": dict(tiles=[63, 2], threads=256, layout_trips=2),
    "G256": dict(tiles=[15] * 17 + [1], threads=256, stride=257, layout_trips=4),
    "C65": dict(tiles=[18] * 7 + [5], threads=256),
    "C256": dict(tiles=[4] * 64 + [1], threads=256),
    "L65": dict(tiles=[18, 17], threads=256, layout_threads=256, layout_trips=2, Hs=5),
    "L256": dict(tiles=[4, 4, 1], threads=256, layout_threads=256, layout_trips=3, Hs=3),
    "LK": dict(tiles=[256, 256, 88], threads=256, k_trips=2, Hs=3),
    "LE": dict(tiles=[256] * 12 + [2], threads=256, k_trips=7, Hs=2),
    "PC": dict(tiles=[18, 6], threads=256, k_trips=1, Hs=3),
    "PD": dict(tiles=[256, 256, 88], threads=256, k_trips=2, Hs=3),
    "PE": dict(tiles=[256] * 12 + [2], threads=256, k_trips=7, Hs=2),
    "Y65": dict(order_threads=128, lane_trips=2, waves_per_block=4),
    "R65": dict(order_threads=128, lane_trips=2, rows_per_block=64),
}


# ---- the launchers' arithmetic, restated: each function names the C line it mirrors ---------------------------------------
def _split(total, T):
    """The sizes of the tiles a loop `for (r0 = 0; r0 < total; r0 += T)` walks."""
    return [min(T, total - r0) for r0 in range(0, total, T)]


def _trips(n, stride):
    """The trips of `for (i = tid; i < n; i += stride)` thread 0 makes."""
    return -(-n // stride)


def row_threads(R, N):
    """csrc/credit, lookahead, plan *_kernels.hip: `const int threads = R * N <= 512 ? 64 : 256;`"""
    return 64 if R * N <= 512 else 256


def reward_tile(R, N, threads, floats=6144):
    """csrc/ext/wf_ext_kernels.h: wf_reward_tile — `T = floats / (sp + sl)`, sp = N | 1, sl = (4 N) | 1, then at least 1, at
    most R, at most `threads`."""
    T = floats // ((N | 1) + ((4 * N) | 1))
    T = max(T, 1)
    return min(T, R, threads)


def reward_stride(K, H):
    """wf_lookahead_kernels.hip / wf_plan_kernels.hip: `Hs = K * (H | 1) <= 4608 ? (H | 1) : H`."""
    return (H | 1) if K * (H | 1) <= 4608 else H


def grad_tile(N):
    """wf_grad_kernels.hip: wfk_launch_grad_reduce — `T = 4096 / stride`, stride = N | 1, then `T < 1 ? 1 : (T > N ? N : T)`,
    and `threads = 2 * T * N <= 512 ? 64 : 256`.  Returns (T, stride, threads)."""
    stride = N | 1
    T = 4096 // stride
    T = 1 if T < 1 else min(T, N)
    return T, stride, (64 if 2 * T * N <= 512 else 256)


def plan_tile(K, H, N, threads):
    """wf_plan_kernels.hip: wfk_launch_plan_advance — `flags = (K + 15) & ~15`, `wf_reward_tile(R, N, threads, 6144 - flags / 4)`."""
    flags = (K + 15) & ~15
    return reward_tile(K * H, N, threads, 6144 - flags // 4)


def launch(name):
    """What the launchers make of the case: the tile sizes, the thread counts, the reward stride, the trips of the strided
    loops — the keys of REACHES[name]."""
    c = CASES[name]
    N, ext = c["N"], c["ext"]
    if ext == "grad":
        T, stride, threads = grad_tile(N)
        # wf_grad_layout_kernel: `for (int t = lane; t < N; t += 64)`
        return dict(tiles=_split(N, T), threads=threads, stride=stride, layout_trips=_trips(N, 64))
    if ext == "credit":
        R = 1 + N * c["K"]
        threads = row_threads(R, N)
        return dict(tiles=_split(R, reward_tile(R, N, threads)), threads=threads)
    if ext == "lookahead":
        K, H = c["K"], c["H"]
        threads = row_threads(K * H, N)
        lt = 64 if K * N <= 64 else 256  # wfk_launch_lookahead_layout: `threads = a->K * a->N <= 64 ? 64 : 256`
        # wf_lookahead_layout_kernel: `for (int q = tid; q < n_traj; q += nth)`; reduce: `for (int k = tid; k < K; k += nth)`
        return dict(tiles=_split(K * H, reward_tile(K * H, N, threads)), threads=threads, layout_threads=lt,
                    layout_trips=_trips(K * N, lt), k_trips=_trips(K, threads), Hs=reward_stride(K, H))
    if ext == "plan":
        K, H = c["K"], c["H"]
        threads = row_threads(K * H, N)
        # wf_plan_reduce: `for (int k = tid; k < K; k += nth)` (returns, ranks); `for (int e = tid; e < HN; e += nth)` (mean)
        return dict(tiles=_split(K * H, plan_tile(K, H, N, threads)), threads=threads, k_trips=_trips(K, threads),
                    Hs=reward_stride(K, H))
    R = PASSES[0] + 1
    # wfk_launch_yawopt_order / wfk_launch_robust_order: `dim3(((a->N + 63) / 64) * 64)`; the advance phases: `t += 64`
    out = dict(order_threads=((N + 63) // 64) * 64, lane_trips=_trips(N, 64))
    if ext == "yawopt":
        # wfk_launch_yawopt_advance: `region = (YO_HDR_BYTES + 4 * N * (R + 1) + 15) & ~15`, `wpb = 49152 / region`, 1 .. 4
        region = (32 * 8 + 32 * 4 + 4 * N * (R + 1) + 15) & ~15
        out["waves_per_block"] = max(1, min(4, 49152 // region))
    else:
        # wf_ext_kernels.h: wf_rowsum_launch — `rpb = 32768 / (4 * stride)`, stride = N | 1, 1 .. 64
        out["rows_per_block"] = max(1, min(64, 32768 // (4 * (N | 1))))
    return out


# ---- inputs and references, computed once ---------------------------------------------------------------------------------
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def wide_layout(N):
    """(x, y) of the jittered grid of N turbines."""
    rng = np.random.default_rng(2)
    per = math.ceil(math.sqrt(N))
    x = (np.arange(N) % per) * 700.0 + rng.uniform(-50, 50, N)
    y = (np.arange(N) // per) * 600.0 + rng.uniform(-50, 50, N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _layout(N):
    return yawopt_ref.ROW3 if N == 3 else wide_layout(N)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case: dict(x, y, ws, wd (B,), and the case's parameters) plus
      grad       yaw, cot (B, N) float32
      credit     yaw (B, N), alt (B, N, K) float32
      lookahead  state, actions (B, K, H, N) float32 (sequence 0 holds), wind (B, H, 2) or None
      plan       state
      yawopt / robust   ws, wd: the kept farms' winds."""
    c = CASES[name]
    N, ext = c["N"], c["ext"]
    x, y = _layout(N)
    out = dict(c, x=x, y=y)
    if ext in ("yawopt", "robust"):
        ws, wd = all_winds()
        keep = np.asarray(c["keep"])
        out.update(ws=ws[keep].copy(), wd=wd[keep].copy(), farms=len(keep))
        return _freeze(out)
    B = c["farms"]
    rng = np.random.default_rng(c["rng"])
    if ext in ("grad", "credit"):
        ws, wd = rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B)
        yaw = rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32)
        if ext == "grad":
            out.update(yaw=yaw, cot=rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32))
        else:
            alt = rng.uniform(-20.0, 20.0, (B, N, c["K"])).astype(np.float32)
            for b, i, k in c["copies"]:
                alt[b, i, k] = yaw[b, i]
            out.update(yaw=yaw, alt=alt)
    else:
        ws, wd = rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B)
        state = _state(rng, B, N)
        state["moves"] = state["moves"].astype(np.int32)
        out.update(state=state)
        if ext == "lookahead":
            K, H = c["K"], c["H"]
            actions = rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)
            actions[:, 0] = 0.0
            wind = None
            if c["wind_per_step"]:
                h = np.arange(H)
                wind = np.stack([ws[:, None] * (1.0 + 0.02 * h), wd[:, None] + 1.5 * h], axis=2)
            out.update(actions=actions, wind=wind)
    out.update(ws=ws, wd=wd)
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def all_winds():
    """The N_WINDS winds Y65 and R65 keep their farms from (yawopt_ref.gpu_case: default_rng(40), 6-12 m/s, any direction)."""
    rng = np.random.default_rng(yawopt_ref.GPU_CASE_SEED)
    ws, wd = rng.uniform(6.0, 12.0, N_WINDS), rng.uniform(0.0, 360.0, N_WINDS)
    ws.setflags(write=False)
    wd.setflags(write=False)
    return ws, wd


def members():
    """(delta, w) of R65: robust_ref.members of MEMBERS."""
    return robust_ref.members(*MEMBERS)


def search_reference(ext, ws, wd):
    """The reference search of Y65 / R65 on the layout of 65 under the winds given (the kept farms', or all N_WINDS)."""
    x, y = wide_layout(65)
    if ext == "yawopt":
        return yawopt_ref.optimize(x, y, ws, wd, passes=PASSES)
    return robust_ref.optimize(x, y, ws, wd, *members(), "fixed", passes=PASSES)


@functools.lru_cache(maxsize=None)
def reference(name, seed=None):
    """The case's reference, frozen: grad_ref.gradient at c = 1 plus "g_c", the gradient at the case's cotangent;
    credit_ref.counterfactual; lookahead_ref.lookahead; plan_ref.plan under the strict bounds (`seed` replaces the case's
    planner seed); yawopt_ref.optimize / robust_ref.optimize on the kept farms."""
    c = case(name)
    ext = c["ext"]
    if ext == "grad":
        r = grad_ref.gradient(c["x"], c["y"], c["ws"], c["wd"], c["yaw"], bounds=GRAD_BOUNDS)
        r["g_c"] = grad_ref.vjp(r["p_plus"], r["p_minus"], r["d"], c["cot"])
    elif ext == "credit":
        r = credit_ref.counterfactual(c["x"], c["y"], c["ws"], c["wd"], c["yaw"], c["alt"], LOAD_COEF)
    elif ext == "lookahead":
        r = lookahead_ref.lookahead(c["x"], c["y"], c["ws"], c["wd"], c["state"], c["actions"], dict(PARAMS, discrete=False), GAMMA,
                                    LOAD_COEF, wind=c["wind"])
    elif ext == "plan":
        r = plan_ref.plan(c["x"], c["y"], c["ws"], c["wd"], c["state"], PARAMS, c["H"], c["K"], c["E"], c["sigma"],
                          c["seed"] if seed is None else seed, GAMMA, LOAD_COEF)
    else:
        r = search_reference(ext, c["ws"], c["wd"])
    return _freeze(r)


def lookahead_bounds(ref, tol):
    """(reward bound (B, K, H), farm-power bound (B, K, H), return bound (B, K) = sum_h g_h bound_h): the bounds of
    tests/test_lookahead_gpu.py — credit_ref.bound / power_bound per row from `tol` (parity.TOL_F64 strict, parity.TOL in the
    default mode), lookahead_ref.discounts."""
    shape = ref["rewards"].shape
    b = credit_ref.bound(ref["out"], ref["wr_rows"], LOAD_COEF, tol).reshape(shape)
    pb = credit_ref.power_bound(ref["out"], tol).reshape(shape)
    return b, pb, (lookahead_ref.discounts(GAMMA, shape[2]) * b).sum(axis=2)


def top_two_gap(ref, tol=parity.TOL_F64):
    """Per farm: (the gap between the two largest reference returns, the sum of their two return bounds)."""
    rb = lookahead_bounds(ref, tol)[2]
    rows = np.arange(rb.shape[0])
    order = np.argsort(-ref["returns"], axis=1, kind="stable")
    first, second = order[:, 0], order[:, 1]
    return ref["returns"][rows, first] - ref["returns"][rows, second], rb[rows, first] + rb[rows, second]
