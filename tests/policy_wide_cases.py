"""TEST INFRASTRUCTURE — the cases tests/test_policy_wide.py (CPU: the cases and the references alone) and
tests/test_policy_wide_gpu.py (the device against the references) share: the glue kernels of policy_returns (csrc/policy) and
policy_scenarios (csrc/polscen) past one tile, one network pass and one trip of their strided loops.  Every case of
tests/policy_ref.py and tests/polscen_ref.py gives one tile per policy (nt == T == C), one pass (b0 == 0) and one trip of every
layer loop (nout G <= 256) — tests/test_policy_wide.py asserts it —; here every case names the branch it is for, and `launch`
restates the plan's and the launchers' arithmetic, so that a case that no longer reaches its branch fails on the CPU.

The inputs come from policy_ref.build / polscen_ref.build — the generators of the old cases: env state with a start yaw at
the bound, parameters scaled by 1 / sqrt(in), the normalisation, the seam-crossing wind per step.  Layouts and winds:
yawopt_ref.gpu_input for Ablaincourt and HornsRev1 (32 winds); the row of three under yawopt_ref.ROW3_WIND, and for a farm
past the fourth a wind drawn as yawopt_ref.gpu_case draws (default_rng(GPU_CASE_SEED), 6-12 m/s, any direction); N = 256:
ext_wide_cases.wide_layout(256) under winds drawn as ext_wide_cases draws them for the lookahead (default_rng(3): 6-12 m/s,
255-285 deg: along the grid's rows).

Policy cases (policy_returns, M = 1):
  PT     row3, central (5,) relu / tanh, 19 farms, K 3, H 3, a wind per step: T = 16 by the cap, advance tiles [16, 3]
  PS     Ablaincourt, shared + free wind (65, 5) softsign, 18 farms, K 2, H 3, a wind per step: tiles [16, 2]; MB = 48: passes
         [48, 48, 16] and [14]; the first layer makes 4 and 2 trips; cnt = 14 leaves groups with i2, i3 invalid inside a strided loop
  PW     Ablaincourt, shared + free wind (256, 65, 5) tanh, 18 farms, K 1, H 2: four layers (the last activation lands in
         bufB), width 256; MB = 12: passes [12 x 9, 4] and [12, 2]; the first layer makes 3 trips
  PH     HornsRev1, central (65, 5) relu / softsign, 11 farms, K 2, H 2: T = 9 by the LDS budget, tiles [9, 2]
  PHS    HornsRev1, shared + free wind (65, 5) relu / tanh, 5 farms, K 1, H 2: T = 5, MB = 39: eleven passes, the last of 10
  P256C  N 256, central (5,) relu, linear output, 3 farms, K 1, H 2: T = 2 by the budget, tiles [2, 1]; the observation loop
         makes 7 trips
  P256S  N 256, shared (5,) softsign, 4 farms, K 1, H 2: T = 3, tiles [3, 1]; MB = 284: passes [284, 284, 200] and [256];
         lds_bytes = 57 344, the budget to the byte
  PR     row3, central (5,) relu, DISCRETE, 70 farms, K 3, H 2: reduce tiles [64, 6] on 256 threads; advance tiles 4 x 16 + 6;
         the discrete central argmax (3 tt), which no case of policy_ref has
  PK     HornsRev1, central (65,) relu / tanh, 1 farm, K 64, H 2: K at its limit; the transpose kernel's grid stride: K P =
         1 350 400 floats on 1024 blocks of 256 threads, 6 trips
  PL     row3, shared (5,) tanh, 2 farms, K 1, H 256: H at its limit
Ensemble cases (policy_scenarios; process polscen_ref.PROCESS unless said otherwise):
  ES     row3, shared + free wind (65, 5) softsign, 19 farms, K 2, M 3, H 3, tail 2: 57 rows per policy in advance tiles
         [16, 16, 16, 9]; tiles 1 and 2 straddle a member boundary
  ER     ES under max_eval_farms = 17 K M: chunks of 17 and 2 farms; the second has C = 17 with 15 padding slots, inside tiles
         [16, 16, 16, 3] that straddle
  EM     row3, central (5,) relu / tanh, 3 farms, K 5, M 64, H 2, tail 7: M at its limit; 192 rows per policy: returns tiles
         [64, 64, 64], each across members; stats: 4 policies per pass, passes [4, 1], the load loop 2 trips (K M = 320);
         paths: 3 blocks
  ET     EM under polscen_ref.STILL, tails 1, 7 and 64: every member return of a policy is equal; the rank tie-break by
         member index runs over two stats passes

The seeds: a case's generator seed is the first of s, s + 1, .. (s = 21 .. 32 in the order of the tables below) for which the
properties tests/test_policy_wide.py asserts on the reference hold — the policies move the turbines, the K policies differ,
every discrete turbine's two best outputs are more than 1e-9 apart, the rows of a later tile / pass act unlike their aliases
in the first, the members' paths differ, EM's five scores are pairwise distinct.  The outcome is SEED_SEARCH: ten of twelve
keep their first seed; PHS takes 26 (at 25 ten entries of later passes repeat their alias: a relu layer that is dead for
them) and PR 42 (at 28 .. 41 between one and eighteen of the 54 rows past tile 0 choose, on all nine (policy, turbine) pairs,
what their alias row chooses: three values per turbine).  tests/test_policy_wide.py shows that the seeds passed over fail."""
import functools

import numpy as np

import ext_wide_cases
import policy_ref
import polscen_ref
import yawopt_ref

WIDE_WIND_SEED = 3  # ext_wide_cases' lookahead generator

# name: (layout, farms, kind, hidden widths, activation, final, use_freewind, discrete, K, H, per-step wind, seed): policy_ref.CASES' format
POLICY = {
    "PT": ("row3", 19, "central", (5,), "relu", "tanh", False, False, 3, 3, True, 21),
    "PS": ("Ablaincourt_", 18, "shared", (65, 5), "softsign", "softsign", True, False, 2, 3, True, 22),
    "PW": ("Ablaincourt_", 18, "shared", (256, 65, 5), "tanh", "tanh", True, False, 1, 2, False, 23),
    "PH": ("HornsRev1_", 11, "central", (65, 5), "relu", "softsign", False, False, 2, 2, False, 24),
    "PHS": ("HornsRev1_", 5, "shared", (65, 5), "relu", "tanh", True, False, 1, 2, False, 26),
    "P256C": ("wide256", 3, "central", (5,), "relu", None, False, False, 1, 2, False, 26),
    "P256S": ("wide256", 4, "shared", (5,), "softsign", "softsign", False, False, 1, 2, False, 27),
    "PR": ("row3", 70, "central", (5,), "relu", None, False, True, 3, 2, False, 42),
    "PK": ("HornsRev1_", 1, "central", (65,), "relu", "tanh", False, False, 64, 2, False, 29),
    "PL": ("row3", 2, "shared", (5,), "tanh", "tanh", False, False, 1, 256, False, 30),
}
# the policy cases under the ensembles (their wind per step is not used: the members' paths are the wind)
BASES = {
    "ES": ("row3", 19, "shared", (65, 5), "softsign", "softsign", True, False, 2, 3, False, 31),
    "EM": ("row3", 3, "central", (5,), "relu", "tanh", False, False, 5, 2, False, 32),
}
# name: dict(base, M, tails — the first is the case's own —, process, max_eval_farms or None)
ENSEMBLE = {
    "ES": dict(base="ES", M=3, tails=(2,), process=polscen_ref.PROCESS, max_eval_farms=None),
    "ER": dict(base="ES", M=3, tails=(2,), process=polscen_ref.PROCESS, max_eval_farms=17 * 2 * 3),
    "EM": dict(base="EM", M=64, tails=(7,), process=polscen_ref.PROCESS, max_eval_farms=None),
    "ET": dict(base="EM", M=64, tails=(1, 7, 64), process=polscen_ref.STILL, max_eval_farms=None),
}
CASES = dict(POLICY, **ENSEMBLE)
POLICY_NAMES, ENSEMBLE_NAMES = tuple(POLICY), tuple(ENSEMBLE)
# the first seed tried for every generator, and the one kept: the first for which tests/test_policy_wide.py's properties hold
SEED_SEARCH = {"PT": (21, 21), "PS": (22, 22), "PW": (23, 23), "PH": (24, 24), "PHS": (25, 26), "P256C": (26, 26), "P256S": (27, 27),
               "PR": (28, 42), "PK": (29, 29), "PL": (30, 30), "ES": (31, 31), "EM": (32, 32)}

_NONE = dict(reduce_tiles=None, reduce_threads=None, returns_tiles=None, stats_passes=None, stats_load_trips=None, paths_blocks=None)
# what every case is for, in the terms of `launch`: asserted by tests/test_policy_wide.py
REACHES = {
    "PT": dict(chunks=[19], T=16, MB=16, advance_tiles=[16, 3], straddles=0, passes={16: [16], 3: [3]},
               layer_trips={16: [1, 1], 3: [1, 1]}, obs_trips=1, lds_bytes=5072, reduce_tiles=[19], reduce_threads=64, transpose_trips=1),
    "PS": dict(chunks=[18], T=16, MB=48, advance_tiles=[16, 2], straddles=0, passes={16: [48, 48, 16], 2: [14]},
               layer_trips={48: [4, 1, 1], 16: [2, 1, 1], 14: [2, 1, 1]}, obs_trips=2, lds_bytes=56528, reduce_tiles=[18],
               reduce_threads=256, transpose_trips=1),
    "PW": dict(chunks=[18], T=16, MB=12, advance_tiles=[16, 2], straddles=0, passes={16: [12] * 9 + [4], 2: [12, 2]},
               layer_trips={12: [3, 1, 1, 1], 4: [1, 1, 1, 1], 2: [1, 1, 1, 1]}, obs_trips=2, lds_bytes=54512, reduce_tiles=[18],
               reduce_threads=256, transpose_trips=1),
    "PH": dict(chunks=[11], T=9, MB=9, advance_tiles=[9, 2], straddles=0, passes={9: [9], 2: [2]},
               layer_trips={9: [1, 1, 1], 2: [1, 1, 1]}, obs_trips=9, lds_bytes=55528, reduce_tiles=[11], reduce_threads=256,
               transpose_trips=1),
    "PHS": dict(chunks=[5], T=5, MB=39, advance_tiles=[5], straddles=0, passes={5: [39] * 10 + [10]},
                layer_trips={39: [3, 1, 1], 10: [1, 1, 1]}, obs_trips=5, lds_bytes=56776, reduce_tiles=[5], reduce_threads=256,
                transpose_trips=1),
    "P256C": dict(chunks=[3], T=2, MB=2, advance_tiles=[2, 1], straddles=0, passes={2: [2], 1: [1]},
                  layer_trips={2: [1, 1], 1: [1, 1]}, obs_trips=7, lds_bytes=39104, reduce_tiles=[3], reduce_threads=256, transpose_trips=1),
    "P256S": dict(chunks=[4], T=3, MB=284, advance_tiles=[3, 1], straddles=0, passes={3: [284, 284, 200], 1: [256]},
                  layer_trips={284: [2, 1], 200: [1, 1], 256: [2, 1]}, obs_trips=10, lds_bytes=57344, reduce_tiles=[4],
                  reduce_threads=256, transpose_trips=1),
    "PR": dict(chunks=[70], T=16, MB=16, advance_tiles=[16, 16, 16, 16, 6], straddles=0, passes={16: [16], 6: [6]},
               layer_trips={16: [1, 1], 6: [1, 1]}, obs_trips=1, lds_bytes=6096, reduce_tiles=[64, 6], reduce_threads=256, transpose_trips=1),
    "PK": dict(chunks=[1], T=1, MB=1, advance_tiles=[1], straddles=0, passes={1: [1]}, layer_trips={1: [1, 1]}, obs_trips=1,
               lds_bytes=6184, reduce_tiles=[1], reduce_threads=256, transpose_trips=6),
    "PL": dict(chunks=[2], T=2, MB=6, advance_tiles=[2], straddles=0, passes={2: [6]}, layer_trips={6: [1, 1]}, obs_trips=1,
               lds_bytes=936, reduce_tiles=[2], reduce_threads=64, transpose_trips=1),
    "ES": dict(chunks=[19], T=16, MB=48, advance_tiles=[16, 16, 16, 9], straddles=2, passes={16: [48], 9: [27]},
               layer_trips={48: [4, 1, 1], 27: [2, 1, 1]}, obs_trips=1, lds_bytes=54224, transpose_trips=1, returns_tiles=[57],
               stats_passes=[2], stats_load_trips=1, paths_blocks=1),
    "ER": dict(chunks=[17, 2], T=16, MB=48, advance_tiles=[16, 16, 16, 3], straddles=2, passes={16: [48], 3: [9]},
               layer_trips={48: [4, 1, 1], 9: [1, 1, 1]}, obs_trips=1, lds_bytes=54224, transpose_trips=1, returns_tiles=[51],
               stats_passes=[2], stats_load_trips=1, paths_blocks=1),
    "EM": dict(chunks=[3], T=16, MB=16, advance_tiles=[16] * 12, straddles=12, passes={16: [16]}, layer_trips={16: [1, 1]}, obs_trips=1,
               lds_bytes=5072, transpose_trips=1, returns_tiles=[64, 64, 64], stats_passes=[4, 1], stats_load_trips=2, paths_blocks=3),
}
REACHES["ET"] = REACHES["EM"]
for _n in REACHES:
    REACHES[_n] = dict(_NONE, **REACHES[_n])


# ---- the plan's and the launchers' arithmetic, restated: each function names the C line it mirrors --------------------------
def _split(total, T):
    """The sizes of the tiles a loop `for (r0 = 0; r0 < total; r0 += T)` walks."""
    return [min(T, total - r0) for r0 in range(0, total, T)]


def _trips(n, stride):
    """The trips of `for (i = tid; i < n; i += stride)` thread 0 makes."""
    return -(-n // stride)


def policy_plan(kind, widths, N, C):
    """csrc/policy/wf_policy_kernels.hip: wf_policy_plan — `budget = 56 * 1024`; the odd strides `xs = width[0] | 1`,
    `as = wmax | 1`, `ds = (3 * N + 2) | 1`, `sp = N | 1`, `sl = (4 * N) | 1`;
    `per_inst = sizeof(double) * (xs + 2 * as)`, `per_row = sizeof(float) * (ds + N + sp + sl) + sizeof(int) + 3 * sizeof(double)`;
    shared: `T = (budget / 2) / per_row`, 1 .. 16, at most C, `MB = (budget - T * per_row) / per_inst`, 1 .. T N;
    central: `T = budget / (per_row + per_inst)`, 1 .. 16, at most C, `MB = T`;
    `lds_bytes = MB * per_inst + T * per_row + 16`.  C is the rows of one policy in a chunk (M C under an ensemble)."""
    budget = 56 * 1024
    wmax = max([1] + list(widths[1:]))
    p = dict(xs=widths[0] | 1, ds=(3 * N + 2) | 1, sp=N | 1, sl=(4 * N) | 1, threads=256)
    p["as"] = wmax | 1
    per_inst = 8 * (p["xs"] + 2 * p["as"])
    per_row = 4 * (p["ds"] + N + p["sp"] + p["sl"]) + 4 + 3 * 8
    if kind == "shared":
        T = (budget // 2) // per_row
        T = 1 if T < 1 else min(T, 16)
        T = min(T, C)
        MB = (budget - T * per_row) // per_inst
        MB = max(MB, 1)
        MB = min(MB, T * N)
    else:
        T = budget // (per_row + per_inst)
        T = 1 if T < 1 else min(T, 16)
        T = min(T, C)
        MB = T
    p.update(T=T, MB=MB, per_inst=per_inst, per_row=per_row, lds_bytes=MB * per_inst + T * per_row + 16)
    return p


def plan_regions(p, N):
    """wf_policy_advance_kernel's LDS, in its order, as (name, first byte, bytes): `wrl`, `rwl`, `psl` [T] doubles; `pw`
    [T][sp] and the load tile [T][sl] floats; `x0` at `pw + ((T * (sp + sl) + 1) & ~1)` [MB][xs] doubles; `bufA`, `bufB`
    [MB][as] doubles; `obs` [T][ds] floats; `actf` [T][N] floats; `ng` [T] ints."""
    T, MB = p["T"], p["MB"]
    out, o = [], 0
    for name, n in (("wrl", 8 * T), ("rwl", 8 * T), ("psl", 8 * T), ("pw+ld", 4 * ((T * (p["sp"] + p["sl"]) + 1) & ~1)),
                    ("x0", 8 * MB * p["xs"]), ("bufA", 8 * MB * p["as"]), ("bufB", 8 * MB * p["as"]), ("obs", 4 * T * p["ds"]),
                    ("actf", 4 * T * N), ("ng", 4 * T)):
        out.append((name, o, n))
        o += n
    return out


def chunk_slots(n_farms, rows, max_eval_farms=None):
    """csrc/ext/wf_ext.hip: run_rows — `C = k.max_eval / R` (R = K, or K M under an ensemble; max_eval_farms defaults to
    65536), `if (C > n) C = n`, `for (first = 0; first < n; first += C)`.  Returns (C, the farms of every chunk)."""
    C = min((65536 if max_eval_farms is None else max_eval_farms) // rows, n_farms)
    return C, _split(n_farms, C)


def advance_launch(p, kind, widths, N, M, C):
    """wfk_launch_policy_advance: `tiles = (M * C + T - 1) / T`; wf_policy_advance_kernel: `s0 = blockIdx.x * T`,
    `nt = min(T, R - s0)`, `m = j / C`; phase 2 `for (q = tid; q < nt * D0; q += nth)`; phase 3
    `n_inst = shared ? nt * N : nt`, `for (b0 = 0; b0 < n_inst; b0 += MB)`, `G = (cnt + 3) >> 2`,
    `for (q = tid; q < nout * G; q += nth)`."""
    T, MB = p["T"], p["MB"]
    tiles = _split(M * C, T)
    starts = range(0, M * C, T)
    straddles = sum(1 for s0, nt in zip(starts, tiles) if s0 // C != (s0 + nt - 1) // C)
    passes = {nt: _split(nt * N if kind == "shared" else nt, MB) for nt in dict.fromkeys(tiles)}
    layer_trips = {cnt: [_trips(nout * ((cnt + 3) >> 2), 256) for nout in widths[1:]] for cnts in passes.values() for cnt in cnts}
    return dict(advance_tiles=tiles, straddles=straddles, passes=passes, layer_trips=layer_trips, obs_trips=_trips(T * (3 * N + 2), 256))


def reduce_launch(N, K, C):
    """wfk_launch_policy_reduce: `per = sizeof(double) * (K + 3) + sizeof(float) * (sp + sll)`, `T = 48 * 1024 / per`, 1 .. 64,
    at most C; `tiles = (C + T - 1) / T`; threads `T * N <= 64 ? 64 : 256`."""
    per = 8 * (K + 3) + 4 * ((N | 1) + ((4 * N) | 1))
    T = 48 * 1024 // per
    T = 1 if T < 1 else min(T, 64)
    T = min(T, C)
    return dict(reduce_tiles=_split(C, T), reduce_threads=64 if T * N <= 64 else 256)


def transpose_trips(K, P):
    """wfk_launch_policy_transpose: `blocks = min(1024, (n + 255) / 256)` of 256 threads, n = K P; the kernel's grid stride
    `for (q = ..; q < n; q += gridDim.x * blockDim.x)`."""
    n = K * P
    blocks = min(1024, (n + 255) // 256)
    return _trips(n, blocks * 256)


def polscen_tile(N, rows):
    """csrc/polscen/wf_polscen_kernels.hip: wf_polscen_tile — `per = 3 * sizeof(double) + sizeof(float) * (sp + sl)`,
    `T = 48 * 1024 / per`, 1 .. 64, at most `rows`; wfk_launch_polscen_returns: `(rows + T - 1) / T` tiles per policy."""
    per = 3 * 8 + 4 * ((N | 1) + ((4 * N) | 1))
    T = 48 * 1024 // per
    T = 1 if T < 1 else min(T, 64)
    return _split(rows, min(T, rows))


def stats_launch(K, M):
    """wfk_launch_polscen_stats: 256 threads; wf_polscen_stats_kernel: `spp = nth / M` policies per pass,
    `for (k0 = 0; k0 < K; k0 += spp)`; the load loop `for (i = tid; i < KM; i += nth)`."""
    return dict(stats_passes=_split(K, 256 // M), stats_load_trips=_trips(K * M, 256))


def paths_blocks(C, M):
    """wfk_launch_polscen_paths: `dim3((n + 63) / 64)` blocks of 64 threads, n = C M."""
    return (C * M + 63) // 64


def param_count(widths):
    return sum((a + 1) * b for a, b in zip(widths[:-1], widths[1:]))


def launch_of(kind, widths, N, n_farms, K, M=1, max_eval_farms=None, ensemble=False):
    """What the plan and the launchers make of a run: the keys of REACHES."""
    C, chunks = chunk_slots(n_farms, K * M, max_eval_farms)
    p = policy_plan(kind, widths, N, M * C)
    out = dict(_NONE, chunks=chunks, T=p["T"], MB=p["MB"], lds_bytes=p["lds_bytes"], transpose_trips=transpose_trips(K, param_count(widths)))
    out.update(advance_launch(p, kind, widths, N, M, C))
    if ensemble:
        out.update(returns_tiles=polscen_tile(N, M * C), paths_blocks=paths_blocks(C, M), **stats_launch(K, M))
    else:
        out.update(reduce_launch(N, K, C))
    return out


def launch(name):
    """What the plan and the launchers make of the case: the keys of REACHES[name]."""
    e = ENSEMBLE.get(name)
    row = BASES[e["base"]] if e else POLICY[name]
    layout, B, kind, hidden, _, _, fw, discrete, K = row[:9]
    N = layout_of(layout)[0].size
    D = 3 * N + 2 if kind == "central" else (5 if fw else 3)
    per = 3 if discrete else 1
    widths = (D,) + tuple(hidden) + (per * N if kind == "central" else per,)
    if e:
        return launch_of(kind, widths, N, B, K, e["M"], e["max_eval_farms"], ensemble=True)
    return launch_of(kind, widths, N, B, K)


# ---- inputs and references, computed once ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout_of(layout, B=0):
    """(x, y, ws, wd) with at least B winds: module docstring."""
    if layout == "wide256":
        x, y = ext_wide_cases.wide_layout(256)
        rng = np.random.default_rng(WIDE_WIND_SEED)
        n = max(B, 1)
        return x, y, rng.uniform(6.0, 12.0, n), rng.uniform(255.0, 285.0, n)
    x, y, ws, wd = yawopt_ref.gpu_input(layout)
    if layout == "row3" and B > len(ws):
        rng = np.random.default_rng(yawopt_ref.GPU_CASE_SEED)
        more = B - len(ws)
        ws, wd = np.concatenate([ws, rng.uniform(6.0, 12.0, more)]), np.concatenate([wd, rng.uniform(0.0, 360.0, more)])
    return x, y, ws, wd


def _row(name, seed):
    row = POLICY[name] if name in POLICY else BASES[name]
    return row if seed is None else row[:-1] + (seed,)


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """A policy case (a name of POLICY or BASES): policy_ref.build's dict; `seed` replaces the row's generator seed."""
    row = _row(name, seed)
    return policy_ref.build(name, row, layout_of(row[0], row[1]))


@functools.lru_cache(maxsize=None)
def reference(name, seed=None):
    return policy_ref.reference_of(case(name, seed))


@functools.lru_cache(maxsize=None)
def ensemble(name, seed=None):
    """An ensemble case: polscen_ref.build's dict plus `tails` and `max_eval_farms`; `seed` replaces the base's generator seed."""
    e = ENSEMBLE[name]
    s = polscen_ref.build(name, case(e["base"], seed), e["M"], e["tails"][0], e["process"])
    return dict(s, tails=e["tails"], max_eval_farms=e["max_eval_farms"])


@functools.lru_cache(maxsize=None)
def ensemble_reference(name, seed=None):
    """polscen_ref.rollouts of the case (ER: ES's — the chunking is not the reference's business)."""
    return polscen_ref.reference_of(ensemble("ES" if name == "ER" else name, seed))
