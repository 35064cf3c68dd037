"""CPU: the cases of tests/ext_wide_cases.py — that each one reaches the branch of the glue kernels it is for, by the
launchers' arithmetic restated in Python, and that the references alone make the GPU comparisons of
tests/test_ext_wide_gpu.py decidable: safe planner farms, search margins, separated top returns.  The references of G65,
G256, C65 and C256 (the float64 oracle on up to 513 farms of 256 turbines) are left to the GPU file."""
import numpy as np
import pytest

import ext_wide_cases as wc
from test_yawopt_gpu import MARGIN


@pytest.mark.parametrize("name", list(wc.CASES))
def test_every_case_reaches_its_branch(name):
    """What ext_wide_cases.REACHES claims for the case is what the restated launch arithmetic gives: the tile sizes (their
    number, a ragged last one), 256 threads, the trips of the strided loops, the reward stride."""
    got, want = wc.launch(name), wc.REACHES[name]
    print(name, got)
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


def test_the_claims_are_the_branches():
    """The claims themselves, in the terms of the kernels: more than one tile everywhere a tile loop runs, ragged last tiles
    where the table says so, K beyond the threads, the even reward stride, more than a wave of turbines."""
    c, r = wc.CASES, wc.REACHES
    assert set(c) == set(r)
    for name in ("G65", "G256", "C65", "C256", "L65", "L256", "LK", "LE", "PC", "PD", "PE"):
        t = r[name]["tiles"]
        assert len(t) > 1 and t[-1] < t[0] and r[name]["threads"] == 256, name  # (every one of them has a ragged last tile)
    assert (len(r["G65"]["tiles"]), len(r["G256"]["tiles"]), len(r["C65"]["tiles"]), len(r["C256"]["tiles"])) == (2, 18, 8, 65)
    assert r["G256"]["tiles"][-1] == 1 and r["C256"]["tiles"][-1] == 1 and r["L256"]["tiles"][-1] == 1
    for name in ("LK", "LE", "PD", "PE"):
        assert c[name]["K"] > r[name]["threads"] and r[name]["k_trips"] >= 2, name
    for name in ("LE", "PE"):
        assert r[name]["Hs"] == c[name]["H"] and c[name]["H"] % 2 == 0, name  # the even stride
    for name in ("L65", "L256", "LK", "PC", "PD"):
        assert r[name]["Hs"] == c[name]["H"] | 1, name
    assert c["L65"]["K"] * c["L65"]["N"] > 256 and r["L65"]["layout_trips"] == 2
    for name in ("Y65", "R65"):
        assert c[name]["N"] > 64 and r[name]["order_threads"] > 64 and r[name]["lane_trips"] == 2, name
    assert r["Y65"]["waves_per_block"] == 4  # (the packing below 4 waves needs N (R + 1) > 2976: not covered here)
    # the restated arithmetic against the sizes the kernels' own comments state
    assert wc.reward_tile(10 ** 6, 80, 256) == 15 and wc.reward_tile(10 ** 6, 256, 256) == 4  # wf_credit_kernels.hip
    assert wc.grad_tile(80)[0] == 50 and wc.grad_tile(165)[0] == 24 and wc.grad_tile(44)[0] == 44  # wf_grad_kernels.hip
    assert wc.reward_stride(1536, 2) == 3 and wc.reward_stride(1537, 2) == 2


def test_layouts():
    for N, per in ((65, 9), (256, 16)):
        x, y = wc.wide_layout(N)
        assert x.shape == y.shape == (N,) and not x.flags.writeable
        i = np.arange(N)
        assert (np.abs(x - (i % per) * 700.0) <= 50.0).all() and (np.abs(y - (i // per) * 600.0) <= 50.0).all()
        d = np.hypot(x[:, None] - x[None, :], y[:, None] - y[None, :])[~np.eye(N, dtype=bool)]
        assert d.min() >= 500.0  # (no two turbines closer than 4 D)


@pytest.mark.parametrize("name", ["G65", "G256"])
def test_a_divisor_beyond_tile_zero_differs_from_its_alias(name):
    """grad: under GRAD_BOUNDS some turbine i of a tile beyond the first has a divisor d_i that differs by more than 0.1 from
    the divisor of turbine i - i0, the one at its place in the first tile: a reduce kernel that drops the tile's offset from
    its divisor cannot pass.  Every divisor is positive."""
    import grad_ref

    c = wc.case(name)
    T = wc.REACHES[name]["tiles"][0]
    d = grad_ref.perturbed(c["yaw"], 1.0, wc.GRAD_BOUNDS)[2]
    assert (d >= 1.0).all() and (d <= 2.0 + 1e-5).all()
    alias = np.abs(d - d[:, np.arange(c["N"]) % T])[:, T:]
    print(f"{name}: {int((d < 1.9).sum())} one-sided quotients, {int((alias > 0.1).sum())} beyond tile 0 unlike their alias")
    assert (alias > 0.1).any()


def test_the_copied_alternatives_sit_beyond_tile_zero():
    """C65: one alternative per farm has the bits of its base entry, in a row of the LAST tile; C256: in tile 32, so that the
    last tile's single row stays a row of its own.  Every other alternative differs from its base entry."""
    for name, tiles_of_copies in (("C65", {7}), ("C256", {32})):
        c = wc.case(name)
        K, T = c["K"], wc.REACHES[name]["tiles"][0]
        same = c["alt"].view(np.uint32) == c["yaw"].view(np.uint32)[:, :, None]
        assert same.sum() == len(c["copies"])
        rows = []
        for b, i, k in c["copies"]:
            assert same[b, i, k]
            rows.append(1 + i * K + k)
        assert min(rows) >= T and {r // T for r in rows} == tiles_of_copies, (name, rows)
    assert len(wc.REACHES["C65"]["tiles"]) == 8 and len({b for b, _, _ in wc.CASES["C65"]["copies"]}) == wc.CASES["C65"]["farms"]


@pytest.mark.parametrize("name", ["PC", "PD", "PE"])
def test_the_planner_cases_are_safe(name):
    """plan_ref.plan under the strict bounds: every farm is safe (the project's cap is 10 %; here none may be unsafe: the
    GPU test compares bits on all of them), and the search moves."""
    c, r = wc.case(name), wc.reference(name)
    print(f"case {name}, planner seed {c['seed']}: smallest margin {r['margin'].min():.2e}, largest strict return bound "
          f"{max(r['plan_bound'].max(), r['hold_bound'].max()):.2e}, gain over the hold {r['plan_return'] - r['hold_return']}")
    assert r["safe"].all() and np.isfinite(r["margin"]).all()
    assert r["plan"].shape == (c["farms"], c["H"], c["N"])
    assert (r["plan"] != 0.0).any(axis=(1, 2)).all() and (r["plan_return"] > r["hold_return"] + 100.0 * r["hold_bound"]).all()
    assert (r["winners"] >= 2).any()


@pytest.mark.parametrize("name", ["Y65", "R65"])
def test_the_kept_farms_decide_clearly(name):
    """Every kept farm has a reference margin >= MARGIN, and at least one of them steers."""
    c, r = wc.case(name), wc.reference(name)
    print(f"{name}: farms {c['keep']} of the {wc.N_WINDS} winds, margins {np.array2string(r['margin'], precision=2)}, "
          f"{int((r['yaw'] != 0.0).any(axis=1).sum())} of {c['farms']} steer")
    assert r["yaw"].shape == (c["farms"], 65) and (r["margin"] >= MARGIN).all()
    assert (r["yaw"] != 0.0).any() and (r["power"] > r["power_initial"]).any()
    assert sorted(c["keep"]) == list(c["keep"]) and max(c["keep"]) < wc.N_WINDS


@pytest.mark.parametrize("name", ["L65", "L256", "LK", "LE"])
def test_the_top_two_returns_are_apart(name):
    """In strict bounds the top two returns of every farm are further apart than the sum of their return bounds (the
    condition tests/test_lookahead_gpu.py states): `best` is comparable.  Gates are open and closed."""
    r = wc.reference(name)
    gap, need = wc.top_two_gap(r)
    print(f"{name}: top-two gap / sum of the two bounds {np.array2string(gap / need, precision=1)}; closed gates {r['gated'].mean():.2f}")
    assert (gap > need).all()
    assert r["gated"].any() and not r["gated"].all()
    assert (r["best"] != 0).all()  # (holding is never the best sequence here: the argmax has something to find)
