"""CPU: the cases of tests/policy_wide_cases.py — that each one reaches the branch of the policy / policy-scenario glue kernels
it is for, by the plan's and the launchers' arithmetic restated in Python; that the cases of tests/policy_ref.py and
tests/polscen_ref.py do NOT reach those branches (the reason for this file); that the restated plan fits its LDS over a sweep
of shapes; and that the references alone make the GPU comparisons of tests/test_policy_wide_gpu.py bite: policies that move
and differ, rows of a later tile and of a later pass that act unlike their aliases in the first, members whose paths differ,
distinct scores.  The same functions pick the cases' seeds (policy_wide_cases.SEED_SEARCH)."""
import itertools

import numpy as np
import pytest

import policy_ref as pr
import policy_wide_cases as wc
import polscen_ref as sr


@pytest.mark.parametrize("name", list(wc.CASES))
def test_every_case_reaches_its_branch(name):
    """What policy_wide_cases.REACHES writes out for the case is what the restated arithmetic gives, every key of it."""
    got, want = wc.launch(name), wc.REACHES[name]
    print(name, got)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


def test_the_claims_are_the_branches():
    """The claims themselves, in the terms of the kernels: a second and a ragged last advance tile, T set by the cap, by the
    budget and by C, a second network pass, a last pass that is no multiple of four inside a strided layer loop, four layers,
    width 256, a second reduce tile, the transpose's grid stride, tiles that straddle members (with padding slots), several
    returns tiles, stats passes and paths blocks, and the limits K = 64, M = 64, H = 256."""
    r = wc.REACHES
    assert set(r) == set(wc.CASES)
    for name in ("PT", "PS", "PW", "PH", "P256C", "P256S", "PR", "ES", "ER"):
        t = r[name]["advance_tiles"]
        assert len(t) > 1 and t[-1] < t[0] == r[name]["T"], name  # a second tile (s0 > 0), the last one ragged (nt < T)
    assert [r[n]["T"] for n in ("PT", "PS", "PW", "PR", "ES", "EM")] == [16] * 6 and wc.POLICY["PT"][1] > 16  # the 16-row cap
    for name, C in (("PH", 11), ("P256C", 3), ("P256S", 4)):  # the LDS budget: below the cap and below C
        assert r[name]["T"] < min(16, C) and wc.POLICY[name][1] == C, name
    assert r["PHS"]["T"] == wc.POLICY["PHS"][1] == 5 and r["PL"]["T"] == 2  # ... and C itself
    assert r["P256S"]["lds_bytes"] == 56 * 1024  # the budget to the byte
    for name in ("PS", "PW", "PHS", "P256S"):
        assert all(len(p) > 1 for nt, p in r[name]["passes"].items() if nt == r[name]["T"]), name  # b0 > 0
    # a last pass whose cnt is no multiple of four (its last group has invalid instances) while that layer loop is strided
    assert r["PS"]["passes"][2] == [14] and 14 % 4 == 2 and r["PS"]["layer_trips"][14][0] == 2
    assert r["PHS"]["passes"][5][-1] == 10 and r["PW"]["passes"][2][-1] == 2
    assert len(wc.POLICY["PW"][3]) + 1 == 4 and 256 in wc.POLICY["PW"][3] and r["PW"]["layer_trips"][12][0] == 3
    assert max(r["PS"]["layer_trips"][48]) == 4 and r["P256C"]["obs_trips"] == 7
    assert r["PR"]["reduce_tiles"] == [64, 6] and r["PR"]["reduce_threads"] == 256 and wc.POLICY["PR"][7]  # (discrete)
    assert r["PK"]["transpose_trips"] == 6 and wc.POLICY["PK"][8] == 64 and wc.POLICY["PL"][9] == 256
    assert r["ES"]["straddles"] == 2 and r["ER"]["straddles"] == 2 and r["ER"]["chunks"] == [17, 2]  # 15 padding slots
    assert r["ES"]["passes"][16] == [48] and r["ES"]["layer_trips"][48][0] == 4
    assert r["EM"]["returns_tiles"] == [64, 64, 64] and r["EM"]["stats_passes"] == [4, 1] and r["EM"]["stats_load_trips"] == 2
    assert r["EM"]["paths_blocks"] == 3 and r["EM"]["straddles"] == len(r["EM"]["advance_tiles"]) == 12
    assert wc.ENSEMBLE["EM"]["M"] == 64 and wc.ENSEMBLE["ET"]["tails"] == (1, 7, 64) and wc.ENSEMBLE["ET"]["process"] == sr.STILL
    # the restated arithmetic against what the library's own documents state
    assert wc.polscen_tile(7, 35) == [35] and wc.chunk_slots(7, 15, 32) == (2, [2, 2, 2, 1])  # tests/test_polscen.py


def _old_launch(c, M=1, max_eval_farms=None, ensemble=False):
    return wc.launch_of(c["spec"]["kind"], c["spec"]["widths"], c["N"], c["B"], c["K"], M, max_eval_farms, ensemble)


def test_the_old_cases_stay_on_the_simplest_paths():
    """The reason for this file, kept checked.  Every case of policy_ref: ONE advance tile per policy with nt == T == C, one
    network pass, one trip of every layer loop, one reduce tile, one transpose trip.  Every case of polscen_ref, at every
    max_eval_farms tests/test_polscen_gpu.py runs: one network pass per tile, one returns tile, one stats pass of one load
    trip, one paths block.  (Under an ensemble the plan is made for M C rows, so there the old cases DO hold tiles that span
    members — every one but `edge` — and three of them a second tile; what they lack is the shared kind in such tiles beyond
    one pass, padding slots inside a straddling tile of several, and everything after the advance kernel.)"""
    for name in pr.NAMES:
        c = pr.case(name)
        g = _old_launch(c)
        print(name, g)
        assert g["chunks"] == [c["B"]] and g["advance_tiles"] == [g["T"]] == [c["B"]] and g["straddles"] == 0, name
        assert list(g["passes"].values()) == [[g["MB"]]], name
        assert all(t == 1 for trips in g["layer_trips"].values() for t in trips), name
        assert g["reduce_tiles"] == [c["B"]] and g["transpose_trips"] == 1, name
    seen = {}
    for name in sr.NAMES:
        s = sr.case(name)
        for me in ((32, 300, 47) if name == "ragged" else (None,)):
            g = seen[name, me] = _old_launch(s["c"], s["M"], me, ensemble=True)
            print(name, me, g)
            assert all(len(p) == 1 for p in g["passes"].values()), (name, me)
            assert len(g["returns_tiles"]) == 1 and len(g["stats_passes"]) == 1 and g["stats_load_trips"] == 1 and g["paths_blocks"] == 1
            assert g["transpose_trips"] == 1 and s["K"] * s["M"] <= 256 and s["K"] <= 3 and s["M"] <= 5
    assert {k: g["advance_tiles"] for k, g in seen.items() if len(g["advance_tiles"]) > 1} == {
        ("abl_central", None): [16, 5], ("horns_central", None): [9, 3], ("ragged", 300): [16, 16, 3]}
    assert all(s["c"]["spec"]["kind"] == "central" for s in map(sr.case, ("abl_central", "horns_central", "ragged")))


KINDS = ("central", "shared")
WIDTHS = ((1,), (5,), (65, 5), (256,), (256, 65, 5), (256, 256, 256))


@pytest.mark.parametrize("N", [1, 3, 7, 80, 255, 256])
def test_the_plan_fits_its_lds(N):
    """The restated plan over C in {1, 2, 15, 16, 17, 100}, both kinds, hidden widths from (1,) to (256, 256, 256), both
    encodings: 1 <= T <= 16, T <= C, MB >= 1, lds_bytes <= 64 KiB — the launch's limit, which the library checks; here never
    more than the 56 KiB budget and the plan's 16 spare bytes —, and the kernel's regions in its order end inside lds_bytes."""
    for kind, hidden, C, per, fw in itertools.product(KINDS, WIDTHS, (1, 2, 15, 16, 17, 100), (1, 3), (False, True)):
        D = 3 * N + 2 if kind == "central" else (5 if fw else 3)
        widths = (D,) + hidden + (per * N if kind == "central" else per,)
        p = wc.policy_plan(kind, widths, N, C)
        assert 1 <= p["T"] <= min(16, C) and p["MB"] >= 1, (kind, widths, C, p)
        assert p["MB"] == p["T"] if kind == "central" else p["MB"] <= p["T"] * N
        regions = wc.plan_regions(p, N)
        end = regions[-1][1] + regions[-1][2]
        assert all(b == a[1] + a[2] for a, (_, b, _) in zip(regions, regions[1:]))
        assert end <= p["lds_bytes"], (kind, widths, C, end, p)
        assert regions[4][1] % 8 == 0  # x0, the first double after the float tile, is aligned
        assert p["lds_bytes"] <= 56 * 1024 + 16 <= 64 * 1024, (kind, widths, C, p)  # (the budget and the plan's 16 spare bytes)


# ---- the properties of the references: what the seeds are picked by -------------------------------------------------------
def _aliases(g, N, shared, C):
    """For a launch `g`: [(row j, turbine t, row j', turbine t')] — (j, t) is served by a later tile or a later pass than the
    first, and (j', t') is what an index without the tile's `s0` / the pass's `b0` would read in its place."""
    out, s0 = [], 0
    for nt in g["advance_tiles"]:
        if s0:
            out += [(s0 + r, t, r, t) for r in range(nt) for t in range(N)]
        if shared:
            b0 = 0
            for cnt in g["passes"][nt]:
                if b0:
                    out += [(s0 + (b0 + i) // N, (b0 + i) % N, s0 + i // N, i % N) for i in range(cnt)]
                b0 += cnt
        s0 += nt
    return out


def policy_properties(name, c, r):
    """Raises AssertionError unless the reference `r` of the policy case `c` shows what the GPU test relies on."""
    K, N = c["K"], c["N"]
    discrete = c["env"]["discrete"]
    hold = np.float32(1.0 if discrete else 0.0)
    assert (r["actions"] != hold).mean() > (0.25 if discrete else 0.5), "the policies do not move the turbines"
    assert all((r["actions"][:, i] != r["actions"][:, j]).any() for i in range(K) for j in range(i + 1, K)), "two policies act alike"
    if discrete:
        assert (r["margin"] > 1e-9).all(), f"a discrete turbine's two best outputs are {r['margin'].min():.1e} apart"
        assert len(np.unique(r["actions"])) == 3
    g = wc.launch(name) if name in wc.POLICY else None  # (a policy case under an ensemble is tiled by the ensemble's rows)
    if g is not None and (len(g["advance_tiles"]) > 1 or any(len(p) > 1 for p in g["passes"].values())):
        pairs = np.array(_aliases(g, N, c["kind"] == "shared", c["B"]))
        a = r["actions"]  # (B, K, H, N): row j is farm j
        unlike = (a[pairs[:, 0], :, :, pairs[:, 1]] != a[pairs[:, 2], :, :, pairs[:, 3]])  # (pairs, K, H)
        if discrete:  # three values per turbine: a ROW, over its turbines and policies, is unlike its alias row
            rows = {j: unlike[pairs[:, 0] == j, :, 0].any() for j in np.unique(pairs[:, 0])}
            assert all(rows.values()), f"rows {[j for j, u in rows.items() if not u]} of a later tile repeat their alias at step 0"
            return f"{len(rows)} aliased rows, all unlike at step 0; {unlike.mean():.3f} of their entries over all steps"
        assert unlike[:, :, 0].all(), f"{(~unlike[:, :, 0]).sum()} entries of a later tile / pass repeat their alias at step 0"
        return f"{len(pairs)} aliased entries, all unlike at step 0, {unlike.mean():.3f} over all steps"
    return ""


def ensemble_properties(name, s, ref):
    """The same for an ensemble case `s` (not under STILL) and polscen_ref.rollouts' `ref`."""
    c = s["c"]
    K, M, N, C = s["K"], s["M"], s["N"], s["B"]
    a = ref["actions"]  # (B, K, M, H, N)
    assert (a != np.float32(0.0)).mean() > 0.5, "the policies do not move the turbines"
    assert all((a[:, i] != a[:, j]).any() for i in range(K) for j in range(i + 1, K)), "two policies act alike"
    w = ref["wind_paths"]  # (B, M, H, 2)
    assert all((w[:, i] != w[:, j]).any(axis=(1, 2)).all() for i in range(M) for j in range(i + 1, M)), "two members of a farm share a path"
    assert all((w[:, i, -1, 1] != w[:, j, -1, 1]).all() for i in range(M) for j in range(i + 1, M))  # (no clip on a direction)
    mr = ref["member_returns"]
    assert all((mr[:, :, i] != mr[:, :, j]).all() for i in range(M) for j in range(i + 1, M)), "two members return alike"
    g = wc.launch(name)
    pairs = np.array(_aliases(g, N, c["kind"] == "shared", C))  # rows j = m C + slot of the whole run's one chunk
    if len(pairs):
        rows = a.transpose(2, 0, 1, 3, 4).reshape(M * C, K, s["H"], N)  # row j = m C + slot
        unlike = rows[pairs[:, 0], :, :, pairs[:, 1]] != rows[pairs[:, 2], :, :, pairs[:, 3]]
        assert unlike.any(axis=2).all(), "a row of a later tile repeats its alias at every step"
        if g["straddles"] and C > g["T"]:
            assert unlike[:, :, 0].all()  # (the alias lies in another slot: unlike from observation 0 on)
    if name == "EM":
        sc = ref["score"]
        assert all((sc[:, i] != sc[:, j]).all() for i in range(K) for j in range(i + 1, K)), "two policies score alike"
        assert len(np.unique(ref["best"])) >= 1
    return f"{len(pairs)} aliased entries"


@pytest.mark.parametrize("name", wc.POLICY_NAMES)
def test_policy_references_show_what_the_cases_are_aimed_at(name):
    """policy_ref.rollout alone, per case: the policies move the turbines; the K policies differ; every discrete turbine's
    two best outputs are more than 1e-9 apart, no turbine left out; every entry a later tile or a later pass serves acts, at
    step 0, unlike the entry an index without s0 / b0 would read.  The kept seed is the first of SEED_SEARCH's start, + 1, ..
    for which this holds."""
    c, r = wc.case(name), wc.reference(name)
    first, kept = wc.SEED_SEARCH[name]
    assert kept == wc.POLICY[name][-1] >= first
    print(f"{name}: seed {kept} (search from {first}): {policy_properties(name, c, r)}")
    H, B, K, N = c["H"], c["B"], c["K"], c["N"]
    assert r["actions"].shape == (B, K, H, N) and r["observations"].shape == (B, K, H, 3 * N + 2)
    assert (c["state"]["yaw"][:, 0] == 40.0).all()
    for seed in range(first, kept):  # the seeds passed over fail, or the rule was not followed
        with pytest.raises(AssertionError):
            policy_properties(name, wc.case(name, seed), wc.reference(name, seed))


@pytest.mark.parametrize("name", ["ES", "EM"])
def test_ensemble_references_show_what_the_cases_are_aimed_at(name):
    """polscen_ref.rollouts alone: the policies move and differ, every two members' paths differ in every value and their
    returns in every (farm, policy), every row of a later tile acts unlike its alias, EM's five scores are pairwise distinct
    on every farm.  The policy case under the ensemble passes policy_properties too (it is what the seed is picked by)."""
    s, ref = wc.ensemble(name), wc.ensemble_reference(name)
    first, kept = wc.SEED_SEARCH[name]
    assert kept == wc.BASES[name][-1] >= first
    print(f"{name}: seed {kept} (search from {first}): {ensemble_properties(name, s, ref)}; "
          f"{policy_properties(name, s['c'], wc.reference(name))}")
    assert ref["member_returns"].shape == (s["B"], s["K"], s["M"]) and ref["wind_paths"].shape == (s["B"], s["M"], s["H"], 2)
    for seed in range(first, kept):  # the seeds passed over fail, or the rule was not followed
        with pytest.raises(AssertionError):
            policy_properties(name, wc.case(name, seed), wc.reference(name, seed))
            ensemble_properties(name, wc.ensemble(name, seed), wc.ensemble_reference(name, seed))


def test_the_still_ensemble_ties_every_member():
    """ET on the reference: under polscen_ref.STILL every path is the current wind held, every member return of a policy is the
    same value, and the ranks are the member indices: the tail mean of any q is that value's running sum over q."""
    import scenario_ref

    s, ref = wc.ensemble("ET"), wc.ensemble_reference("ET")
    held = np.stack([s["ws"], s["wd"]], axis=1)[:, None, None]
    assert np.array_equal(ref["wind_paths"], np.broadcast_to(held, ref["wind_paths"].shape))
    mr = ref["member_returns"]
    assert (mr == mr[:, :, :1]).all()
    assert np.array_equal(scenario_ref.ranks(mr), np.broadcast_to(np.arange(s["M"]), mr.shape))
    assert all((mr[:, i, 0] != mr[:, j, 0]).all() for i in range(s["K"]) for j in range(i + 1, s["K"]))  # (the policies still differ)
