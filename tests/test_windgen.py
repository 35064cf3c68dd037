"""CPU: the wind generator extension (include/wfwindgen.h) — header, binding table, kernel metadata — and the properties of the
reference the GPU tests use (tests/windgen_ref.py: the synthetic wind process restated in NumPy)."""
import os
import re

import numpy as np
import pytest

import wind_ref
import windgen_ref
from conftest import ROOT
from ext_checks import assert_no_private_segment, compile_kernels, declared, makefile

B, T = windgen_ref.B_CASES, windgen_ref.T_CASES
ROW_EXTENSIONS = ("credit", "lookahead", "plan", "rollout", "retgrad")


@pytest.fixture(scope="module")
def cases():
    return {name: windgen_ref.case(name) for name in windgen_ref.CASES}


def test_windgen_header_is_bound_and_exported():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    syms = declared("wfwindgen.h")
    want = ["wf_windgen_" + n for n in ("create", "destroy", "generate", "set_kernel", "step", "get", "seek", "window", "read", "kernel_info",
                                        "last_error")] + [f"wf_{x}_set_wind_source" for x in ROW_EXTENSIONS]
    assert syms == sorted(want)
    assert sorted(_lib.WINDGEN_ABI) == syms
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.wf_version() == 7  # (wfstep.h and WF_ABI_VERSION are not touched)
    for table in (_lib.ABI, _lib.PROBE_ABI, _lib.YAWOPT_ABI, _lib.ROSE_ABI, _lib.ROBUST_ABI, _lib.GRAD_ABI, _lib.CREDIT_ABI,
                  _lib.LOOKAHEAD_ABI, _lib.PLAN_ABI, _lib.SERIES_ABI, _lib.ROLLOUT_ABI, _lib.RETGRAD_ABI):
        assert not set(table) & set(_lib.WINDGEN_ABI)
    assert [n for n, _ in _lib.WindProcess._fields_] == list(windgen_ref.KEYS)
    text = open(os.path.join(ROOT, "include", "wfwindgen.h")).read()
    assert "THE PROJECT'S OWN definitions" in text and "PARITY UNPINNED beyond" in text and "tests/windgen_ref.py" in text
    assert "act AT TICK 0 ONLY" in text  # (wd_lo / wd_hi)
    assert re.search(r"^#define WF_WINDGEN_KERNELS 2$", text, flags=re.M)


def test_windgen_kernels_have_no_private_segment(tmp_path):
    """The generator's two kernels, compiled with the Makefile's flags: exactly these, no private segment, no spilled register,
    no out-of-line call; no LDS in the serial one, the 32 KiB tile in the other.  Metadata only."""
    mk = makefile()
    assert "WINDGENOBJ = windgen/wf_windgen_kernels.o windgen/wf_windgen_abi.o" in mk and "$(WINDGENOBJ): %.o: %.hip" in mk
    assert re.search(r"^\$\(OUT\):.*\$\(WINDGENOBJ\)", mk, flags=re.M) and re.search(r"^\trm -f .*windgen/\*\.o", mk, flags=re.M)
    assert "-ffp-contract=off" in mk
    seen, text = compile_kernels("windgen/wf_windgen_kernels.hip", tmp_path)
    assert_no_private_segment(seen, ("wf_windgen_kernel", "wf_windgen_tiled_kernel"))
    lds = {("tiled" if "tiled" in n else "serial"): m["group_segment_fixed_size"] for n, m in seen.items()}
    assert lds == {"serial": 0, "tiled": 2 * 32 * 64 * 8}, seen
    assert "s_swappc_b64" not in text


def test_the_planner_and_the_generator_share_one_deviate():
    """The deviate moved from the planner's kernels into a header both include: one definition."""
    csrc = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    plan = open(os.path.join(csrc, "plan", "wf_plan_kernels.hip")).read()
    gen = open(os.path.join(csrc, "windgen", "wf_windgen_kernels.hip")).read()
    head = open(os.path.join(csrc, "ext", "wf_deviate.h")).read()
    assert '#include "../ext/wf_deviate.h"' in plan and '#include "../ext/wf_deviate.h"' in gen
    assert "1.7320508075688772" in head and "1.7320508075688772" not in plan and "1.7320508075688772" not in gen


def test_default_case_gives_every_farm_a_wind_of_its_own(cases):
    g = cases["default"]
    assert g["ws"].shape == g["wd"].shape == (T, B)
    assert len({(s, d) for s, d in zip(g["ws"][5], g["wd"][5])}) == B  # all 259 farms distinct at tick 5
    s = wind_ref.sample(windgen_ref.CASES["default"][0], B, windgen_ref.CASES["default"][1])
    assert np.array_equal(g["ws"][0], s["ws"]) and np.array_equal(g["wd"][0], s["wd"])  # tick 0 is the reset draw
    assert (g["rate"] == 0.0).all()  # (no ramp)


def test_clip_case_stores_speeds_on_both_bounds_and_directions_past_the_reset_bounds(cases):
    g, d = cases["clip"], wind_ref.dist_of(windgen_ref.CASES["clip"][1])
    ws, wd = g["ws"][1:], g["wd"][1:]
    assert int((ws == d["ws_lo"]).sum()) == 2636 and int((ws == d["ws_hi"]).sum()) == 1621
    assert ws.min() == d["ws_lo"] and ws.max() == d["ws_hi"]
    assert int((g["x"] < d["ws_lo"]).sum()) == 2636 and int((g["x"] > d["ws_hi"]).sum()) == 1621  # the latent is not clipped
    # wd_lo / wd_hi act at tick 0 only
    assert ((g["wd"][0] >= d["wd_lo"]) & (g["wd"][0] <= d["wd_hi"])).all()
    assert int(((wd < d["wd_lo"]) | (wd > d["wd_hi"])).sum()) == 1021


def test_wrap_case_crosses_zero_and_a_full_turn(cases):
    g = cases["wrap"]
    assert int((g["y"] < 0.0).sum()) == 1314 and int((g["y"] >= 360.0).sum()) == 1539
    assert ((g["wd"] >= 0.0) & (g["wd"] < 360.0)).all()
    assert np.array_equal(g["wd"], windgen_ref.wrap360(g["y"]))


def test_ramp_case_leaves_the_first_turn_on_both_sides(cases):
    g = cases["ramp"]
    assert int((g["y"] < -360.0).sum()) == 1007 and int((g["y"] >= 720.0).sum()) == 94
    assert ((g["wd"] >= 0.0) & (g["wd"] < 360.0)).all()
    assert (np.abs(g["rate"]) < 25.0).all() and (g["rate"] < 0).any() and (g["rate"] > 0).any()
    assert len(set(g["rate"])) == B  # a ramp of its own per farm


def test_frozen_case_holds_tick_0(cases):
    g = cases["frozen"]
    assert (g["ws"] == g["ws"][0]).all() and (g["wd"] == g["wd"][0]).all()


def test_a_given_tick_0_is_wrapped_not_clipped():
    ws0 = np.full(5, 40.0)  # above the default ws_hi = 28: stored as given
    wd0 = np.array([-725.0, -0.0, 360.0, 725.0, 359.5])
    g = windgen_ref.generate(7, 5, 3, windgen_ref.process_of((0.5, 0.0, 0.0, 0.0, 0.0)), None, (ws0, wd0))
    assert np.array_equal(g["ws"][0], ws0) and np.array_equal(g["wd"][0], [355.0, 0.0, 0.0, 5.0, 359.5])
    assert (g["ws"][1:] == 28.0).all()  # ... while the latent stays at 40 and later speeds are clipped


def test_a_farms_series_does_not_depend_on_the_batch():
    for name in ("default", "ramp"):
        seed, dist, process = windgen_ref.CASES[name]
        big, small = windgen_ref.generate(seed, B, T, process, dist), windgen_ref.generate(seed, 7, T, process, dist)
        for k in ("ws", "wd", "x", "y"):
            assert np.array_equal(big[k][:, :7], small[k]), (name, k)


def test_window_of_the_reference_holds_the_last_tick():
    g = windgen_ref.case("default", B=9, T=6)
    w, avail = windgen_ref.window(g, t=3, first=1, H=4, farms=[8, 2, 2])
    assert avail == 2 and w.shape == (3, 4, 2)
    assert np.array_equal(w[0, :, 0], g["ws"][[4, 5, 5, 5], 8]) and np.array_equal(w[1], w[2])


def test_stationary_variance_of_the_speed():
    """B = 4099 farms from one speed, T = 400 ticks, no clip in reach: the sample variance of x over the farms at the last
    tick against sigma^2 / (1 - (1 - a)^2).  Measured on this reference: -2.3 % (0.62652 against 0.64103; the standard error
    of a sample variance over 4099 farms is about 2.2 %) — asserted within the 5 % the definition is held to."""
    a, sigma = 0.05, 0.25
    n = wind_ref.B_CASES
    g = windgen_ref.generate(1234, n, 400, windgen_ref.process_of((a, sigma, 0.0, 0.0, 0.0)), None,
                             (np.full(n, 8.0), np.full(n, 270.0)))
    x = g["x"][-1]
    assert x.min() > 3.0 and x.max() < 28.0
    want = sigma ** 2 / (1.0 - (1.0 - a) ** 2)
    got = float(x.var(ddof=1))
    print("variance", got, "expected", want, "relative", got / want - 1.0)
    assert abs(got / want - 1.0) < 0.05
    assert abs(float(x.mean()) - 8.0) < 4.0 * np.sqrt(want / n)
