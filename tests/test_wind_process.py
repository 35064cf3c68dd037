"""CPU side of the checks of the on-device wind process: the properties of the NumPy reference (tests/wind_ref.py) that
tests/test_wind_process_gpu.py relies on, asserted on the reference alone — what each case is aimed at, that no draw sits
near a bin tie or a wrap (so device rounding cannot move a bin), and the range of the series start."""
import numpy as np
import pytest

import plan_ref
import wind_ref as wr

B = wr.B_CASES


@pytest.fixture(scope="module")
def drawn():
    return {name: (wr.dist_of(ov), wr.sample(seed, B, ov), wr.binned(seed, B, ov, step)) for name, (seed, ov, step) in wr.CASES.items()}


def test_batch_spans_blocks_with_a_partial_last_one():
    assert B == 4099 and (B + 255) // 256 == 17 and B % 256 == 3


def test_u01_is_the_53_bit_midpoint_grid():
    z, f = np.array([0], np.uint32), np.array([0xFFFFFFFF], np.uint32)
    assert wr.u01(z, z)[0] == 2.0 ** -54 and wr.u01(f, f)[0] == 1.0 - 2.0 ** -54
    assert wr.u01(np.array([1], np.uint32), z)[0] == (2.0 ** 21 + 0.5) * 2.0 ** -53  # hi is the upper word
    assert wr.u01(z, np.array([1 << 11], np.uint32))[0] == 1.5 * 2.0 ** -53  # the low 11 bits of lo are dropped
    assert wr.u01(z, np.array([(1 << 11) - 1], np.uint32))[0] == 2.0 ** -54


def test_cases_show_what_they_are_aimed_at(drawn):
    d, s, b = drawn["default"]
    assert (s["ws"] == d["ws_lo"]).sum() == 2 and (s["ws_raw"] < d["ws_lo"]).sum() == 2
    assert ((s["wd_raw"] >= 0) & (s["wd_raw"] < 360)).all() and np.array_equal(s["wd"], s["wd_raw"])
    d, s, b = drawn["wrap"]
    assert (s["wd_raw"] >= 360.0).sum() == 1501 and b["folded"].sum() == 514 and b["K"] == 180
    assert (b["bin"][b["folded"]] == 0).all() and (b["wd"][b["folded"]] == 0.0).all()
    d, s, b = drawn["clip"]
    assert ((s["ws"] == d["ws_lo"]).sum(), (s["ws"] == d["ws_hi"]).sum()) == (1256, 561)
    assert ((s["wd"] == d["wd_lo"]).sum(), (s["wd"] == d["wd_hi"]).sum()) == (395, 385)
    assert (s["ws"] >= d["ws_lo"]).all() and (s["ws"] <= d["ws_hi"]).all() and (s["wd"] >= 100.0).all() and (s["wd"] <= 260.0).all()
    d, s, b = drawn["neg"]
    assert (s["wd_raw"] < 0.0).sum() == B and (s["wd_raw"] < -360.0).sum() > B // 2  # more than one turn below 0
    assert (s["wd"] >= 0.0).all() and (s["wd"] < 360.0).all() and b["folded"].sum() == 885 and b["K"] == 8
    # the wrapped direction is the raw one modulo 360, to rounding
    for name, (d, s, b) in drawn.items():
        t = (s["wd_wrapped"] - s["wd_raw"]) / 360.0
        assert np.abs(t - np.rint(t)).max() < 1e-12, name


def test_no_draw_sits_near_a_bin_tie_or_a_wrap(drawn):
    """The condition under which the binned comparison may be exact on every farm: device rounding (a few ulp of a direction
    below 1000 degrees in magnitude, 1e-12 deg) cannot cross a margin of 1e-5 bins or 1e-6 deg."""
    worst = 1.0
    for name, (d, s, b) in drawn.items():
        assert wr.tie_margin(b["q"]) >= 1e-5, name
        assert wr.wrap_margin(s["wd_raw"]) >= 1e-6, name
        assert np.abs(s["wd_raw"]).max() < 1000.0
        worst = min(worst, wr.tie_margin(b["q"]))
        assert np.array_equal(b["wd"], b["bin"] * wr.CASES[name][2]) and b["bin"].min() >= 0 and b["bin"].max() < b["K"]
        # the binned directions differ from the un-binned ones: the two paths cannot be confused
        assert (b["wd"] != s["wd"]).mean() > 0.8, name
    assert 5e-5 < worst < 6e-5  # (the clip case)


def test_seeds_that_differ_above_bit_31_give_different_draws():
    for name in ("wrap", "clip"):
        seed, ov, _ = wr.CASES[name]
        assert seed >> 32 and seed < 2 ** 64
        a, lo = wr.sample(seed, B, ov), wr.sample(seed & 0xFFFFFFFF, B, ov)
        assert (a["ws_raw"] != lo["ws_raw"]).mean() > 0.99 and (a["wd_raw"] != lo["wd_raw"]).mean() > 0.99
    assert (wr.series_start(5, B, 65537) != wr.series_start(5 + (1 << 32), B, 65537)).mean() > 0.99


def test_streams_and_words_are_all_distinct():
    """Each of the mistakes the device comparison is to catch moves the reference itself by order one."""
    seed, ov, _ = wr.CASES["default"]
    b = np.arange(B, dtype=np.uint64)
    r0, r1, r2 = (plan_ref.philox4x32_10(seed, b, s) for s in (0, 1, 2))
    s = wr.sample(seed, B, ov)
    rad = np.sqrt(-2.0 * np.log(wr.u01(r0[:, 2], r0[:, 3])))
    swapped = 270.0 + 20.0 * np.sqrt(-2.0 * np.log(wr.u01(r0[:, 3], r0[:, 2]))) * np.cos(2.0 * np.pi * wr.u01(r1[:, 0], r1[:, 1]))
    stream0 = 270.0 + 20.0 * rad * np.cos(2.0 * np.pi * wr.u01(r0[:, 0], r0[:, 1]))
    for other in (swapped, stream0):
        assert np.median(np.abs(other - s["wd_raw"])) > 1.0
    assert (r0 != r1).all() and (r1 != r2).any(axis=1).all()


def test_series_start_is_a_multiply_shift_below_T():
    for T in (1, 2, 7, 65537, 2 ** 31 - 1):
        st = wr.series_start(5, B, T)
        assert st.dtype == np.int32 and st.min() >= 0 and st.max() < T
    assert (wr.series_start(5, B, 1) == 0).all() and set(wr.series_start(5, B, 2)) == {0, 1}
    assert set(wr.series_start(5, B, 7)) == set(range(7))
    # an off-by-one of the shift or the product would show: the starts follow the word, floor(word T / 2^32)
    word = plan_ref.philox4x32_10(5, np.arange(B, dtype=np.uint64), 2)[:, 0].astype(object)
    T = 65537
    assert [int(w * T // 2 ** 32) for w in word] == list(wr.series_start(5, B, T))
    assert wr.series_start(5, B, 2 ** 31 - 1).max() > 2 ** 30  # the range is used: the product needs 64 bits
