"""The lean float64 routines of csrc/wf_f64_math.h on the device, through the hook library libwfcheck.so (built from
csrc/check/wf_math_check.hip under the product's flags), against mpmath at 50 digits: arguments, references, the error measure
and the bounds are tests/f64_math_cases.py's.  Every test prints the routine's worst error next to the device library's on the
same arguments (run with -s to see them); only the lean figure is asserted."""
import numpy as np
import pytest

import f64_math_cases as fc
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return helpers.load_wfcheck()


def _fmt(fig):
    return ", ".join(f"{k} {v:.3g}" for k, v in fig.items())


@pytest.mark.parametrize("name", sorted(fc.IDS))
def test_routine_within_its_bound(lib, name):
    args = fc.cases(name)
    got = helpers.math_check(lib, fc.IDS[name], *args, n_out=fc.N_OUT[name])
    ref = helpers.math_check(lib, fc.LIB_IDS[fc.LIB_OF[name]], *args, n_out=fc.N_OUT[name])
    fig, bad = fc.violations(name, got)
    lib_fig, _ = fc.violations(name, ref)
    print(f"\n[f64] {name:13s} n {args[0].size:5d} | lean: {_fmt(fig)} | library: {_fmt(lib_fig)}")
    if bad.size:
        i = bad[:5]
        detail = [(tuple(float(a[j]).hex() for a in args), tuple(float(g[j]) for g in got),
                   tuple(float(fc.ulp_error(g, r)[j]) for g, r in zip(got, fc.reference(name)))) for j in i]
        pytest.fail(f"{name}: {bad.size} of {args[0].size} arguments outside the bound ({_fmt(fig)}); first: {detail}")


def test_special_values(lib):
    for name, args, want in fc.SPECIALS:
        (got,) = helpers.math_check(lib, fc.IDS[name], *(np.array([a]) for a in args))
        got = float(got[0])
        if want != want:
            assert got != got, (name, args, got)
        else:
            assert got == want and np.signbit(got) == np.signbit(want), (name, args, got, want)


def test_launcher_handles_a_last_partial_block_and_refuses_bad_arguments(lib):
    import torch

    x = np.linspace(0.5, 2.0, 257 * 3)  # four blocks, the last one with 3 threads
    (got,) = helpers.math_check(lib, fc.IDS["sqrt_pos"], x)
    assert np.abs(got / np.sqrt(x) - 1.0).max() < 5e-16
    t = torch.ones(4, dtype=torch.float64, device="cuda")
    assert lib.wf_math_check(fc.IDS["pow_any"], t.data_ptr(), None, t.data_ptr(), None, 4, None) == -1  # second input missing
    assert lib.wf_math_check(fc.IDS["rcp64"], None, None, t.data_ptr(), None, 4, None) == -1
    assert lib.wf_math_check(fc.IDS["rcp64"], t.data_ptr(), None, t.data_ptr(), None, 0, None) == 0
    (nan,) = helpers.math_check(lib, 57, x[:4])  # an id nobody defined
    assert np.isnan(nan).all()
