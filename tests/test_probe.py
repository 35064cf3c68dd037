"""CPU: the probe extension (include/wfprobe.h) — header, binding table, kernel metadata — and a guard on the reference the
GPU tests use (tests/probe_ref.py: the numpy oracle with a ghost turbine)."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wf_[a-z0-9_]+)\s*\(", text)))


def test_probe_header_is_bound_and_the_step_abi_is_untouched():
    from wfcrl_env_amd import _lib

    lib = _lib.load()
    probe = _declared("wfprobe.h")
    assert {"wf_probe_create", "wf_probe_destroy", "wf_probe_set_points", "wf_probe_sample", "wf_probe_last_error"} <= set(probe)
    assert all(s.startswith("wf_probe_") for s in probe), probe
    for s in probe:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
        assert s in _lib.PROBE_ABI, f"PROBE_ABI lacks {s}"
        assert getattr(lib, s).argtypes == _lib.PROBE_ABI[s][1]  # bound by load()
    assert set(_lib.PROBE_ABI) == set(probe)
    assert lib.wf_version() == 7
    assert set(_lib.ABI) == set(_declared("wfstep.h"))
    assert not set(_lib.ABI) & set(_lib.PROBE_ABI)


def test_probe_kernels_have_no_private_segment(tmp_path):
    """Both probe kernels, compiled with the Makefile's flags: no private segment, no spilled vector or scalar register
    (a kernel with a private segment pays ~20 us per launch on MI355X: tests/test_abi.py states the measurement).  Metadata only."""
    src = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^FLAGS \?= (.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "PROBEOBJ = probe/wf_probe_kernels.o probe/wf_probe_abi.o" in mk and "$(PROBEOBJ): %.o: %.hip" in mk and "\t$(HIPCC) $(FLAGS) -c -o $@ $<" in mk
    out = tmp_path / "wf_probe_kernels.s"
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(src, "probe", "wf_probe_kernels.hip")],
                   check=True, capture_output=True)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for block in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        seen[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "group_segment_fixed_size")}
    assert len(seen) == 2 and any("wf_probe_state_kernel" in n for n in seen) and any("wf_probe_sample_kernel" in n for n in seen), seen
    for name, m in seen.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 65536, (name, m)
    assert "s_swappc_b64" not in text  # no out-of-line call


@pytest.mark.parametrize("name", ["Turb3_Row1_", "Ablaincourt_", "Turb16_Row5_"])
@pytest.mark.parametrize("veer", [0.0, 5.0])
def test_ghost_reference_is_consistent_under_a_shift(layouts, name, veer):
    """Two ghosts a quarter diameter apart (laterally, in the wind frame) share six rotor-grid points: the oracle must give
    the same flow there from either — the reference does not depend on WHICH ghost carries a point.  A ghost does not move
    the real turbines upstream of it, and the TI grid of every real turbine — of every source that acts on a ghost — is
    uniform on these fixtures (so "the source's centre TI" is exactly what the oracle uses for every grid column).
    Bound 1e-11 m/s: the two runs rotate about different bounding-box centres, which perturbs coordinates of ~1e4 m by
    ~2e-12 m; with flow gradients below 0.1 (m/s)/m that is 2e-13 m/s, taken 50 x."""
    import probe_ref
    from oracle.floris_gch_numpy import ModelParams, farm_step

    l = layouts[name]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    N, p0 = len(x), ModelParams(veer=veer)
    rng = np.random.default_rng(zlib.crc32(f"ghost-shift/{name}/{veer}".encode()))
    for wd in (270.0, 251.3, 93.0):
        ws = rng.uniform(6.0, 12.0)
        yaw = rng.uniform(-30, 30, N)
        base = farm_step(x, y, ws, wd, yaw, p0, return_fields=True)
        assert np.ptp(base["TI"].reshape(N, 9), axis=1).max() == 0.0
        xr, yr, back = probe_ref.wind_frame(x, y, wd)
        for gx, gy, down in probe_ref.draw_ghosts(rng, x, y, wd, n_down=2, n_up=1):
            gxr, gyr, _ = probe_ref.wind_frame(np.append(x, gx), np.append(y, gy), wd)  # (another centre: compare differences)
            xp, yp = gxr[N] - gxr[0] + xr[0], gyr[N] - gyr[0] + yr[0]
            gx2, gy2 = back(xp, yp + p0.D / 4.0)
            a = probe_ref.ghost_fields(x, y, ws, wd, yaw, gx, gy, p0)
            b = probe_ref.ghost_fields(x, y, ws, wd, yaw, gx2, gy2, p0)
            for k in "UVW":
                assert np.abs(a[k][1:] - b[k][:2]).max() <= 1e-11, (name, wd, k)
            pa, pb = probe_ref.ghost_points(gx, gy, wd, p0), probe_ref.ghost_points(gx2, gy2, wd, p0)
            assert np.abs(pa[1:] - pb[:2]).max() <= 1e-9  # (the shared points ARE the same places)
            up = xr < xp - 1.0
            assert np.abs(a["U_real"][up] - base["U"][up]).max(initial=0.0) <= 1e-11
            assert a["sources_ti_uniform"] and b["sources_ti_uniform"]


def test_ghost_reference_where_a_source_has_a_ti_grid_of_its_own():
    """The branch of probe_ref.ghost_uvw the layouts above never take.  Turbine B stands 14 D behind the yawed turbine A
    and 2 D beside it: only one column of its rotor grid lies within the 2 D band of A's wake-added turbulence, so B's TI
    differs between its columns, and a ghost behind B reads in its side columns a TI that is not B's centre TI.
    ghost_uvw then takes each side column from the centre column of a ghost moved onto it.  Held here: the fixture does
    force that branch; the centre column is the plain ghost's, untouched; the side columns do differ from the plain ghost's
    (the repair is not a no-op); and the repaired reference depends on the place alone — two ghosts a quarter diameter
    apart agree on their six shared points within the 1e-11 m/s of the shift test above."""
    import probe_ref
    from oracle.floris_gch_numpy import ModelParams, farm_step

    p0 = ModelParams()
    D = p0.D
    x, y = np.array([0.0, 14.0 * D]), np.array([0.0, 2.0 * D])
    ws, wd, yaw = 8.0, 270.0, np.array([-25.0, 10.0])
    ti_b = farm_step(x, y, ws, wd, yaw, p0, return_fields=True)["TI"][1]
    assert np.ptp(ti_b[:, 1]) > 1e-3 and ti_b[0, 1] != ti_b[1, 1]  # B: a TI per column, the centre's differs from a side's
    gx, gy = 18.0 * D, 2.3 * D
    plain = probe_ref.ghost_fields(x, y, ws, wd, yaw, gx, gy, p0)
    assert not plain["sources_ti_uniform"]
    uvw, uniform = probe_ref.ghost_uvw(x, y, ws, wd, yaw, gx, gy, p0)
    assert not uniform
    assert np.array_equal(uvw[1], np.stack([plain["U"][1], plain["V"][1], plain["W"][1]], axis=-1))
    assert np.abs(uvw[0, :, 0] - plain["U"][0]).max() > 1e-6  # (B's side-column TI moves u behind it by far more than the tolerance in use)
    shifted, _ = probe_ref.ghost_uvw(x, y, ws, wd, yaw, gx, gy + D / 4.0, p0)
    pa, pb = probe_ref.ghost_points(gx, gy, wd, p0), probe_ref.ghost_points(gx, gy + D / 4.0, wd, p0)
    assert np.abs(pa[1:] - pb[:2]).max() <= 1e-9
    assert np.abs(uvw[1:] - shifted[:2]).max() <= 1e-11
    # a ghost upstream of B has A alone as its source, whose TI grid is uniform: one ghost is enough there
    assert probe_ref.ghost_uvw(x, y, ws, wd, yaw, 5.0 * D, 0.2 * D, p0)[1]
