"""CPU: the wind ensemble of include/wfscenario.h exists ONCE in the sources (csrc/ensemble/).  Source-level, no GPU: the four
extensions that score something over M wind futures — scenario/, scenplan/, rollscen/, polscen/ — take the path walk, the
statistics, the host checks and the Python argument handling from one place each and restate none of it."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
EXTENSIONS = ("scenario", "scenplan", "rollscen", "polscen")
DEVICE = os.path.join("ensemble", "wf_ensemble.h")
HOST = os.path.join("ensemble", "wf_ensemble_host.h")


def _sources():
    """{path under csrc/: text} of every source file there."""
    paths = [p for ext in ("*.h", "*.hip") for p in glob.glob(os.path.join(CSRC, "**", ext), recursive=True)]
    return {os.path.relpath(p, CSRC): open(p).read() for p in paths}


def test_the_four_kernel_files_include_the_ensemble():
    src = _sources()
    assert DEVICE in src and HOST in src
    for ext in EXTENSIONS:
        text = src[os.path.join(ext, "wf_%s_kernels.hip" % ext)]
        own = src[os.path.join(ext, "wf_%s.h" % ext)]
        # directly, or through the extension's own header (rollscen's includes the scenario extension's)
        assert "ensemble/wf_ensemble.h" in text + own + (src[os.path.join("scenario", "wf_scenario.h")] if ext == "rollscen" else ""), ext
        assert "wf_ensemble_" in text or "wf_member_statistics" in text, ext
        assert "KNOWN SECOND COPIES" not in text, ext


def test_the_path_walk_is_defined_once():
    """Outside ensemble/wf_ensemble.h no source file draws from Philox streams 16, 17 or 18 — a stream literal on a line with a
    Philox or deviate call —, and no file of the four extensions wraps a direction (fmod: the other users of fmod under csrc/
    — the step and resolve kernels, the visit order, the rose look-up, the wind generator — wrap other things)."""
    src = _sources()
    header = src[DEVICE]
    for literal in ("16u", "17u", "18u"):
        assert re.search(r"\b%s\b" % literal, header), literal
    assert "fmod(" in header and "WF_ENSEMBLE_TILE 2048" in header
    draw = re.compile(r"(philox4x32_10|wf_deviate)\w*\(.*\b1[678]u\b")
    for path, text in src.items():
        if path == DEVICE:
            continue
        assert not [line for line in text.splitlines() if draw.search(line)], path
        if path.split(os.sep)[0] in EXTENSIONS:
            assert "fmod(" not in text, path
            assert not re.search(r"#define WF_\w+_TILE\b", text), path  # (the tile size: WF_ENSEMBLE_TILE)


def test_one_pin_macro():
    src = _sources()
    defined = [path for path, text in src.items() if re.search(r"#define WF_\w*IN_VGPR", text)]
    assert defined == [os.path.join("ext", "wf_ext_kernels.h")], defined


def test_the_host_checks_are_defined_once():
    src = _sources()
    assert '"tail must be in 1..M' in src[HOST]
    for path, text in src.items():
        if path.endswith("_abi.hip"):
            assert "tail must be in 1..M" not in text, path
        if path != os.path.join("ext", "wf_ext.h"):
            assert not re.search(r"\bbool (in_unit|non_negative)\(", text), path
        if path != os.path.join("ext", "wf_ext.h"):
            assert "env.yaw = h->d_env_yaw" not in text, path
    for ext in EXTENSIONS:
        text = src[os.path.join(ext, "wf_%s_abi.hip" % ext)]
        assert "check_ensemble" in text and "check_ensemble_anchor(" in text and "ensemble_args(" in text, ext


def test_the_python_argument_handling_is_defined_once():
    text = open(os.path.join(ROOT, "wfcrl-env_amd", "backend.py")).read()
    assert text.count("unknown wind process parameter") == 1  # (generate_wind shares the ensemble's helper)
    assert text.count("needs a wind process") == 1
    assert text.count("anchor must be") + text.count('"anchor", "(n_farms, 2)') == 1
    assert text.count('("ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp")') == 1
