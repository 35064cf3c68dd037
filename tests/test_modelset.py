"""CPU: wake-model parameter sets per farm (include/wfmodelset.h) — the binding table against the header, the Python
validation that needs no device, and the resource limits of the two new translation units.  The HIP side of it:
tests/test_modelset_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "wfmodelset.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wf_[a-z_]+)\s*\(", text)))


def test_binding_table_is_the_headers_surface():
    from wfcrl_env_amd import _lib

    syms = declared_symbols()
    assert {"wf_set_model_sets", "wf_get_model_sets", "wf_model_set_from_model"} <= set(syms)
    assert set(_lib.MODELSET_ABI) == set(syms)
    lib = _lib.load()
    for s in syms:
        assert hasattr(lib, s), f"libwfstep.so does not export {s}"
    assert not set(_lib.MODELSET_ABI) & set(_lib.ABI)  # include/wfstep.h's table stays its own
    # the struct mirrors the header's field list, in order
    text = open(os.path.join(ROOT, "include", "wfmodelset.h")).read()
    body = re.search(r"typedef struct wf_model_set \{(.*?)\} wf_model_set;", text, flags=re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", body.replace("double", ""))) == _lib._MODEL_SET_FIELDS
    assert len(_lib._MODEL_SET_FIELDS) == 18 and set(_lib._MODEL_SET_FIELDS) <= set(_lib._MODEL_DOUBLES)


def test_python_validation_needs_no_device():
    from wfcrl_env_amd import _lib
    from wfcrl_env_amd.backend import default_model, normalize_model_sets
    from wfcrl_env_amd.vec_env import VecWindFarmEnv

    base = default_model()
    cols, S = normalize_model_sets([{"ambient_ti": 0.04}, {"ka": 0.3, "veer": 2.0}, {}], base)
    assert S == 3 and set(cols) == set(_lib._MODEL_SET_FIELDS)
    assert list(cols["ambient_ti"]) == [0.04, base["ambient_ti"], base["ambient_ti"]] and list(cols["ka"]) == [base["ka"], 0.3, base["ka"]]
    assert list(cols["veer"]) == [0.0, 2.0, 0.0] and (cols["defl_ka"] == base["defl_ka"]).all()
    cols, S = normalize_model_sets({"shear": np.array([0.1, 0.2])}, base)
    assert S == 2 and list(cols["shear"]) == [0.1, 0.2] and list(cols["beta"]) == [base["beta"]] * 2
    with pytest.raises(ValueError, match=r"unknown model-set field\(s\): \['hub_height'\]"):
        normalize_model_sets([{"hub_height": 100.0}], base)
    with pytest.raises(ValueError, match=r"unknown model-set field\(s\): \['tsr'\]"):
        normalize_model_sets({"tsr": [8.0]}, base)
    with pytest.raises(ValueError, match="same length"):
        normalize_model_sets({"ka": [0.3, 0.4], "kb": [0.004]}, base)
    with pytest.raises(ValueError, match="kb is not finite"):
        normalize_model_sets([{"kb": float("inf")}], base)
    with pytest.raises(ValueError, match="ambient_ti must be > 0"):
        normalize_model_sets({"ambient_ti": [0.06, -0.01]}, base)
    chk = VecWindFarmEnv._check_model_randomization
    mr = chk(dict(ranges={"ka": (0.27, 0.49)}), 1000)
    assert mr["n_sets"] == 256 and mr["resample"] == "reset" and mr["ranges"] == {"ka": (0.27, 0.49)}
    assert chk(dict(ranges={"ka": (0.3, 0.4)}, n_sets=3, resample="once"), 8)["n_sets"] == 3
    assert chk(dict(sets=[{}]), 4)["set_of"] is None
    for bad, msg in ((dict(ranges={"air_density": (1.0, 1.2)}), r"unknown model-set field\(s\): \['air_density'\]"),
                     (dict(ranges={"ka": (0.5, 0.3)}), "lo <= hi"), (dict(ranges={"ka": (0.3, 0.4)}, n_sets=9), "1..env_batch"),
                     (dict(ranges={"ka": (0.3, 0.4)}, resample="step"), "'reset' or 'once'"), (dict(n_sets=2), "give ranges"),
                     (dict(sets=[{}], ranges={}), "either")):
        with pytest.raises(ValueError, match=msg):
            chk(bad, 8)


def test_new_float64_units_have_no_private_segment(tmp_path):
    """tests/test_abi.py::test_float64_kernels_have_no_private_segment for the units of wake-model parameter sets: compiled
    with the Makefile's flags, their kernels hold no private segment, spill no vector register and call nothing out of line;
    the four-wave unit keeps 128 VGPRs, no spilled scalar register and the static LDS of wf_resolve4_mt.hip."""
    src = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
    flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only"]
    nolicm = ["-mllvm", "-disable-machine-licm"]
    for unit, extra in (("wf_resolve_ms.hip", []), ("wf_resolve4_ms.hip", nolicm)):
        out = tmp_path / (unit + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra + ["-o", str(out), os.path.join(src, unit)], check=True, capture_output=True)
        text = out.read_text()
        kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)
        seen = {n: (int(p), int(v)) for n, p, v in kernels if "wf_resolve" in n}
        assert len(seen) == 1 and "_ms_kernel" in next(iter(seen)), seen
        for name, (private, spills) in seen.items():
            assert private == 0 and spills == 0, (name, private, spills)
        assert "s_swappc_b64" not in text  # no out-of-line call anywhere in the file
        if unit == "wf_resolve4_ms.hip":
            m = re.search(r"\.group_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.name:\s+\S*wf_resolve4\S*\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
            assert m, "kernel metadata of wf_resolve4_ms_kernel not found"
            lds_static, sgpr_spills, vgprs = (int(v) for v in m.groups())
            assert vgprs <= 128 and sgpr_spills == 0, (vgprs, sgpr_spills)
            assert lds_static <= 29888, lds_static  # (the several-definitions unit's footprint: four tables; the sets add nothing)
    mk = open(os.path.join(src, "Makefile")).read()
    assert "$(SETRES) -c -o $@ wf_resolve4_ms.hip" in mk and "$(FLAGS) -c -o $@ wf_resolve_ms.hip" in mk  # (what this test compiled is what ships)
