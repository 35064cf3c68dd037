"""TEST INFRASTRUCTURE — what the CPU tests of the extensions (test_yawopt.py, test_rose.py, test_robust.py, test_grad.py)
share: the functions a public header declares, and the metadata of one extension's kernels compiled the way the Makefile
compiles them.  No GPU."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "wfcrl-env_amd", "csrc")
METADATA = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "group_segment_fixed_size")


def declared(header):
    """The wf_* functions include/<header> declares (comments left out), sorted."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wf_[a-z0-9_]+)\s*\(", text)))


def makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def compile_kernels(hip, tmp_path):
    """`hip` (a path under csrc/) compiled for the device with the Makefile's FLAGS: ({kernel's mangled name: its METADATA},
    the assembly listing).  A file without kernels gives no entries."""
    flags = re.search(r"^FLAGS \?= (.*)$", makefile(), flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = tmp_path / (os.path.basename(hip)[:-len(".hip")] + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, hip)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    if "amdhsa.kernels:" in text:
        for block in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            seen[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in METADATA}
    return seen, text


def assert_no_private_segment(seen, kernels):
    """`seen` holds exactly `kernels`, none with a private segment or a spilled register."""
    assert len(seen) == len(kernels) and all(any(k in n for n in seen) for k in kernels), seen
    for name, m in seen.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
