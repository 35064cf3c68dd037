"""Test-only stand-ins.  `OracleStep` has the call surface of wfcrl_env_amd.backend.WfStep but evaluates
the float64 C oracle on the CPU, so the host-side env surface (interface, mdp, envs, wrappers, registry)
can be exercised in the CPU suite.  It lives under tests/ — the product has no CPU path."""
import ctypes
import os

import numpy as np

from oracle import c_oracle
from wfcrl_env_amd.interface import HipFlorisInterface

# the test hook of csrc/wf_f64_math.h (csrc/check/wf_math_check.hip), built next to libwfstep.so by csrc/Makefile
WFCHECK_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wfcrl-env_amd", "libwfcheck.so")


def load_wfcheck():
    """libwfcheck.so with the signature of its one launcher; a missing library raises."""
    from wfcrl_env_amd import _lib

    _lib._share_hip_runtime_with_torch()  # (torch first: one HIP runtime in the process, as for libwfstep.so)
    lib = ctypes.CDLL(WFCHECK_PATH)
    lib.wf_math_check.restype = ctypes.c_int
    lib.wf_math_check.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_longlong, ctypes.c_void_p]
    return lib


def math_check(lib, fn, *args, n_out=1):
    """Routine `fn` (an id of tests/f64_math_cases.py) over float64 argument arrays, on cuda:0 on torch's current stream:
    a tuple of n_out float64 NumPy arrays."""
    import torch

    ins = [torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda() for a in args]
    outs = [torch.full_like(ins[0], float("nan")) for _ in range(n_out)]
    rc = lib.wf_math_check(int(fn), ins[0].data_ptr(), ins[1].data_ptr() if len(ins) > 1 else None, outs[0].data_ptr(),
                           outs[1].data_ptr() if n_out > 1 else None, ins[0].numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"wf_math_check({fn}) returned {rc}"
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


class OracleStep:
    def __init__(self, xcoords, ycoords, env_batch=1, device_id=0, model=None):
        self.x, self.y = np.asarray(xcoords, float), np.asarray(ycoords, float)
        self.num_turbines, self.env_batch = len(self.x), env_batch
        self.ws = self.wd = None
        self.calls = 0
        self.wind_sets = 0

    def set_wind(self, ws, wd):
        self.ws, self.wd = np.atleast_1d(np.asarray(ws, float)), np.atleast_1d(np.asarray(wd, float))
        self.wind_sets += 1

    def step(self, yaw, out=None):
        self.calls += 1
        yaw = np.asarray(yaw, np.float32).reshape(self.env_batch, self.num_turbines).astype(np.float64)
        r = c_oracle.farm_step_batch(self.x, self.y, self.ws, self.wd, yaw, nthreads=1)
        return {k: v.astype(np.float32) for k, v in r.items()}

    def sync(self):
        pass

    def close(self):
        pass


class OracleFlorisInterface(HipFlorisInterface):
    def _make_backend(self, xcoords, ycoords, device_id, model):
        return OracleStep(xcoords, ycoords)


class OracleStep64(OracleStep):
    """The same stand-in handing back float64 (no float32 device surface in between): what the reference's
    FLORIS object hands its interface.  Used where host-side arithmetic is compared at 1e-12."""

    def step(self, yaw, out=None):
        self.calls += 1
        yaw = np.asarray(yaw, np.float32).reshape(self.env_batch, self.num_turbines).astype(np.float64)
        return dict(c_oracle.farm_step_batch(self.x, self.y, self.ws, self.wd, yaw, nthreads=1))


class OracleFlorisInterface64(HipFlorisInterface):
    def _make_backend(self, xcoords, ycoords, device_id, model):
        return OracleStep64(xcoords, ycoords)
