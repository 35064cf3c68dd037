"""TEST INFRASTRUCTURE — the on-device wind process (csrc/wf_kernels.hip: wf_wind_sample_kernel, wf_wind_sample_binned_kernel,
wf_series_start_kernel, on csrc/wf_philox.h) restated in NumPy on top of plan_ref.philox4x32_10, line by line: every draw of
every farm is predicted, not just its distribution.

  u01(hi, lo)   (((hi << 32 | lo) >> 11) + 0.5) 2^-53: 53 bits, in (0, 1)
  farm b        r0 = philox(seed, counter b, stream 0), r1 = philox(seed, counter b, stream 1)
  speed         clip(scale (-log u01(r0[0], r0[1]))^(1 / shape), lo, hi)
  direction     mean + std sqrt(-2 log u01(r0[2], r0[3])) cos(2 pi u01(r1[0], r1[1])) (Box-Muller), fmod(., 360), + 360 if
                negative, clip(lo, hi)
  binned        bin = rint(direction / step) mod K, K = 360 / step (360 -> bin 0); direction = bin step
  series start  (philox(seed, b, stream 2)[0] * T) >> 32

The cases and what each is aimed at (tests/test_wind_process.py asserts these properties on the reference alone;
tests/test_wind_process_gpu.py compares the device with it)."""
import numpy as np

import plan_ref

DEFAULT = dict(ws_scale=8.0, ws_shape=8.0, ws_lo=3.0, ws_hi=28.0, wd_mean=270.0, wd_std=20.0, wd_lo=0.0, wd_hi=360.0)

B_CASES = 4099  # 17 blocks of 256, the last one with 3 threads

# name -> (seed, distribution overrides, direction step of the binned run)
CASES = {
    "default": (1234, {}, 5.0),
    "wrap": ((0xC0FFEE << 32) | 7, dict(wd_mean=359.0, wd_std=3.0), 2.0),  # a seed with bits above 31; directions across 360
    "clip": (2 ** 63 + 5, dict(ws_scale=10.0, ws_shape=2.0, ws_lo=6.0, ws_hi=14.0, wd_mean=180.0, wd_std=60.0, wd_lo=100.0,
                              wd_hi=260.0), 10.0),  # the top bit of the seed; many draws on every clip bound
    "neg": (99, dict(wd_mean=-725.0, wd_std=40.0), 45.0),  # every raw direction negative: fmod's sign, then + 360
}


def dist_of(overrides):
    d = dict(DEFAULT)
    d.update(overrides)
    return d


def u01(hi, lo):
    v = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)
    return (v.astype(np.float64) + 0.5) * 2.0 ** -53


def sample(seed, B, dist=None):
    """The draws of farms 0 .. B - 1: dict(ws, wd — what the kernel stores —, ws_raw before the clip, wd_raw before fmod,
    wd_wrapped before the clip)."""
    d = dist_of(dist or {})
    b = np.arange(B, dtype=np.uint64)
    r0, r1 = plan_ref.philox4x32_10(seed, b, 0), plan_ref.philox4x32_10(seed, b, 1)
    e = -np.log(u01(r0[:, 0], r0[:, 1]))
    ws_raw = d["ws_scale"] * np.power(e, 1.0 / d["ws_shape"])
    ws = np.minimum(np.maximum(ws_raw, d["ws_lo"]), d["ws_hi"])
    rad = np.sqrt(-2.0 * np.log(u01(r0[:, 2], r0[:, 3])))
    wd_raw = d["wd_mean"] + d["wd_std"] * rad * np.cos(2.0 * np.pi * u01(r1[:, 0], r1[:, 1]))
    w = np.fmod(wd_raw, 360.0)
    w = np.where(w < 0.0, w + 360.0, w)
    wd = np.minimum(np.maximum(w, d["wd_lo"]), d["wd_hi"])
    return {"ws": ws, "wd": wd, "ws_raw": ws_raw, "wd_raw": wd_raw, "wd_wrapped": w}


def binned(seed, B, dist, step):
    """The binned run: dict(ws, wd = bin * step, bin, K, q = direction / step before rounding, folded — rint(q) == K —)
    plus sample()'s fields under "raw"."""
    s = sample(seed, B, dist)
    K = int(round(360.0 / step))
    q = s["wd"] / step
    k = np.rint(q).astype(np.int64)
    return {"ws": s["ws"], "wd": (k % K) * step, "bin": (k % K).astype(np.int32), "K": K, "q": q, "folded": k == K, "raw": s}


def tie_margin(q):
    """The smallest | frac(q) - 1/2 |: how far the nearest draw is from changing its bin."""
    return float(np.abs(np.abs(q - np.floor(q)) - 0.5).min())


def wrap_margin(wd_raw):
    """The smallest distance (degrees) of a raw direction from a multiple of 360: how far the nearest draw is from wrapping
    differently."""
    t = wd_raw / 360.0
    return float((np.abs(t - np.rint(t)) * 360.0).min())


def series_start(seed, B, T):
    """(B,) int32 start rows of a T-row series."""
    r = plan_ref.philox4x32_10(seed, np.arange(B, dtype=np.uint64), 2)[:, 0].astype(np.uint64)
    return ((r * np.uint64(T)) >> np.uint64(32)).astype(np.int32)
