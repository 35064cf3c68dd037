"""TEST INFRASTRUCTURE — the synthetic wind process (include/wfwindgen.h: DEFINITION; csrc/windgen/wf_windgen_kernels.hip)
restated in NumPy on plan_ref (Philox, the deviate) and wind_ref (tick 0, u01), line by line: every tick of every farm is
predicted, not just its distribution.  float64 throughout; every product and sum is one rounding, in the header's order.

  tick 0      (S0, D0) = wind_ref.sample(seed, B, dist), or the caller's: S0 = ws0, D0 = fmod(wd0, 360), + 360 if negative
  ramp        rate = wd_ramp (2 u01(r[0], r[1]) - 1), r = philox(seed, counter b, stream 3)
  deviate     z(b, u, stream) = plan_ref.deviate(seed, farm b, index u, stream)
  tick u >= 1 x_u = (x_{u-1} + ws_revert (S0 - x_{u-1})) + ws_sigma z(b, u, 4)
              m_u = D0 + rate u
              y_u = (y_{u-1} + wd_revert (m_u - y_{u-1})) + wd_sigma z(b, u, 5)
              speed_u = clip(x_u, ws_lo, ws_hi);  direction_u = fmod(y_u, 360), + 360 if negative
The latent (x, y) is neither clipped nor wrapped; dist's wd_lo / wd_hi act at tick 0 only.

The cases and what each is aimed at (tests/test_windgen.py asserts these properties on the reference alone;
tests/test_windgen_gpu.py compares the device with it)."""
import numpy as np

import plan_ref
import wind_ref

B_CASES = 259  # two blocks of the device kernel's launch whatever its block size up to 256, the last with 3 threads
T_CASES = 37
KEYS = ("ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp")


def process_of(values):
    """dict of the five process parameters from a tuple in KEYS' order (or a dict: missing parameters 0)."""
    if isinstance(values, dict):
        return {k: float(values.get(k, 0.0)) for k in KEYS}
    return dict(zip(KEYS, (float(v) for v in values)))


# name -> (seed, distribution overrides, process); seeds and distributions are wind_ref.CASES' unless stated
CASES = {
    "default": (wind_ref.CASES["default"][0], wind_ref.CASES["default"][1], process_of((0.05, 0.25, 0.05, 1.5, 0.0))),
    # no reversion of the speed under a large sigma: many stored speeds on either bound; directions leave [wd_lo, wd_hi]
    "clip": (wind_ref.CASES["clip"][0], wind_ref.CASES["clip"][1], process_of((0.0, 1.0, 0.2, 4.0, 0.0))),
    # directions around 359: the latent crosses 0 and 360 both ways
    "wrap": (wind_ref.CASES["wrap"][0], wind_ref.CASES["wrap"][1], process_of((0.1, 0.3, 0.1, 2.0, 0.0))),
    # a ramp of up to 25 degrees per tick followed tightly: latents more than a turn below 0 and above 360
    "ramp": (99, dict(wd_mean=10.0, wd_std=5.0), process_of((0.1, 0.1, 1.0, 0.5, 25.0))),
    "frozen": (wind_ref.CASES["default"][0], wind_ref.CASES["default"][1], process_of((0.0, 0.0, 0.0, 0.0, 0.0))),
}


def wrap360(wd):
    w = np.fmod(np.asarray(wd, np.float64), 360.0)
    return np.where(w < 0.0, w + 360.0, w)


def ramp_rate(seed, B, wd_ramp):
    r = plan_ref.philox4x32_10(seed, np.arange(B, dtype=np.uint64), 3)
    return float(wd_ramp) * (2.0 * wind_ref.u01(r[:, 0], r[:, 1]) - 1.0)


def generate(seed, B, T, process, dist=None, tick0=None):
    """The series of farms 0 .. B - 1: dict(ws, wd — (T, B), what the kernel stores —, x, y — (T, B), the latents —, rate (B,)).
    tick0 = (ws0, wd0), (B,) each: tick 0 given instead of drawn."""
    p = process_of(process)
    d = wind_ref.dist_of(dist or {})
    B, T = int(B), int(T)
    if tick0 is None:
        s = wind_ref.sample(seed, B, dist)
        S0, D0 = s["ws"], s["wd"]
    else:
        S0 = np.array(tick0[0], np.float64).reshape(B)
        D0 = wrap360(np.array(tick0[1], np.float64).reshape(B))
    rate = ramp_rate(seed, B, p["wd_ramp"])
    b = np.arange(B, dtype=np.uint64)
    x, y = np.empty((T, B)), np.empty((T, B))
    x[0], y[0] = S0, D0
    for u in range(1, T):
        zs = plan_ref.deviate(seed, b, np.full(B, u, np.uint64), 4)
        zd = plan_ref.deviate(seed, b, np.full(B, u, np.uint64), 5)
        x[u] = (x[u - 1] + p["ws_revert"] * (S0 - x[u - 1])) + p["ws_sigma"] * zs
        m = D0 + rate * float(u)
        y[u] = (y[u - 1] + p["wd_revert"] * (m - y[u - 1])) + p["wd_sigma"] * zd
    ws = np.minimum(np.maximum(x, d["ws_lo"]), d["ws_hi"])
    wd = wrap360(y)
    ws[0], wd[0] = S0, D0  # (tick 0 is stored as it is: the draw is clipped already, a caller's is the caller's)
    return {"ws": ws, "wd": wd, "x": x, "y": y, "rate": rate}


def case(name, B=B_CASES, T=T_CASES, tick0=None):
    seed, dist, process = CASES[name]
    return generate(seed, B, T, process, dist, tick0)


def rows(g, farms=None):
    """(n, T, 2) [speed, direction] of the listed farms (None: all): the layout of backend.WfStep.generated_wind."""
    a = np.stack([g["ws"].T, g["wd"].T], axis=-1)
    return a if farms is None else a[np.asarray(farms, np.int64).reshape(-1)]


def window(g, t, first, H, farms=None):
    """((n, H, 2), available): include/wfseries.h's window at cursor t, every farm on its own rows."""
    import series_ref

    T = g["ws"].shape[0]
    return rows(g, farms)[:, series_ref.ticks(T, t, first, H)], series_ref.available(T, t, first, H)
