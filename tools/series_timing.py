"""Time-series episodes (csrc/series/, include/wfseries.h): what planning and look-ahead under the series' coming rows cost
with wind="series" — the window read on the device by one kernel — next to the way a caller had to do it before: the rows
gathered on the host from the start rows and the tick count, uploaded, and passed as wind=.  Writes
profiles/series_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env in series mode (64 rows, a start row per farm,
env_config, env_reset, three ticks with random env steps), continuous control, gamma 0.95, default mode, the default widths
(1, 1/2, 1/4) yaw_step, E = K / 4 elites:
    HornsRev1 x 256 farms, K = 32, H = 8, I = 3
    Ablaincourt x 4096 farms, K = 16, H = 4, I = 3
Per configuration, after 2 warm-up rounds, `reps` rounds (at least 5) in which the variants alternate; per variant the median,
the smallest and the largest, and spread = largest - smallest:
    plan_host_rows_ms / lookahead_host_rows_ms   between two events: the NumPy gather of (n_farms, H, 2) rows, the upload,
                   plan_actions(wind=rows) / lookahead_returns(wind=rows) — the host time lies between the events too
    plan_series_ms / lookahead_series_ms         the same calls with wind="series" (a library that has the series extension)
    plan_held_ms / lookahead_held_ms             wind=None on a handle that is NOT in series mode (a wind per farm): the path
                   the extension must leave as it was
    window_us      wind_preview(H) into a preallocated tensor alone: 20 launches between two events, per launch
The tool runs on a checkout WITHOUT the series extension as well (it then measures the host-rows and held variants only):
that is how the baseline of the commit before is taken; pass its output as the third argument and the result holds both
and the comparison the extension is accepted by — the series call no slower than the baseline's host-rows call beyond the
baseline's own spread, the held calls within that spread of the baseline's.
Run from the repo root on an MI355X:  python tools/series_timing.py [reps, default 9] [output file] [baseline json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "series_timing.json")
BASELINE = sys.argv[3] if len(sys.argv) > 3 else None
HAS_SERIES = hasattr(WfStep, "wind_preview")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA, SIGMA, T, TICKS = 0.95, (5.0, 2.5, 1.25), 64, 3


def timed(fn):
    """ms between two events around fn(), host time included; the stream is idle when the first is recorded."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "spread": float(np.max(v) - np.min(v))}


def workload(label, name, B, K, H):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N, E = len(x), K // 4
    rng = np.random.default_rng(7)
    series = np.stack([rng.uniform(6.0, 12.0, T), rng.uniform(0.0, 360.0, T)], axis=1)
    start = rng.integers(0, T, B).astype(np.int32)

    def steps(w):
        w.env_config(**ENV)
        w.env_reset()
        for _ in range(TICKS):
            if w is ws:
                w.wind_series_step()
            w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))

    ws = WfStep(x, y, env_batch=B)  # in series mode
    ws.set_wind_series(series, start=start)
    steps(ws)
    wn = WfStep(x, y, env_batch=B)  # a wind per farm, held
    wn.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    steps(wn)
    act = torch.from_numpy(rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)).cuda()
    pout = {"first_action": torch.empty((B, N), dtype=torch.float32, device="cuda"), "plan_return": torch.empty(B, dtype=torch.float64, device="cuda")}
    lout = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda"), "best": torch.empty(B, dtype=torch.int32, device="cuda")}
    pkw = dict(candidates=K, elites=E, sigma=SIGMA, seed=7, gamma=GAMMA, want=tuple(pout), out=pout)
    lkw = dict(gamma=GAMMA, want=tuple(lout), out=lout)

    def rows():  # what a caller had to do: the coming rows from the start rows and the tick count, on the host, then the upload
        u = np.minimum(TICKS + 1 + np.arange(H), T - 1)
        return torch.from_numpy(series[(start[:, None] + u[None, :]) % T]).cuda()

    run = {"plan_host_rows": lambda: ws.plan_actions(H, wind=rows(), **pkw),
           "lookahead_host_rows": lambda: ws.lookahead_returns(act, wind=rows(), **lkw),
           "plan_held": lambda: wn.plan_actions(H, **pkw),
           "lookahead_held": lambda: wn.lookahead_returns(act, **lkw)}
    if HAS_SERIES:
        run["plan_series"] = lambda: ws.plan_actions(H, wind="series", **pkw)
        run["lookahead_series"] = lambda: ws.lookahead_returns(act, wind="series", **lkw)
    ms = {k: [] for k in run}
    for r in range(2 + REPS):  # (alternating: the variants share whatever else the machine is doing)
        for k, fn in run.items():
            v = timed(fn)
            if r >= 2:
                ms[k].append(v)
    res = {"workload": label, "layout": name, "turbines": N, "farms": B, "candidates": K, "elites": E, "horizon": H,
           "iterations": len(SIGMA), "series_rows": T, "reps": REPS, **{k + "_ms": stats(v) for k, v in ms.items()}}
    if HAS_SERIES:
        same = ws.plan_actions(H, wind="series", **dict(pkw, out=None))
        want = ws.plan_actions(H, wind=rows(), **dict(pkw, out=None))
        res["series_equals_host_rows"] = bool(all(np.array_equal(np.asarray(same[k]), want[k].cpu().numpy()) for k in same))
        buf = torch.empty((B, H, 2), dtype=torch.float64, device="cuda")
        win = []
        for r in range(2 + REPS):
            v = timed(lambda: [ws.wind_preview(H, out=buf) for _ in range(20)]) / 20.0 * 1e3
            if r >= 2:
                win.append(v)
        res["window_us"] = stats(win)
        res["kernels"] = ws.series_kernel_info()
    ws.close()
    wn.close()
    print(json.dumps(res), flush=True)
    return res


def compare(res, base):
    """Per workload and call: the figures the extension is accepted by, from this run and the baseline's."""
    out = []
    for r, b in zip(res, base):
        assert r["workload"] == b["workload"]
        c = {"workload": r["workload"]}
        for call in ("plan", "lookahead"):
            host, held = b[call + "_host_rows_ms"], b[call + "_held_ms"]
            if call + "_series_ms" in r:
                s = r[call + "_series_ms"]["median"]
                c[call + "_series_vs_baseline_host_rows"] = {"series_ms": s, "baseline_ms": host["median"], "baseline_spread_ms": host["spread"],
                                                             "no_slower_beyond_spread": bool(s <= host["median"] + host["spread"])}
            h = r[call + "_held_ms"]["median"]
            c[call + "_held_vs_baseline"] = {"held_ms": h, "baseline_ms": held["median"], "baseline_spread_ms": held["spread"],
                                             "within_spread": bool(abs(h - held["median"]) <= held["spread"])}
        out.append(c)
    return out


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 32, H = 8, I = 3, default mode", "HornsRev1_", 256, 32, 8),
           workload("Ablaincourt x 4096, K = 16, H = 4, I = 3, default mode", "Ablaincourt_", 4096, 16, 4)]
    doc = {"device": torch.cuda.get_device_name(0), "series_extension": HAS_SERIES,
           "method": "HIP events around each call, host work included; 2 warm-up rounds, `reps` rounds with the variants alternating; "
                     "median, min, max, spread = max - min", "workloads": res}
    if BASELINE:
        base = json.load(open(BASELINE))
        doc["baseline"] = {"what": "the same tool on the commit before the series extension", "workloads": base["workloads"]}
        doc["comparison"] = compare(res, base["workloads"])
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
