"""Expected power over a wind rose on the device (csrc/rose/, include/wfrose.h): what an evaluation costs, against the same
evaluation written with the API the project had before.  Writes profiles/rose_timing.json.

Workloads, one MI355X, default (non-strict) mode, a 72-direction x 22-speed rose (0, 5, .. 355 deg x 4 .. 25 m/s):
  HornsRev1 (80 turbines), 2 cases (zero yaw and a yaw table)        3 168 rows
  Ablaincourt (7 turbines), 8 cases (zero, a table, 6 fixed rows)    12 672 rows
Per workload, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
  total_ms / step_ms / glue_ms   median of `reps` runs of WfStep.expected_power with torch outputs — HIP events on the handle's
             stream (wf_rose_last_timing): first to last launch; the evaluator's wf_set_wind_counts + wf_step; the lay-out and
             reducing kernels
  wall_ms    the same calls between two torch events around the Python call (the host's share included)
  loop_ms    THE BASELINE: a Python loop over the 72 directions of set_wind(speeds per row, ONE direction) + step + a torch
             float64 sum, on a handle of cases x speeds farms — the shared-geometry, pair-table path the direction-loop
             driver of the issue would take.  Its yaw rows (the table looked up per condition) are prepared BEFORE the
             clock starts, which favours the loop.  Runs of the two alternate; ratio = total_ms / loop_ms.
  agreement  largest relative distance between the two results' condition powers (both default mode)
Run from the repo root on an MI355X:  python tools/rose_timing.py [reps, default 10] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rose_ref  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rose_timing.json")
WD = np.arange(0.0, 360.0, 5.0)
WS = np.arange(4.0, 26.0, 1.0)
TAB_WD, TAB_WS = np.arange(0.0, 360.0, 10.0), np.array([4.0, 7.0, 10.0, 13.0])


def loop_baseline(w2, ws_t, wd_t, yaw_t, freq_t, C, S):
    """The evaluation with set_wind + step + torch sums: returns (weighted (C,), condition (C, D, S))."""
    D = wd_t.numel()
    cond = torch.empty((C, D, S), dtype=torch.float64, device="cuda")
    for d in range(D):
        w2.set_wind(ws_t, wd_t[d:d + 1])
        p = w2.step(yaw_t[d])["power"]
        cond[:, d, :] = p.double().sum(dim=1).view(C, S)
    return (cond * freq_t[None]).sum(dim=(1, 2)), cond


def workload(label, name, n_cases):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N, D, S, C = len(x), WD.size, WS.size, n_cases
    rng = np.random.default_rng(7)
    freq = rng.uniform(0.0, 1.0, (D, S))
    freq /= freq.sum()
    table = rng.uniform(-25.0, 25.0, (TAB_WD.size, TAB_WS.size, N)).astype(np.float32)
    fixed = [rng.uniform(-25.0, 25.0, N).astype(np.float32) for _ in range(C - 2)]
    cases = ("zero", ("table", 0)) + tuple(fixed)
    w = WfStep(x, y, env_batch=1)
    w.set_yaw_table(table, TAB_WD, TAB_WS, "linear")
    out = {"weighted_power": torch.empty(C, dtype=torch.float64, device="cuda"),
           "weighted_turbine_power": torch.empty((C, N), dtype=torch.float64, device="cuda"),
           "condition_power": torch.empty((C, D, S), dtype=torch.float32, device="cuda")}
    # the baseline's handle and inputs: rows (case, speed) per direction, the yaw of every row prepared on the host
    w2 = WfStep(x, y, env_batch=C * S)
    yaw = np.stack([rose_ref.case_yaw(c, WD, WS, N, {0: (table, TAB_WD, TAB_WS, "linear")}) for c in cases])  # (C, D, S, N)
    yaw_t = torch.as_tensor(np.ascontiguousarray(yaw.transpose(1, 0, 2, 3).reshape(D, C * S, N)), device="cuda")
    ws_t = torch.as_tensor(np.tile(WS, C), device="cuda")
    wd_t, freq_t = torch.as_tensor(WD, device="cuda"), torch.as_tensor(freq, device="cuda")

    def ours():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = w.expected_power(WD, WS, freq, cases, out=out)
        b.record()
        b.synchronize()
        return r, a.elapsed_time(b), w.rose_timing()

    def theirs():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = loop_baseline(w2, ws_t, wd_t, yaw_t, freq_t, C, S)
        b.record()
        b.synchronize()
        return r, a.elapsed_time(b)

    for _ in range(2):
        ours(), theirs()
    wall, dev, loop = [], [], []
    for _ in range(REPS):  # alternating: the two share whatever else the machine is doing
        r, ms, t = ours()
        wall.append(ms), dev.append(t)
        (lw, lc), ms = theirs()
        loop.append(ms)
    gap = float(((r["condition_power"].double() - lc).abs() / lc.clamp(min=1.0e3)).max().item())
    wgap = float(((r["weighted_power"] - lw).abs() / lw).max().item())
    info, kinfo = w.kernel_info(), w.rose_kernel_info()
    w.close(), w2.close()
    med = lambda k: float(np.median([d[k] for d in dev]))  # noqa: E731
    res = {"workload": label, "layout": name, "turbines": N, "directions": D, "speeds": S, "cases": C, "rows": D * C * S, "reps": REPS,
           "total_ms": med("total_ms"), "step_ms": med("step_ms"), "glue_ms": med("glue_ms"),
           "total_ms_min": float(np.min([d["total_ms"] for d in dev])), "wall_ms": float(np.median(wall)),
           "loop_ms": float(np.median(loop)), "loop_ms_min": float(np.min(loop)), "loop_farms_per_step": C * S,
           "ratio_total_over_loop": med("total_ms") / float(np.median(loop)), "ratio_wall_over_loop": float(np.median(wall) / np.median(loop)),
           "rows_per_s": D * C * S / (med("total_ms") * 1e-3),
           "agreement_condition_power": gap, "agreement_weighted_power": wgap, "rose_kernels": kinfo,
           "parent_kernel": {k: info[k] for k in ("lanes_per_env", "slots_per_lane", "pair_table", "one_block_kernel")}}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    res = [workload("HornsRev1, 72 x 22 rose, 2 cases", "HornsRev1_", 2), workload("Ablaincourt, 72 x 22 rose, 8 cases", "Ablaincourt_", 8)]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream (wf_rose_last_timing) and torch events "
                   "around the calls; 2 warm-up runs, median of `reps`; the extension and the direction loop alternate", "workloads": res}, f, indent=1)
        f.write("\n")
