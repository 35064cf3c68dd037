"""Batched yaw optimisation on the device (csrc/yawopt/, include/wfyawopt.h): what a run costs, and how far the default mode's
result lies from the strict (float64) one.  Writes profiles/yawopt_timing.json and profiles/yawopt_default_vs_strict.json.

Timing, default passes (5, 4), one MI355X, HIP events on the handle's stream:
  HornsRev1 x 1024 farms under ONE wind, HornsRev1 x 1024 farms under a wind per farm, Ablaincourt x 4096 farms under a wind
  per farm.  Per workload, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs, two events per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with an event around every launch (these runs are a little slower
               themselves — `total_detail_ms` — the events take stream time)
    plain_loop_ms   the same number of wf_step calls on the SAME evaluator handle, batch and wind with nothing between them:
               the only fair baseline; ratio = total_ms / plain_loop_ms, runs of the two alternating
    farms_per_s, farm_steps_per_s (evaluated candidate farms, the rows that pad a pass below K_max included)
Default against strict: the farms of tests/test_yawopt_gpu.py (tests/yawopt_ref.gpu_case) — the largest relative distance between
the farm power the default mode reports and the strict run's; the test asserts twice that, or 2e-4.
Run from the repo root on an MI355X:  python tools/yawopt_timing.py [reps, default 10] [output directory, default profiles]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import yawopt_ref  # noqa: E402
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT_DIR = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
PASSES = (5, 4)


def workload(label, name, B, per_farm):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    if per_farm:
        w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    else:
        w.set_wind(8.0, 263.0)
    out = {"yaw": torch.empty((B, N), dtype=torch.float32, device="cuda"), "power": torch.empty(B, dtype=torch.float32, device="cuda"),
           "power_initial": torch.empty(B, dtype=torch.float32, device="cuda")}
    n_steps = len(PASSES) * N
    rows = max(PASSES) + 1
    n_eval = min(B, 65536 // rows) * rows  # the farms of the optimiser's evaluator
    for _ in range(2):
        w.optimize_yaw(passes=PASSES, out=out)
        w.yawopt_timing()
    plain_loop_ms(w, w._yawopt(), n_steps, n_eval)
    total, plain = [], []
    for _ in range(REPS):  # alternating: the two share whatever else the machine is doing
        w.optimize_yaw(passes=PASSES, out=out)
        total.append(w.yawopt_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._yawopt(), n_steps, n_eval))
    w.yawopt_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.optimize_yaw(passes=PASSES, out=out)
        det.append(w.yawopt_timing())
    w.yawopt_timing(detail=False)
    gain = float((out["power"] / out["power_initial"]).mean().item() - 1.0)
    info = w.kernel_info()
    w.close()
    t, p = float(np.median(total)), float(np.median(plain))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "wind": "per farm" if per_farm else "shared", "passes": list(PASSES),
         "visits": n_steps, "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])),
         "step_ms": float(np.median([d["step_ms"] for d in det])), "glue_ms": float(np.median([d["glue_ms"] for d in det])),
         "farms_per_s": B / (t * 1e-3), "farm_steps_per_s": n_eval * n_steps / (t * 1e-3),
         "mean_gain_over_zero_yaw": gain, "parent_kernel": {k: info[k] for k in ("lanes_per_env", "slots_per_lane", "pair_table", "one_block_kernel")}}
    print(json.dumps(r))
    return r


def default_vs_strict():
    rows, worst = [], 0.0
    for name in ("Ablaincourt_", "Turb16_Row5_"):
        x, y, ws, wd = yawopt_ref.gpu_case(LAYOUTS, name)
        w = WfStep(x, y, env_batch=len(ws))
        w.set_wind(ws, wd)
        s, d = w.optimize_yaw(strict=True), w.optimize_yaw()
        w.close()
        gap = np.abs(d["power"] / s["power"] - 1.0)
        rows.append({"layout": name, "farms": len(ws), "seed": yawopt_ref.GPU_CASE_SEED, "max_rel_gap": float(gap.max()),
                     "farms_with_another_yaw": int((d["yaw"] != s["yaw"]).any(axis=1).sum())})
        worst = max(worst, float(gap.max()))
    return {"what": "largest relative distance between the farm power optimize_yaw reports in the default mode and in strict mode, "
                    "same farms (tests/yawopt_ref.gpu_case), default passes; measured by tools/yawopt_timing.py on one MI355X",
            "max_rel_gap": worst, "cases": rows}


if __name__ == "__main__":
    gap = default_vs_strict()
    print(json.dumps(gap))
    res = [workload("HornsRev1 x 1024, shared wind", "HornsRev1_", 1024, False),
           workload("HornsRev1 x 1024, a wind per farm", "HornsRev1_", 1024, True),
           workload("Ablaincourt x 4096, a wind per farm", "Ablaincourt_", 4096, True)]
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, "yawopt_default_vs_strict.json"), "w") as f:
        json.dump(gap, f, indent=1)
        f.write("\n")
    with open(os.path.join(OUT_DIR, "yawopt_timing.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "optimisation and plain wf_step loop alternate", "workloads": res}, f, indent=1)
        f.write("\n")
