"""On an MI355X: cost of wake-model parameter sets per farm (every farm solved by the float64 kernels of wf_resolve_ms.hip /
wf_resolve4_ms.hip, its constants copied from a table per farm) beside the SAME handle in plain mode 2 without sets.

HornsRev1 x 4096 and Ablaincourt x 4096, a wind per farm, 16 sets.  Stream events around a window of steps (wf_timing_*), both
sides warmed up, five repeats alternating the two sides in one process.  Writes profiles/modelset_timing.json (or the path
given as the first argument): per shape the five per-step times of each side, their medians, the ratio of the medians and the
run-to-run spread (max - min) / median of each side.  A third side — the several-definitions kernels with the model as the
one definition and no sets — says how much of the difference is the build the new units stand on.
Run from the repo root:  python tools/modelset_timing.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/modelset_timing.json"
L = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
B, S, REPEATS = 4096, 16, 5
record = {"farms": B, "sets": S, "wind": "one per farm", "repeats": REPEATS, "timer": "stream events around a window of steps (wf_timing_begin / wf_timing_end)",
          "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, steps in (("HornsRev1_", 40), ("Ablaincourt_", 200)):
    l = L[name]
    N = l["num_turbines"]
    rng = np.random.default_rng(7)
    ws, wd = np.clip(8 * rng.weibull(8, B), 3, 28), rng.normal(270, 20, B) % 360
    sets = {"ambient_ti": rng.uniform(0.04, 0.12, S), "ka": rng.uniform(0.27, 0.49, S), "shear": rng.uniform(0.08, 0.2, S),
            "ch_constant": rng.uniform(0.42, 0.62, S)}
    set_of = rng.integers(0, S, B).astype(np.int32)
    g = torch.Generator(device="cuda").manual_seed(1)
    yaw = (torch.rand((B, N), device="cuda", generator=g) * 60 - 30).float()
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B)
    w.set_risk_resolve(2)
    w.set_wind(ws, wd)
    out = w.step(yaw)

    # a third side, for attribution: the several-definitions kernels the new units are built on, with the model as the one
    # definition and no sets (a handle of its own: definitions are part of the model)
    w1 = WfStep(l["xcoords"], l["ycoords"], env_batch=B, model=dict(turbine_defs=[{}], turbine_type_of=[0] * N))
    w1.set_wind(ws, wd)
    out1 = w1.step(yaw)

    def window(h=None, o=None):
        h, o = (w, out) if h is None else (h, o)
        for _ in range(3):
            h.step(yaw, o)
        h.sync()
        h.timing_begin()
        for _ in range(steps):
            h.step(yaw, o)
        return h.timing_end() / steps

    times = {"mode2": [], "sets": [], "one_definition_no_sets": []}
    waves = None
    for _ in range(REPEATS):
        w.clear_model_sets()
        times["mode2"].append(window())
        w.set_model_sets(sets, set_of)
        times["sets"].append(window())
        waves = w.model_sets_kernel()
        times["one_definition_no_sets"].append(window(w1, out1))
    w.close()
    w1.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    row = {"turbines": N, "steps_per_window": steps, "waves_per_farm_with_sets": waves,
           "ms_per_step": {k: [round(float(x), 5) for x in v] for k, v in times.items()},
           "median_ms": {k: round(v, 5) for k, v in med.items()},
           "ratio_sets_over_mode2": round(med["sets"] / med["mode2"], 4),
           "ratio_sets_over_one_definition": round(med["sets"] / med["one_definition_no_sets"], 4),
           "spread": {k: round(float((max(v) - min(v)) / med[k]), 4) for k, v in times.items()},
           "farm_steps_per_s_with_sets": round(B / med["sets"] * 1e3)}
    record["shapes"][name.rstrip("_") + f" x {B}"] = row
    print(name, json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
json.dump(record, open(OUT, "w"), indent=1)
