"""Wake-model calibration on the device (csrc/calib/, include/wfcalib.h): what a fit — I iterations of the cross-entropy method
over S candidate parameter sets, each solved under C conditions — costs, next to the step calls it is made of and next to the
way a user had to write it before.  Writes profiles/calib_timing.json.

One MI355X.  Twin problems: measurements from the oracle-free device itself (WfStep(model_sets=truth)), five free fields
(ambient_ti, ka, kb, alpha, beta), E = S / 8 elites, the default widths' first I:
    HornsRev1, G = 1 problem, S = 64, C = 64, I = 4
    Ablaincourt, G = 16 problems, S = 32, C = 16, I = 4
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of calibrate_model, torch tensors in and out, two HIP events per run (first to last
               launch); wall_ms: the same calls by the host's clock, from the call to the drained stream
    step_ms / glue_ms   median of `reps` more runs with 2 I + 2 events per chunk; glue = the I + 1 launches of the one kernel
    plain_loop_ms   the same number of wf_step calls on the object's OWN evaluator handle (it holds sets: every row in float64),
               nothing between
    hand_written_ms   what a user wrote before this extension, by the host's clock: a handle of G S C farms; per iteration the
               candidates drawn on the host, set_model_sets (the host-side constants, an allocation, an upload, two stream
               drains), one step, the squares summed with torch, topk, the elites read back
    kernels    wf_calib_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/calib_timing.py [reps, default 10] [output file]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "calib_timing.json")
SIGMA = (0.25, 0.12, 0.06, 0.03)
BOUNDS = {"ambient_ti": (0.03, 0.15), "ka": (0.15, 0.6), "kb": (0.001, 0.01), "alpha": (0.3, 0.9), "beta": (0.04, 0.12)}
TRUTH = {"ambient_ti": 0.085, "ka": 0.31, "kb": 0.0055, "alpha": 0.68, "beta": 0.07}


def hand_written(h, rows_yaw, G, S, C, E, obs, scale, start, rng):
    """The same method over the API the project had before, on a handle `h` of G S C farms whose wind is the rows', under the
    rows' yaw `rows_yaw`: per iteration host draws, set_model_sets, one step, torch sums and topk, the elites read back.  Host clock, milliseconds."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    names = list(BOUNDS)
    lo, hi = np.array([BOUNDS[f][0] for f in names]), np.array([BOUNDS[f][1] for f in names])
    mu = np.tile(np.array([start[f] for f in names]), (G, 1))
    best = mu.copy()
    set_of = (np.arange(G * S * C) // C).astype(np.int32)
    for s in SIGMA:
        cand = np.clip(mu[:, None] + s * (hi - lo) * rng.standard_normal((G, S, len(names))), lo, hi)
        cand[:, 0], cand[:, 1] = best, mu
        h.set_model_sets({f: cand[..., j].reshape(-1) for j, f in enumerate(names)}, set_of)
        p = h.step(rows_yaw)["power"].double().view(G, S, C, -1)
        loss = (((p - obs[:, None]) / scale) ** 2).sum(dim=(2, 3))
        top = loss.topk(E, dim=1, largest=False).indices.cpu().numpy()
        rows = np.arange(G)[:, None]
        mu = cand[rows, top].mean(axis=1)
        best = cand[np.arange(G), top[:, 0]]
        last = loss.min(dim=1).values
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, last


def workload(label, name, G, S, C):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N, E, I = len(x), max(1, S // 8), len(SIGMA)
    rng = np.random.default_rng(7)
    ws, wd = rng.uniform(7.0, 10.5, (G, C)), 270.0 + rng.uniform(-15.0, 15.0, (G, C))
    yaw = rng.uniform(-20.0, 20.0, (G, C, N)).astype(np.float32)
    site = WfStep(x, y, env_batch=G * C, model_sets=[TRUTH], model_set_of=np.zeros(G * C, np.int32))
    site.set_wind(ws.reshape(-1), wd.reshape(-1))
    obs = torch.as_tensor(np.asarray(site.step(yaw.reshape(G * C, N))["power"], np.float64)).cuda().view(G, C, N)
    site.close()
    w = WfStep(x, y)
    scale = w.rated_power()
    start = w.model_set_from_model()
    dev = [torch.as_tensor(a).cuda() for a in (ws, wd, yaw)]
    kw = dict(candidates=S, elites=E, sigma=SIGMA, seed=7, scale=scale)
    # the hand-written way's handle: G S C farms, row (g, s, c) under condition (g, c)
    h = WfStep(x, y, env_batch=G * S * C)
    h.set_wind(np.repeat(ws[:, None], S, axis=1).reshape(-1), np.repeat(wd[:, None], S, axis=1).reshape(-1))
    rows_yaw = torch.as_tensor(np.repeat(yaw[:, None], S, axis=1).reshape(G * S * C, N)).cuda()
    per_chunk = min(G, 65536 // (S * C))
    chunks = -(-G // per_chunk)
    n_eval = per_chunk * S * C

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = w.calibrate_model(*dev, obs, BOUNDS, **kw)
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        call()
        w.calib_timing()
        plain_loop_ms(w, w._calib(), I * chunks, n_eval)
        hand_written(h, rows_yaw, G, S, C, E, obs, scale, start, rng)
    total, wall, plain, hand = [], [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        fit, ms = call()
        wall.append(ms)
        total.append(w.calib_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._calib(), I * chunks, n_eval))
        ms, r_hand = hand_written(h, rows_yaw, G, S, C, E, obs, scale, start, rng)
        hand.append(ms)
    w.calib_timing(detail=True)
    det = []
    for _ in range(REPS):
        call()
        det.append(w.calib_timing())
    w.calib_timing(detail=False)
    quality = {"median_init_loss": float(fit["init_loss"].median().item()), "median_best_loss": float(fit["best_loss"].median().item()),
               "hand_written_median_best_loss": float(r_hand.median().item()), "invalid_candidates": int(fit["n_invalid"].sum().item())}
    kernels = w.calib_kernel_info()
    w.close()
    h.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "problems": G, "candidates": S, "conditions": C, "elites": E, "iterations": I,
         "sigma": list(SIGMA), "free_fields": list(BOUNDS), "rows_per_problem": S * C, "chunks": chunks, "evaluator_farms": n_eval,
         "evaluator_steps": I * chunks, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)), "wall_ms": float(np.median(wall)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "hand_written_ms": q, "hand_written_ms_min": float(np.min(hand)), "ratio_total_over_hand_written": t / q,
         "ratio_wall_over_hand_written": float(np.median(wall)) / q,
         "farm_solves_per_s": G * S * C * I / (t * 1e-3), "quality": quality, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1, G = 1, S = 64, C = 64, I = 4", "HornsRev1_", 1, 64, 64),
           workload("Ablaincourt, G = 16, S = 32, C = 16, I = 4", "Ablaincourt_", 16, 32, 16)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream (total, step, glue, plain loop) and "
                   "the host's clock to a drained stream (wall, hand-written); 2 warm-up runs, median of `reps`; device call, plain wf_step "
                   "loop on the evaluator and the hand-written set_model_sets way alternate", "workloads": res}, f, indent=1)
        f.write("\n")
