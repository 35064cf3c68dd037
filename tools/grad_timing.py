"""Yaw sensitivities on the device (csrc/grad/, include/wfgrad.h): what one gradient of every farm costs, next to the step
calls it is made of and next to the Python loop a user had to write before.  Writes profiles/grad_timing.json.

One MI355X, HIP events on the handle's stream, default mode, step 1 deg, bounds (-45, 45), a random cotangent, yaw uniform
in [-20, 20]: HornsRev1 x 256 farms and Ablaincourt x 4096 farms, a wind per farm.  Per workload, after 2 warm-up runs (the
first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of yaw_gradient(yaw, c) — power and gradient, torch tensors in and out —, two events per
               run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with four events per chunk (these runs are a little slower themselves —
               `total_detail_ms`); glue = lay-out + reduce kernels
    jacobian_total_ms   the same run with the (farms, N, N) float64 Jacobian written as well
    plain_loop_ms   the same number of wf_step calls on the object's OWN evaluator handle, batch and wind with nothing between
               them: the step-only time
    python_loop_ms  what a user wrote before this extension: 2 N + 1 WfStep.step calls on the PARENT handle (its farms, its
               wind) with the perturbed yaws and the weighted sums in torch float64 — the same quotient; the three alternate
    kernels    wf_grad_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/grad_timing.py [reps, default 10] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "grad_timing.json")
H, LO, HI = 1.0, -45.0, 45.0
ROBUST_GLUE_SHARE = 0.022  # profiles/robust_timing.json, HornsRev1 x 256: glue over step time of the robust search


def python_loop(w, yaw, c):
    """The quotient of include/wfgrad.h with the API the project had before: 2 N + 1 steps of the parent and torch sums."""
    B, N = yaw.shape
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    power = w.step(yaw)["power"]
    y64, c64 = yaw.double(), c.double()
    yp, ym = torch.clamp(y64 + H, max=HI).float(), torch.clamp(y64 - H, min=LO).float()
    d = yp.double() - ym.double()
    grad = torch.empty((B, N), dtype=torch.float64, device=yaw.device)
    row = yaw.clone()
    for i in range(N):
        row[:, i] = yp[:, i]
        pp = w.step(row)["power"].double()
        row[:, i] = ym[:, i]
        pm = w.step(row)["power"].double()
        row[:, i] = yaw[:, i]
        grad[:, i] = ((pp - pm) * c64).sum(dim=1) / d[:, i]
    b.record()
    b.synchronize()
    return a.elapsed_time(b), power, grad


def workload(label, name, B):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    R = 2 * N + 1
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    yaw = torch.from_numpy(rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32)).cuda()
    out = {"power": torch.empty((B, N), dtype=torch.float32, device="cuda"), "gradient": torch.empty((B, N), dtype=torch.float64, device="cuda")}
    outj = dict(out, jacobian=torch.empty((B, N, N), dtype=torch.float64, device="cuda"))
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(step=H, bounds=(LO, HI))
    for _ in range(2):
        w.yaw_gradient(yaw, c, out=out, **kw)
        w.grad_timing()
        w.yaw_gradient(yaw, c, jacobian=True, out=outj, **kw)
        w.grad_timing()
        plain_loop_ms(w, w._grad(), chunks, n_eval)
        python_loop(w, yaw, c)
    total, jac, plain, loop = [], [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.yaw_gradient(yaw, c, out=out, **kw)
        total.append(w.grad_timing()["total_ms"])
        w.yaw_gradient(yaw, c, jacobian=True, out=outj, **kw)
        jac.append(w.grad_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._grad(), chunks, n_eval))
        ms, p_loop, g_loop = python_loop(w, yaw, c)
        loop.append(ms)
    w.grad_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.yaw_gradient(yaw, c, out=out, **kw)
        det.append(w.grad_timing())
    w.grad_timing(detail=False)
    torch.cuda.synchronize()
    scale = torch.maximum(out["gradient"].abs(), g_loop.abs()).max().item()
    agree = {"power_bits_equal": bool(torch.equal(out["power"], p_loop)),
             "gradient_max_abs_diff_over_largest": float((out["gradient"] - g_loop).abs().max().item() / scale)}
    kernels = w.grad_kernel_info()
    w.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(loop))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "wind": "per farm", "rows_per_farm": R, "chunks": chunks,
         "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "jacobian_total_ms": float(np.median(jac)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue,
         "glue_share_of_step": glue / step, "robust_search_glue_share_of_step": ROBUST_GLUE_SHARE,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "python_loop_ms": q, "python_loop_ms_min": float(np.min(loop)), "python_loop_steps": R, "ratio_total_over_python_loop": t / q,
         "farm_gradients_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3),
         "against_python_loop": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, a wind per farm", "HornsRev1_", 256),
           workload("Ablaincourt x 4096, a wind per farm", "Ablaincourt_", 4096)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device gradient, its Jacobian variant, plain wf_step loop on the evaluator and the Python loop on the parent alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
