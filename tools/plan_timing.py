"""The receding-horizon planner on the device (csrc/plan/, include/wfplan.h): what a plan — I iterations of the cross-entropy
method over K action sequences of H steps — costs for every farm, next to the step calls it is made of and next to the way a
user had to write it before.  Writes profiles/plan_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95, default mode, the default widths
(1, 1/2, 1/4) yaw_step, E = K / 4 elites:
    HornsRev1 x 256 farms, K = 32, H = 8, I = 3
    Ablaincourt x 4096 farms, K = 16, H = 4, I = 3
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of plan_actions — first_action, mean and plan_return, torch tensors in and out —, two
               events per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with 2 I + 2 events per chunk; glue = the I + 1 launches of the one kernel
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    hand_written_ms   what a user wrote before this extension: I calls of lookahead_returns, the candidates drawn with torch
               on the device (randn, clamp), topk of the returns, a gather and a mean in between, the best sequence kept
    kernels    wf_plan_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/plan_timing.py [reps, default 10] [output file]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "plan_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA = 0.95
SIGMA = (5.0, 2.5, 1.25)


def hand_written(w, mean, K, E, gen):
    """The same method over the API the project had before: per iteration torch draws, one lookahead_returns, topk and mean."""
    B, H, N = mean.shape
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    mu, best = mean.clone(), torch.zeros_like(mean)
    rows = torch.arange(B, device="cuda")
    for s in SIGMA:
        seqs = (mu[:, None] + s * torch.randn((B, K, H, N), device="cuda", generator=gen)).clamp_(-5.0, 5.0)
        seqs[:, 0], seqs[:, 1] = best, mu
        r = w.lookahead_returns(seqs, gamma=GAMMA, want=("returns", "best"))
        top = r["returns"].topk(E, dim=1).indices
        mu = seqs[rows[:, None], top].double().mean(dim=1).float()
        best = seqs[rows, r["best"].long()]
        ret = r["returns"][rows, r["best"].long()]
    b.record()
    b.synchronize()
    return a.elapsed_time(b), best, ret


def workload(label, name, B, K, H):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N, R, E, I = len(x), K * H, K // 4, len(SIGMA)
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    mean = torch.zeros((B, H, N), dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    out = {"first_action": torch.empty((B, N), dtype=torch.float32, device="cuda"), "mean": torch.empty_like(mean),
           "plan_return": torch.empty(B, dtype=torch.float64, device="cuda"), "hold_return": torch.empty(B, dtype=torch.float64, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(candidates=K, elites=E, sigma=SIGMA, seed=7, gamma=GAMMA, mean=mean, want=tuple(out), out=out)
    for _ in range(2):
        w.plan_actions(H, **kw)
        w.plan_timing()
        plain_loop_ms(w, w._plan(), I * chunks, n_eval, load=True)
        hand_written(w, mean, K, E, gen)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.plan_actions(H, **kw)
        total.append(w.plan_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._plan(), I * chunks, n_eval, load=True))
        ms, _, r_hand = hand_written(w, mean, K, E, gen)
        hand.append(ms)
    w.plan_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.plan_actions(H, **kw)
        det.append(w.plan_timing())
    w.plan_timing(detail=False)
    torch.cuda.synchronize()
    gain = out["plan_return"] - out["hold_return"]
    quality = {"median_gain_over_hold": float(gain.median().item()), "share_of_farms_better_than_hold": float((gain > 0).double().mean().item()),
               "hand_written_median_gain_over_hold": float((r_hand - out["hold_return"]).median().item())}
    kernels = w.plan_kernel_info()
    w.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "candidates": K, "elites": E, "horizon": H, "iterations": I,
         "sigma": list(SIGMA), "gamma": GAMMA, "mode": "default", "wind": "per farm, held over the horizon", "rows_per_farm": R,
         "chunks": chunks, "evaluator_farms": n_eval, "evaluator_steps": I * chunks, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "hand_written_ms": q, "hand_written_ms_min": float(np.min(hand)), "ratio_total_over_hand_written": t / q,
         "farm_plans_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R * I / (t * 1e-3), "quality": quality, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 32, H = 8, I = 3, a wind per farm, default mode", "HornsRev1_", 256, 32, 8),
           workload("Ablaincourt x 4096, K = 16, H = 4, I = 3, a wind per farm, default mode", "Ablaincourt_", 4096, 16, 4)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written lookahead_returns way alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
