"""Scenario rollouts on the device (csrc/rollscen/, include/wfrollscen.h): what scoring K yaw-table controllers in closed loop
over H steps under an ensemble of M wind futures costs for every farm, next to the step calls it is made of and next to the way
a user had to write it before.  Writes profiles/rollscen_timing.json.  Recorded, not gated.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95, process (0.1, 0.5, 0.05, 2.0, 0.5),
tail M / 4, risk weight 0.5; K = 8 controllers — controller_grid over gains (1, 0.5), deadbands (0, 2) and leads (0, 1) — on a
synthetic steering table over the whole circle:
    HornsRev1 x 256 farms, K = 8, M = 8, H = 16, default mode and strict
    Ablaincourt x 4096 farms, K = 8, M = 8, H = 4, default mode and strict
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of controller_scenarios — expected_returns, cvar, score and best, torch tensors out —, two
               events per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with four events per chunk; glue = lay-out + reduce kernels
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    hand_way_ms   what a user wrote before this extension, on the same commit: M calls of controller_returns(wind = the
               member's path), then torch mean, topk and argmax over the stacked returns.  The member paths are handed to it
               as a device tensor made beforehand (this extension's own wind_paths): drawing and uploading them is NOT in
               its time
    kernels    wf_rollscen_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/rollscen_timing.py [reps, default 10] [output file]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rollscen_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA, LAM, SEED = 0.95, 0.5, 7
PROCESS = dict(ws_revert=0.1, ws_sigma=0.5, wd_revert=0.05, wd_sigma=2.0, wd_ramp=0.5)


def steering_table(N, twd, tws):
    """(Dt, St, N) float32: per turbine an amplitude of 8 to 24 degrees, a sine of period 90 degrees in the direction, shrinking
    with the speed — what the look-up is given matters here, not whether it is an optimum."""
    amp = np.random.default_rng(1).uniform(8.0, 24.0, N)
    speed = 1.0 - 0.25 * np.arange(len(tws)) / (len(tws) - 1)
    return (np.sin(np.pi * twd / 45.0)[:, None, None] * speed[None, :, None] * amp[None, None, :]).astype(np.float32)


def hand_way(w, ctl, H, paths, q, strict):
    """The statistics with the API the project had before: a rollout call per member, the reductions in torch."""
    M = paths.shape[1]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ret = torch.stack([w.controller_returns(ctl, H, gamma=GAMMA, wind=paths[:, m].contiguous(), strict=strict, want=("returns",))["returns"]
                       for m in range(M)], dim=2)
    mean = ret.mean(dim=2)
    cvar = ret.topk(q, dim=2, largest=False).values.mean(dim=2)
    score = (1.0 - LAM) * mean + LAM * cvar
    best = score.argmax(dim=1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), score, best


def workload(label, name, B, K, M, H, strict):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    R, q = K * M * H, max(1, M // 4)
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    twd, tws = np.arange(5.0, 360.0, 10.0), np.array([6.0, 8.0, 10.0, 12.0])
    w.set_yaw_table(steering_table(N, twd, tws), twd, tws, interp="linear", slot=0)
    ctl, _ = WfStep.controller_grid([1.0, 0.5], [0.0, 2.0], [0, 1], slot=0)
    assert len(ctl["alpha"]) == K
    names = ("expected_returns", "cvar", "score")
    out = {k: torch.empty((B, K), dtype=torch.float64, device="cuda") for k in names}
    out["best"] = torch.empty(B, dtype=torch.int32, device="cuda")
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(process=PROCESS, seed=SEED, gamma=GAMMA, tail=q, risk_weight=LAM, strict=strict)
    paths = w.controller_scenarios(ctl, H, M, want="wind_paths", out={"wind_paths": torch.empty((B, M, H, 2), dtype=torch.float64, device="cuda")}, **kw)["wind_paths"]
    kw.update(want=names + ("best",), out=out)
    for _ in range(2):
        w.controller_scenarios(ctl, H, M, **kw)
        w.controller_scenarios_timing()
        plain_loop_ms(w, w._rollscen(), chunks, n_eval, load=True)
        hand_way(w, ctl, H, paths, q, strict)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.controller_scenarios(ctl, H, M, **kw)
        total.append(w.controller_scenarios_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._rollscen(), chunks, n_eval, load=True))
        ms, s_hand, b_hand = hand_way(w, ctl, H, paths, q, strict)
        hand.append(ms)
    w.controller_scenarios_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.controller_scenarios(ctl, H, M, **kw)
        det.append(w.controller_scenarios_timing())
    w.controller_scenarios_timing(detail=False)
    torch.cuda.synchronize()
    spread = out["score"].max(dim=1).values - out["score"].min(dim=1).values
    agree = {"score_max_abs_diff": float((out["score"] - s_hand).abs().max().item()),
             "score_median_spread_within_a_farm": float(spread.median().item()),
             "best_agree_share": float((out["best"].long() == b_hand).double().mean().item())}
    kernels = w.controller_scenarios_kernel_info()
    w.close()
    t, p, h = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "controllers": K, "members": M, "horizon": H, "gamma": GAMMA,
         "tail": q, "risk_weight": LAM, "process": PROCESS, "control": "continuous", "mode": "strict" if strict else "default",
         "rows_per_farm": R, "chunks": chunks, "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "hand_way_ms": h, "hand_way_ms_min": float(np.min(hand)), "ratio_total_over_hand_way": t / h,
         "farm_scenarios_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3), "against_hand_way": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = []
    for strict in (False, True):
        mode = "strict" if strict else "default mode"
        res.append(workload(f"HornsRev1 x 256, K = 8, M = 8, H = 16, a wind per farm, {mode}", "HornsRev1_", 256, 8, 8, 16, strict))
        res.append(workload(f"Ablaincourt x 4096, K = 8, M = 8, H = 4, a wind per farm, {mode}", "Ablaincourt_", 4096, 8, 8, 4, strict))
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written way (M rollout calls + torch) alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
