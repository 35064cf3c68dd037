"""The scenario planner on the device (csrc/scenplan/, include/wfscenplan.h): what a plan of every farm — I iterations of K
candidates of H steps, each scored over M wind futures — costs, next to the step calls it is made of and next to the way a
user had to write it before.  Writes profiles/scenplan_timing.json.  Recorded, not gated.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95, process (0.1, 0.5, 0.05, 2.0, 0.5),
tail M / 4, risk weight 0.5, E = K / 4 elites, I = 3 iterations of the default widths — tools/scenario_timing.py's two shapes:
    HornsRev1 x 256 farms, K = 16, M = 8, H = 8, default mode and strict
    Ablaincourt x 4096 farms, K = 8, M = 8, H = 4, default mode and strict
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of plan_scenarios — plan, plan_score, first_action, mean, torch tensors out —, two events
               per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with 2 I + 2 events per chunk; glue = the paths kernel + the I + 1 launches
               of the advance kernel
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    hand_way_ms   what a user wrote before this extension, on the same commit: I calls of scenario_returns — which draws the
               same member paths on the device each time — with the candidates formed in torch before each and torch topk,
               mean and argmax behind it.  It is handed the device's own deviates as a device tensor made beforehand
               (tests/plan_ref.py's Philox in NumPy: drawing and uploading them is NOT in its time), so that the two ways
               can name the same plan: its candidates then have the device's bits, its elite mean is a torch sum
    kernels    wf_scenplan_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/scenplan_timing.py [reps, default 10] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_ref  # noqa: E402  (the deviate, restated in NumPy)
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "scenplan_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA, LAM, SEED, SCENARIO_SEED = 0.95, 0.5, 3, 7
SIGMA = (5.0, 2.5, 1.25)
PROCESS = dict(ws_revert=0.1, ws_sigma=0.5, wd_revert=0.05, wd_sigma=2.0, wd_ramp=0.5)


def deviates(B, K, H, N):
    """[I][B][K][H][N] float64 on the device: the planner's deviates of every farm, iteration and element (k < 2 unused)."""
    idx = np.arange(K * H * N, dtype=np.uint64).reshape(1, K, H, N)
    farm = np.arange(B, dtype=np.uint64).reshape(B, 1, 1, 1)
    return torch.from_numpy(np.stack([plan_ref.deviate(SEED, farm, idx, i) for i in range(len(SIGMA))])).cuda()


def hand_way(w, z, E, M, q, strict):
    """The plan with the API the project had before: a scenario_returns call per iteration, draws and refit in torch."""
    I, B, K, H, N = z.shape
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    mu = torch.zeros((B, H, N), dtype=torch.float32, device="cuda")
    best = torch.zeros_like(mu)
    rows = torch.arange(B, device="cuda")
    for i in range(I):
        cand = (mu[:, None].double() + SIGMA[i] * z[i]).clamp_(-ENV["yaw_step"], ENV["yaw_step"]).float()
        cand[:, 0], cand[:, 1] = best, mu
        score = w.scenario_returns(cand, M, PROCESS, seed=SCENARIO_SEED, gamma=GAMMA, tail=q, risk_weight=LAM, strict=strict,
                                   want=("score",))["score"]
        elite = torch.zeros_like(score, dtype=torch.bool).scatter_(1, score.topk(E, dim=1).indices, True)
        mu = ((cand.double() * elite[:, :, None, None]).sum(dim=1) / E).float()
        win = score.argmax(dim=1)
        best = cand[rows, win]
        plan_score = score[rows, win]
    b.record()
    b.synchronize()
    return a.elapsed_time(b), best, plan_score


def workload(label, name, B, K, M, H, strict, z):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    R, q, E, I = K * M * H, max(1, M // 4), max(1, K // 4), len(SIGMA)
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    out = {"plan": torch.empty((B, H, N), dtype=torch.float32, device="cuda"), "plan_score": torch.empty(B, dtype=torch.float64, device="cuda"),
           "first_action": torch.empty((B, N), dtype=torch.float32, device="cuda"), "mean": torch.empty((B, H, N), dtype=torch.float32, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(candidates=K, elites=E, members=M, process=PROCESS, sigma=SIGMA, seed=SEED, scenario_seed=SCENARIO_SEED, gamma=GAMMA, tail=q,
              risk_weight=LAM, strict=strict, want=tuple(out), out=out)
    for _ in range(2):
        w.plan_scenarios(H, **kw)
        w.plan_scenarios_timing()
        plain_loop_ms(w, w._scenplan(), chunks * I, n_eval, load=True)
        hand_way(w, z, E, M, q, strict)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.plan_scenarios(H, **kw)
        total.append(w.plan_scenarios_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._scenplan(), chunks * I, n_eval, load=True))
        ms, p_hand, s_hand = hand_way(w, z, E, M, q, strict)
        hand.append(ms)
    w.plan_scenarios_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.plan_scenarios(H, **kw)
        det.append(w.plan_scenarios_timing())
    w.plan_scenarios_timing(detail=False)
    torch.cuda.synchronize()
    same = (out["plan"] == p_hand).all(dim=2).all(dim=1)
    agree = {"same_plan_share": float(same.double().mean().item()),
             "plan_score_max_abs_diff_where_same_plan": float((out["plan_score"] - s_hand)[same].abs().max().item()) if bool(same.any()) else None,
             "plan_score_mean": float(out["plan_score"].mean().item()), "hand_way_plan_score_mean": float(s_hand.mean().item())}
    kernels = w.plan_scenarios_kernel_info()
    w.close()
    t, p, h = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "candidates": K, "elites": E, "members": M, "horizon": H,
         "iterations": I, "sigma": SIGMA, "gamma": GAMMA, "tail": q, "risk_weight": LAM, "process": PROCESS, "control": "continuous",
         "mode": "strict" if strict else "default", "rows_per_farm": R, "chunks": chunks, "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "hand_way_ms": h, "hand_way_ms_min": float(np.min(hand)), "ratio_total_over_hand_way": t / h,
         "farm_plans_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R * I / (t * 1e-3), "against_hand_way": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = []
    shapes = (("HornsRev1 x 256, K = 16, M = 8, H = 8", "HornsRev1_", 256, 16, 8, 8), ("Ablaincourt x 4096, K = 8, M = 8, H = 4", "Ablaincourt_", 4096, 8, 8, 4))
    for label, name, B, K, M, H in shapes:
        z = deviates(B, K, H, len(LAYOUTS[name]["xcoords"]))
        for strict in (False, True):
            res.append(workload(f"{label}, I = 3, a wind per farm, {'strict' if strict else 'default mode'}", name, B, K, M, H, strict, z))
        del z
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written way (I scenario_returns calls + torch) alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
