"""Policy rollouts over a wind ensemble on the device (csrc/polscen/, include/wfpolscen.h): what the mean, the tail mean and the
choice of K parameter vectors over M wind futures cost for every farm, next to the step calls they are made of and next to the
way a user had to write it with the API of the commit before.  Writes profiles/polscen_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95, tanh networks with random weights
(tools/policy_timing.py's), H = 16, M = 8, tail = 2, risk_weight = 0.5, in the default mode and strict:
    HornsRev1 x 256 farms, K = 8, central 242-64-64-80
    Ablaincourt x 4096 farms, K = 1 and K = 16, shared 3-32-32-1
Per configuration, after 2 warm-up runs (the first builds the evaluators and times their kernel families):
    total_ms   median (min, max) of `reps` runs of policy_scenarios — expected_returns, cvar, score and best, torch tensors in
               and out —, two events per run
    step_ms / glue_ms   median of `reps` more runs with the events split per launch; glue = every kernel between two steps and
               the evaluator's wind update after every advance
    plain_loop_ms   the same number of wf_step calls (H + 1 per chunk: power and load) on the object's OWN evaluator, nothing between
    hand_written_ms   the parent commit's API: scenario_returns once for wind_paths (one all-hold sequence), M calls of
               policy_returns(wind=wind_paths[:, m]), then torch mean / topk / argmax over the M returns
    same_best  whether both ways name the same policy on every farm (the member returns are the same bits; the torch mean and
               tail mean add in another order)
Run from the repo root on an MI355X:  python tools/polscen_timing.py [reps, default 5] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ext_timing import plain_loop_ms  # noqa: E402
from tools.policy_timing import ENV, GAMMA, LAYOUTS, network  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "polscen_timing.json")
H, M, TAIL, LAM, SEED = 16, 8, 2, 0.5, 3
PROCESS = dict(ws_revert=0.05, ws_sigma=0.25, wd_revert=0.05, wd_sigma=1.5, wd_ramp=0.5)
BOUNDS = (3.0, 28.0)


def hand_written(w, par_t, spec, hold, strict):
    """expected_returns, cvar, score, best with the parent commit's API, between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    paths = w.scenario_returns(hold, M, PROCESS, seed=SEED, gamma=GAMMA, tail=TAIL, bounds=BOUNDS, strict=strict, want=("wind_paths",))["wind_paths"]
    rets = [w.policy_returns(par_t, spec, H, gamma=GAMMA, wind=paths[:, m].contiguous(), strict=strict, want=("returns",))["returns"]
            for m in range(M)]
    mr = torch.stack(rets, dim=2)
    mean = mr.mean(dim=2)
    cvar = mr.topk(TAIL, dim=2, largest=False).values.mean(dim=2)
    score = (1.0 - LAM) * mean + LAM * cvar
    best = score.argmax(dim=1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), best, mr


def workload(label, name, B, kind, widths, K, strict):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    rng = np.random.default_rng(7)
    params, spec = network(kind, widths, N, K, rng)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    par_t = torch.from_numpy(params).cuda()
    hold = torch.zeros((B, 1, H, N), dtype=torch.float32, device="cuda")
    f8 = torch.float64
    out = {"expected_returns": torch.empty((B, K), dtype=f8, device="cuda"), "cvar": torch.empty((B, K), dtype=f8, device="cuda"),
           "score": torch.empty((B, K), dtype=f8, device="cuda"), "best": torch.empty(B, dtype=torch.int32, device="cuda")}
    rows = K * M
    per_chunk = min(B, 65536 // rows)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * rows
    kw = dict(seed=SEED, gamma=GAMMA, tail=TAIL, risk_weight=LAM, bounds=BOUNDS, strict=strict, out=out)
    run = lambda **k: w.policy_scenarios(par_t, spec, H, M, PROCESS, **dict(kw, **k))
    for _ in range(2):
        run()
        w.policy_scenarios_timing()
        plain_loop_ms(w, w._polscen(), chunks * (H + 1), n_eval, load=True)
        hand_written(w, par_t, spec, hold, strict)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        run()
        total.append(w.policy_scenarios_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._polscen(), chunks * (H + 1), n_eval, load=True))
        ms, best_hand, mr_hand = hand_written(w, par_t, spec, hold, strict)
        hand.append(ms)
    w.policy_scenarios_timing(detail=True)
    det = []
    for _ in range(REPS):
        run()
        det.append(w.policy_scenarios_timing())
    w.policy_scenarios_timing(detail=False)
    extra = run(out=None, want=("member_returns", "best", "expected_returns", "cvar"))
    torch.cuda.synchronize()
    same_best = bool((extra["best"].long() == best_hand).all().item())
    agree = {"same_best_on_every_farm": same_best, "farms_with_another_best": int((extra["best"].long() != best_hand).sum().item()),
             "member_returns_same_bits": bool(torch.equal(extra["member_returns"], mr_hand)),
             "expected_return_mean": float(extra["expected_returns"].mean().item()),
             "mean_minus_cvar_mean": float((extra["expected_returns"] - extra["cvar"]).mean().item())}
    kernels = w.policy_scenarios_kernel_info()
    w.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "policies": K, "members": M, "horizon": H, "tail": TAIL,
         "risk_weight": LAM, "gamma": GAMMA, "kind": kind, "widths": list(widths), "control": "continuous",
         "mode": "strict" if strict else "default", "rows_per_farm": rows, "chunks": chunks, "evaluator_farms": n_eval,
         "steps_per_chunk": H + 1, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "glue_exceeds_step": bool(glue > step),
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "plain_loop_ms_max": float(np.max(plain)), "ratio_total_over_plain_loop": t / p,
         "hand_written_ms": q, "hand_written_ms_min": float(np.min(hand)), "hand_written_ms_max": float(np.max(hand)),
         "ratio_total_over_hand_written": t / q, "one_call_is_ahead": bool(t < q),
         "farm_rollouts_per_s": B * rows / (t * 1e-3), "results": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
    res = []
    for strict in (False, True):
        mode = "strict" if strict else "default mode"
        res += [workload(f"HornsRev1 x 256, K = 8, M = 8, H = 16, central 242-64-64-80, {mode}", "HornsRev1_", 256, "central", (242, 64, 64, 80), 8, strict),
                workload(f"Ablaincourt x 4096, K = 1, M = 8, H = 16, shared 3-32-32-1, {mode}", "Ablaincourt_", 4096, "shared", (3, 32, 32, 1), 1, strict),
                workload(f"Ablaincourt x 4096, K = 16, M = 8, H = 16, shared 3-32-32-1, {mode}", "Ablaincourt_", 4096, "shared", (3, 32, 32, 1), 16, strict)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median (min, max) of "
                   "`reps`; the one call, the plain wf_step loop on its evaluator and the hand-written way alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
