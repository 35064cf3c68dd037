"""Multi-step look-ahead returns on the device (csrc/lookahead/, include/wflookahead.h): what the returns of K action
sequences of H steps cost for every farm, next to the step calls they are made of and next to the way a user had to write
them before.  Writes profiles/lookahead_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95:
    HornsRev1 x 256 farms, K = 32, H = 8, default mode and strict
    Ablaincourt x 4096 farms, K = 16, H = 4, default mode
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of lookahead_returns — returns and best, torch tensors in and out —, two events per run
               (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with four events per chunk; glue = lay-out + reduce kernels
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    python_way_ms   what a user wrote before this extension: a second WfStep of B K farms; the env state read back, repeated
               K times and set with env_set_state, the winds repeated and set; a Python loop of H env_step calls; the
               discounted sum and the argmax in torch float64 — every call; the three alternate
    kernels    wf_lookahead_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/lookahead_timing.py [reps, default 10] [output file]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lookahead_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA = 0.95


def python_way(w, w2, actions):
    """The returns with the API the project had before: K copies of every farm's env state in a second handle, H env steps."""
    B, K, H, N = actions.shape
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = w.env_get_state()
    ws, wd = w.get_wind(as_torch=True)
    w2.env_set_state({"yaw": np.repeat(st["yaw"], K, axis=0), "acc": np.repeat(st["acc"], K, axis=0), "moves": np.repeat(st["moves"], K)})
    w2.set_wind(ws.repeat_interleave(K), wd.repeat_interleave(K))
    ret = torch.zeros(B * K, dtype=torch.float64, device="cuda")
    g = 1.0
    for h in range(H):
        r = w2.env_step(actions[:, :, h].reshape(B * K, N), want=("reward",))["reward"]
        ret = ret + g * r.double()
        g = g * GAMMA
    ret = ret.reshape(B, K)
    best = ret.argmax(dim=1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), ret, best


def workload(label, name, B, K, H, strict):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    R = K * H
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    actions = torch.from_numpy(rng.uniform(-5.0, 5.0, (B, K, H, N)).astype(np.float32)).cuda()
    w2 = WfStep(x, y, env_batch=B * K)  # the hand-written way's second handle
    w2.env_config(**ENV)
    w2.env_reset()
    w2.set_risk_resolve(2 if strict else 1)
    out = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda"), "best": torch.empty(B, dtype=torch.int32, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(gamma=GAMMA, strict=strict, out=out)
    for _ in range(2):
        w.lookahead_returns(actions, **kw)
        w.lookahead_timing()
        plain_loop_ms(w, w._lookahead(), chunks, n_eval, load=True)
        python_way(w, w2, actions)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.lookahead_returns(actions, **kw)
        total.append(w.lookahead_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._lookahead(), chunks, n_eval, load=True))
        ms, r_hand, b_hand = python_way(w, w2, actions)
        hand.append(ms)
    w.lookahead_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.lookahead_returns(actions, **kw)
        det.append(w.lookahead_timing())
    w.lookahead_timing(detail=False)
    torch.cuda.synchronize()
    spread = out["returns"].max(dim=1).values - out["returns"].min(dim=1).values
    agree = {"returns_max_abs_diff": float((out["returns"] - r_hand).abs().max().item()),
             "returns_median_spread_within_a_farm": float(spread.median().item()),
             "best_agree_share": float((out["best"].long() == b_hand).double().mean().item())}
    kernels = w.lookahead_kernel_info()
    w.close()
    w2.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "sequences": K, "horizon": H, "gamma": GAMMA,
         "control": "continuous", "mode": "strict" if strict else "default", "wind": "per farm, held over the horizon",
         "rows_per_farm": R, "chunks": chunks, "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "python_way_ms": q, "python_way_ms_min": float(np.min(hand)), "ratio_total_over_python_way": t / q,
         "farm_lookaheads_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3), "against_python_way": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 32, H = 8, a wind per farm, default mode", "HornsRev1_", 256, 32, 8, False),
           workload("HornsRev1 x 256, K = 32, H = 8, a wind per farm, strict", "HornsRev1_", 256, 32, 8, True),
           workload("Ablaincourt x 4096, K = 16, H = 4, a wind per farm, default mode", "Ablaincourt_", 4096, 16, 4, False)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written env_step way alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
