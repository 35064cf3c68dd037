"""The gradient of look-ahead returns with respect to the action sequences on the device (csrc/retgrad/,
include/wfretgrad.h): what the gradient of ONE action sequence of H steps costs for every farm, next to the step calls it is
made of and next to the way a user had before.  Writes profiles/retgrad_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm, continuous control, gamma 0.95, delta 1:
    HornsRev1 x 256 farms, K = 1, H = 8, default mode and strict
    Ablaincourt x 4096 farms, K = 1, H = 4, default mode and strict
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of return_gradient — returns and action_gradient, torch tensors in and out —, two events
               per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with four events per chunk; glue = lay-out + reduce kernels
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    lookahead_way_ms   the way a user has without this extension: lookahead_returns over the 2 H N + 1 sequences that move one
               action by +-delta each (built once, outside the timing), in calls of at most 4096 / H sequences, and the
               central differences in torch — median of max(3, reps / 3) runs.  It evaluates H (2 H N + 1) rows per farm,
               this extension H (2 N + 1): `rows_ratio_expected` is the quotient of the two counts, `ratio_measured` the
               quotient of the two times
    kernels    wf_retgrad_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/retgrad_timing.py [reps, default 10] [output file]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "retgrad_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA, DELTA = 0.95, 1.0


def perturbed_sequences(actions):
    """(B, 2 H N + 1, H, N): the sequence itself, then for every (h, i) the sequence with actions[h][i] + delta and - delta."""
    B, _, H, N = actions.shape
    eye = torch.eye(H * N, device=actions.device, dtype=actions.dtype).reshape(H * N, H, N) * DELTA
    base = actions[:, 0]
    return torch.cat([base[:, None], base[:, None] + eye[None], base[:, None] - eye[None]], dim=1).contiguous()


def lookahead_way(w, seqs, strict):
    """The central differences of lookahead_returns over the perturbed sequences, K H <= 4096 per call."""
    B, S, H, N = seqs.shape
    per_call = 4096 // H
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ret = torch.cat([w.lookahead_returns(seqs[:, s:s + per_call].contiguous(), gamma=GAMMA, strict=strict, want="returns")["returns"]
                     for s in range(0, S, per_call)], dim=1)
    grad = ((ret[:, 1:1 + H * N] - ret[:, 1 + H * N:]) / (2.0 * DELTA)).reshape(B, H, N)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), grad


def workload(label, name, B, H, strict):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N, K = len(x), 1
    R = K * H * (2 * N + 1)
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    actions = torch.from_numpy(rng.uniform(-3.0, 3.0, (B, K, H, N)).astype(np.float32)).cuda()
    seqs = perturbed_sequences(actions)
    out = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda"),
           "action_gradient": torch.empty((B, K, H, N), dtype=torch.float64, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(gamma=GAMMA, delta=DELTA, strict=strict, out=out, want=("returns", "action_gradient"))
    for _ in range(2):
        w.return_gradient(actions, **kw)
        w.return_gradient_timing()
        plain_loop_ms(w, w._retgrad(), chunks, n_eval, load=True)
    lookahead_way(w, seqs, strict)
    total, plain = [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.return_gradient(actions, **kw)
        total.append(w.return_gradient_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._retgrad(), chunks, n_eval, load=True))
    hand = []
    for _ in range(max(3, REPS // 3)):
        ms, g_hand = lookahead_way(w, seqs, strict)
        hand.append(ms)
    w.return_gradient_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.return_gradient(actions, **kw)
        det.append(w.return_gradient_timing())
    w.return_gradient_timing(detail=False)
    mask = w.return_gradient(actions, gamma=GAMMA, delta=DELTA, strict=strict, want="pass_mask")["pass_mask"]
    torch.cuda.synchronize()
    # where every flag of the sequence passes, the two ways differentiate the same thing (at the gates and clips they do not)
    open_ = (mask[:, 0] == 3).all(dim=1, keepdim=True).expand(-1, H, -1)
    diff = (out["action_gradient"][:, 0] - g_hand).abs()
    agree = {"share_of_turbines_with_all_flags_open": float(open_.double().mean().item()),
             "max_abs_diff_there": float(diff[open_].max().item()) if open_.any() else None,
             "median_abs_gradient_there": float(out["action_gradient"][:, 0][open_].abs().median().item()) if open_.any() else None}
    kernels = w.return_gradient_kernel_info()
    w.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "sequences": K, "horizon": H, "gamma": GAMMA, "delta": DELTA,
         "mode": "strict" if strict else "default", "wind": "per farm, held over the horizon",
         "rows_per_farm": R, "chunks": chunks, "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "lookahead_way_ms": q, "lookahead_way_ms_min": float(np.min(hand)), "lookahead_way_rows_per_farm": H * (2 * H * N + 1),
         "rows_ratio_expected": H * (2 * H * N + 1) / R, "ratio_measured": q / t,
         "farm_gradients_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3), "against_lookahead_way": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 1, H = 8, a wind per farm, default mode", "HornsRev1_", 256, 8, False),
           workload("HornsRev1 x 256, K = 1, H = 8, a wind per farm, strict", "HornsRev1_", 256, 8, True),
           workload("Ablaincourt x 4096, K = 1, H = 4, a wind per farm, default mode", "Ablaincourt_", 4096, 4, False),
           workload("Ablaincourt x 4096, K = 1, H = 4, a wind per farm, strict", "Ablaincourt_", 4096, 4, True)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call and plain wf_step loop on the evaluator alternate; the lookahead way afterwards",
                   "workloads": res}, f, indent=1)
        f.write("\n")
