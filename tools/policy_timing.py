"""Closed-loop rollouts of MLP policies on the device (csrc/policy/, include/wfpolicy.h): what the returns of K parameter
vectors over H steps cost for every farm, next to the step calls they are made of and next to the way a user had to write it
before.  Writes profiles/policy_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm held over the horizon, continuous control, gamma 0.95, tanh networks
with random weights (scaled by 1 / sqrt(in)) and a tanh output scaled to the yaw step, default mode:
    HornsRev1 x 256 farms, K = 8, H = 16, central 242-64-64-80
    Ablaincourt x 4096 farms, K = 1 and K = 16, H = 16, shared 3-32-32-1
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of policy_returns — returns and best, torch tensors in and out —, two events per run
    step_ms / glue_ms   median of `reps` more runs with the events split per launch; glue = begin + advance + reduce kernels
    plain_loop_ms   the same number of wf_step calls (H + 1 per chunk: power and load) on the object's OWN evaluator, nothing between
    python_way_ms   what a user wrote before this extension: a second WfStep of n K farms given the env state (env_set_state,
               every farm's state K times) and the wind; one step at the current yaw for the first observation; a Python
               loop of H times a float32 torch MLP (bmm over the K policies) and env_step; the discounted sum in torch float64.
               Its returns differ from the extension's: float32 network, no fixed order (recorded)
    kernels    wf_policy_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/policy_timing.py [reps, default 10] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd import policy as P  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "policy_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA = 0.95


def network(kind, widths, N, K, rng):
    D = widths[0]
    if kind == "central":
        shift = np.concatenate([np.zeros(N), np.full(N, 8.0), np.full(N, 270.0), [8.0, 270.0]])
        scale = np.concatenate([np.full(N, 1 / 20.0), np.full(N, 1 / 4.0), np.full(N, 1 / 15.0), [1 / 4.0, 1 / 15.0]])
    else:
        shift, scale = np.array([0.0, 8.0, 270.0]), np.array([1 / 20.0, 1 / 4.0, 1 / 15.0])
    spec = P.mlp_spec(kind, widths, "tanh", "tanh", out_scale=5.0, shift=shift, scale=scale)
    vecs = []
    for _ in range(K):
        parts = []
        for a, b in zip(widths[:-1], widths[1:]):
            parts += [rng.uniform(-1.0, 1.0, a * b) * (2.0 / np.sqrt(a)), rng.uniform(-0.5, 0.5, b)]
        vecs.append(np.concatenate(parts))
    assert D == shift.size
    return np.ascontiguousarray(np.stack(vecs), dtype=np.float32), spec


def torch_layers(params, spec):
    """[(W (K, in, out), b (K, 1, out))] float32 CUDA tensors of the K parameter vectors."""
    widths, out, o = spec["widths"], [], 0
    t = torch.from_numpy(params).cuda()
    for a, b in zip(widths[:-1], widths[1:]):
        W = t[:, o:o + a * b].reshape(-1, b, a).transpose(1, 2).contiguous()
        o += a * b
        out.append((W, t[:, o:o + b].reshape(-1, 1, b).contiguous()))
        o += b
    return out


def python_way(w, w2, layers, spec, n, K, N, H):
    """The K policies' returns with the API the project had before: an env of n K farms stepped H times around a torch MLP."""
    shift = torch.from_numpy(spec["shift"]).float().cuda()
    scale = torch.from_numpy(spec["scale"]).float().cuda()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = w.env_get_state()
    w2.env_set_state({"yaw": np.repeat(st["yaw"], K, axis=0), "acc": np.repeat(st["acc"], K, axis=0), "moves": np.repeat(st["moves"], K)})
    ws, wd = w.get_wind()
    w2.set_wind(np.repeat(ws, K), np.repeat(wd, K))
    fw = torch.from_numpy(np.stack([np.repeat(ws, K), np.repeat(wd, K)], axis=1)).float().cuda()
    yaw = torch.from_numpy(np.repeat(st["yaw"], K, axis=0)).cuda()
    o = w2.step(yaw)
    lws, lwd = o["wind_speed"], o["wind_direction"]
    ret = torch.zeros(n * K, dtype=torch.float64, device="cuda")
    g = 1.0
    for h in range(H):
        if spec["kind"] == "central":
            x = ((torch.cat([yaw, lws, lwd, fw], dim=1) - shift) * scale).reshape(n, K, -1).transpose(0, 1)  # (K, n, D)
        else:
            x = ((torch.stack([yaw, lws, lwd], dim=2) - shift) * scale).reshape(n, K, N, 3).transpose(0, 1).reshape(K, n * N, 3)
        for l, (W, bias) in enumerate(layers):
            x = torch.tanh(torch.baddbmm(bias, x, W))
        act = (5.0 * x).reshape(K, n, N).transpose(0, 1).reshape(n * K, N).contiguous()
        r = w2.env_step(act, want=("reward", "yaw", "wind_speed", "wind_direction"))
        yaw, lws, lwd = r["yaw"], r["wind_speed"], r["wind_direction"]
        ret = ret + g * r["reward"].double()
        g = g * GAMMA
    b.record()
    b.synchronize()
    return a.elapsed_time(b), ret.reshape(n, K)


def workload(label, name, B, kind, widths, K, H):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    rng = np.random.default_rng(7)
    params, spec = network(kind, widths, N, K, rng)
    ws0, wd0 = rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws0, wd0)
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    w2 = WfStep(x, y, env_batch=B * K)  # the hand-written way's env of n K farms
    w2.env_config(**ENV)
    w2.set_wind(np.repeat(ws0, K), np.repeat(wd0, K))
    w2.env_reset()
    layers = torch_layers(params, spec)
    par_t = torch.from_numpy(params).cuda()
    out = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda"), "best": torch.empty(B, dtype=torch.int32, device="cuda")}
    per_chunk = min(B, 65536 // K)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * K
    kw = dict(gamma=GAMMA, out=out)
    for _ in range(2):
        w.policy_returns(par_t, spec, H, **kw)
        w.policy_timing()
        plain_loop_ms(w, w._policy(), chunks * (H + 1), n_eval, load=True)
        python_way(w, w2, layers, spec, B, K, N, H)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.policy_returns(par_t, spec, H, **kw)
        total.append(w.policy_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._policy(), chunks * (H + 1), n_eval, load=True))
        ms, r_hand = python_way(w, w2, layers, spec, B, K, N, H)
        hand.append(ms)
    w.policy_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.policy_returns(par_t, spec, H, **kw)
        det.append(w.policy_timing())
    w.policy_timing(detail=False)
    extra = w.policy_returns(par_t, spec, H, gamma=GAMMA, want=("returns", "gated", "actions"))
    torch.cuda.synchronize()
    ret = out["returns"]
    agree = {"returns_max_abs_diff_to_python_way": float((ret - r_hand).abs().max().item()),
             "returns_median_abs_diff_to_python_way": float((ret - r_hand).abs().median().item()),
             "return_mean": float(ret.mean().item()), "return_spread_over_policies_mean": float((ret.max(dim=1).values - ret.min(dim=1).values).mean().item()),
             "mean_abs_action": float(extra["actions"].abs().mean().item()), "mean_gated_pairs": float(extra["gated"].double().mean().item())}
    kernels = w.policy_kernel_info()
    w.close()
    w2.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "policies": K, "horizon": H, "gamma": GAMMA, "kind": kind,
         "widths": list(widths), "parameters": int(params.shape[1]), "control": "continuous", "mode": "default", "wind": "per farm, held",
         "rows_per_farm": K, "chunks": chunks, "evaluator_farms": n_eval, "steps_per_chunk": H + 1, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "glue_exceeds_step": bool(glue > step),
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "python_way_ms": q, "python_way_ms_min": float(np.min(hand)), "ratio_total_over_python_way": t / q,
         "farm_rollouts_per_s": B * K / (t * 1e-3), "farm_steps_per_s": B * K * H / (t * 1e-3), "results": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 8, H = 16, central 242-64-64-80, default mode", "HornsRev1_", 256, "central", (242, 64, 64, 80), 8, 16),
           workload("Ablaincourt x 4096, K = 1, H = 16, shared 3-32-32-1, default mode", "Ablaincourt_", 4096, "shared", (3, 32, 32, 1), 1, 16),
           workload("Ablaincourt x 4096, K = 16, H = 16, shared 3-32-32-1, default mode", "Ablaincourt_", 4096, "shared", (3, 32, 32, 1), 16, 16)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written torch MLP + env_step way alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
