"""Closed-loop rollouts of yaw-table controllers on the device (csrc/rollout/, include/wfrollout.h): what the returns of K
controllers over H steps cost for every farm, next to the step calls they are made of and next to the way a user had to write
the ONE untuned controller before.  Writes profiles/rollout_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm and a wind per step (a slow swing of the direction plus noise),
continuous control, gamma 0.95, a synthetic steering table on a 2.5 deg grid (NEAREST), default mode:
    HornsRev1 x 256 farms, K = 8, H = 64      Ablaincourt x 4096 farms, K = 16, H = 16
The K controllers are the grid alpha x deadband x lead of WfStep.controller_grid; controller 0 is the untuned one.
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of controller_returns — returns and best, torch tensors in and out —, two events per run
    step_ms / glue_ms   median of `reps` more runs with four events per chunk; glue = lay-out + reduce kernels
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    python_way_ms   what a user wrote before this extension, for the untuned controller ALONE (1 / K of the work): a second
               WfStep of B farms given the env state (env_set_state) and the wind; a Python loop of H times lut_policy's
               action, set_wind to the step's wind, env_set_prev_wind, env_step; the discounted sum in torch float64
    series_ahead_ms / series_by_rows_ms   the parent in series mode: wind="series" (the window enqueued on the device) against
               the window gathered on the host from series_state() and passed as wind= (host time included)
    kernels    wf_rollout_kernel_info: vgprs / static LDS bytes / private-segment bytes
Run from the repo root on an MI355X:  python tools/rollout_timing.py [reps, default 10] [output file]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rollout_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
GAMMA = 0.95
TWD, TWS = np.arange(0.0, 360.0, 2.5), np.array([6.0, 8.0, 10.0, 12.0])


def steering_table(N, rng):
    """(Dt, St, N) float32: per turbine an amplitude of 8 to 24 deg times one sine period over +-20 deg around west."""
    d = (TWD - 270.0 + 180.0) % 360.0 - 180.0
    shape = np.where(np.abs(d) <= 20.0, np.sin(np.pi * d / 20.0), 0.0)
    return (shape[:, None, None] * np.linspace(1.0, 0.75, TWS.size)[None, :, None] * rng.uniform(8.0, 24.0, N)[None, None, :]).astype(np.float32)


def swing(rng, B, H, ws0, wd0):
    h = np.arange(1, H + 1)
    phase = rng.uniform(0.0, 2.0 * np.pi, (B, 1))
    ar = np.zeros((B, H))
    e = rng.normal(0.0, 2.0, (B, H))
    for i in range(1, H):
        ar[:, i] = 0.7 * ar[:, i - 1] + e[:, i]
    wd = wd0[:, None] + 14.0 * (np.sin(2.0 * np.pi * h[None, :] / 40.0 + phase) - np.sin(phase)) + ar
    ws = ws0[:, None] * (1.0 + 0.03 * np.sin(2.0 * np.pi * h[None, :] / 11.0 + phase))
    return np.ascontiguousarray(np.stack([ws, wd], axis=2))


def python_way(w, w2, wind):
    """The untuned controller's return with the API the project had before: a copy of the env stepped H times with lut_policy."""
    B, H = wind.shape[:2]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    w2.env_set_state(w.env_get_state())
    ws, wd = w.get_wind()
    w2.set_wind(ws, wd)
    ret = torch.zeros(B, dtype=torch.float64, device="cuda")
    g, prev = 1.0, ws
    for h in range(H):
        act = w2.lut_policy(0, want=("action",), as_torch=True)["action"]  # at the wind the env shows before the step
        w2.set_wind(wind[:, h, 0], wind[:, h, 1])
        w2.env_set_prev_wind(prev)
        r = w2.env_step(act, want=("reward",))["reward"]
        ret = ret + g * r.double()
        g, prev = g * GAMMA, wind[:, h, 0]
    b.record()
    b.synchronize()
    return a.elapsed_time(b), ret


def by_rows(w, ctl, H, series, out):
    """wind= gathered on the host: the cursor read back, the window indexed in NumPy, uploaded with the call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    cur = w.series_state()
    T = cur["T"]
    ticks = np.minimum(cur["t"] + 1 + np.arange(H), T - 1)
    rows = series[(cur["start"][:, None] + ticks[None, :]) % T]
    w.controller_returns(ctl, H, gamma=GAMMA, wind=torch.from_numpy(np.ascontiguousarray(rows)).cuda(), out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def workload(label, name, B, grid, H):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    ctl, params = WfStep.controller_grid(*grid)
    K = len(params)
    R = K * H
    rng = np.random.default_rng(7)
    table = steering_table(N, rng)
    ws0, wd0 = rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B)
    wind = swing(rng, B, H, ws0, wd0)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws0, wd0)
    w.env_config(**ENV)
    w.env_reset()
    w.set_yaw_table(table, TWD, TWS, interp="nearest")
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    w2 = WfStep(x, y, env_batch=B)  # the hand-written way's copy of the env
    w2.env_config(**ENV)
    w2.env_reset()
    w2.set_wind(ws0, wd0)
    w2.set_yaw_table(table, TWD, TWS, interp="nearest")
    wind_t = torch.from_numpy(wind).cuda()
    out = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda"), "best": torch.empty(B, dtype=torch.int32, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(gamma=GAMMA, wind=wind_t, out=out)
    for _ in range(2):
        w.controller_returns(ctl, H, **kw)
        w.rollout_timing()
        plain_loop_ms(w, w._rollout(), chunks, n_eval, load=True)
        python_way(w, w2, wind)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.controller_returns(ctl, H, **kw)
        total.append(w.rollout_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._rollout(), chunks, n_eval, load=True))
        ms, r_hand = python_way(w, w2, wind)
        hand.append(ms)
    w.rollout_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.controller_returns(ctl, H, **kw)
        det.append(w.rollout_timing())
    w.rollout_timing(detail=False)
    extra = w.controller_returns(ctl, H, gamma=GAMMA, wind=wind_t, want=("returns", "gated"))
    torch.cuda.synchronize()
    ret = out["returns"]
    rel = (ret - ret[:, :1]) / ret[:, :1].abs()
    agree = {"untuned_returns_max_abs_diff": float((ret[:, 0] - r_hand).abs().max().item()),
             "untuned_return_mean": float(ret[:, 0].mean().item()),
             "best_controller_share": np.bincount(out["best"].cpu().numpy(), minlength=K).astype(float).tolist(),
             "mean_gain_over_untuned_by_controller": rel.mean(dim=0).cpu().numpy().tolist(),
             "mean_gated_pairs_by_controller": extra["gated"].double().mean(dim=0).cpu().numpy().tolist()}
    kernels = w.rollout_kernel_info()
    # the series-ahead variant: the same farms on a series of 4 H rows, three ticks in
    T = 4 * H
    series = np.ascontiguousarray(swing(np.random.default_rng(9), 1, T, np.array([8.0]), np.array([268.0]))[0])
    w.set_wind_series(series, start=rng.integers(0, T, B).astype(np.int32))
    w.env_reset()
    for _ in range(3):
        w.wind_series_step()
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    ahead, rows = [], []
    for i in range(2 + REPS):
        w.controller_returns(ctl, H, gamma=GAMMA, wind="series", out=out)
        t_ahead = w.rollout_timing()["total_ms"]
        t_rows = by_rows(w, ctl, H, series, out)
        if i >= 2:
            ahead.append(t_ahead)
            rows.append(t_rows)
    w.close()
    w2.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    sa, sr = float(np.median(ahead)), float(np.median(rows))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "controllers": K, "horizon": H, "gamma": GAMMA,
         "grid": {"alpha": list(grid[0]), "deadband": list(grid[1]), "lead": list(grid[2])},
         "control": "continuous", "mode": "default", "wind": "per farm and per step", "rows_per_farm": R, "chunks": chunks,
         "evaluator_farms": n_eval, "reps": REPS,
         "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue, "glue_share_of_step": glue / step,
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "python_way_one_controller_ms": q, "python_way_one_controller_ms_min": float(np.min(hand)),
         "ratio_total_over_python_way_one_controller": t / q, "ratio_per_controller_over_python_way": t / K / q,
         "series_ahead_ms": sa, "series_by_rows_ms": sr, "ratio_series_ahead_over_by_rows": sa / sr,
         "farm_rollouts_per_s": B * K / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3), "results": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 8, H = 64, a wind per farm and step, default mode", "HornsRev1_", 256,
                    ([1.0, 0.3], [0.0, 5.0], [0, 1]), 64),
           workload("Ablaincourt x 4096, K = 16, H = 16, a wind per farm and step, default mode", "Ablaincourt_", 4096,
                    ([1.0, 0.5, 0.25, 0.1], [0.0, 5.0], [0, 1]), 16)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written lut_policy + env_step way alternate",
                   "workloads": res}, f, indent=1)
        f.write("\n")
