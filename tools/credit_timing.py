"""Per-agent counterfactual rewards on the device (csrc/credit/, include/wfcredit.h): what the difference rewards of every
farm cost, next to the step calls they are made of and next to the way a user had to write them before — and how accurate a
default-mode difference is on a large farm.  Writes profiles/credit_timing.json.

One MI355X, HIP events on the handle's stream.  The parent is a fused env (env_config, env_reset, three random env steps, so
that accumulators and gates are live), a wind per farm; base = the joint ACTION, alternatives = actions as well:
    HornsRev1 x 256 farms, K = 1 (hold), continuous control, default mode and strict
    Ablaincourt x 4096 farms, K = 3 (down / hold / up by 1 deg), discrete control, default mode
Per configuration, after 2 warm-up runs (the first builds the evaluator and times its kernel families):
    total_ms   median of `reps` runs of counterfactual_rewards — reward and difference, torch tensors in and out —, two
               events per run (first to last launch)
    step_ms / glue_ms   median of `reps` more runs with four events per chunk; glue = lay-out + reduce kernels
    plain_loop_ms   the same number of wf_step calls (power and load) on the object's OWN evaluator handle, nothing between
    python_way_ms   what a user wrote before this extension: a second WfStep of B (1 + N K) farms; the env's gate and clip
               restated in torch to lay out the rows, the winds repeated and set, one step, the reward and the differences
               reduced in torch float64 — every call; the three alternate
    kernels    wf_credit_kernel_info: vgprs / static LDS bytes / private-segment bytes
ACCURACY (the last entry): HornsRev1, 4 farms (yawopt_ref.gpu_case), base yaw uniform in [-20, 20] (seed 51, farm 0 at zero),
K = 2 (zero yaw; clip(yaw + 5, +-25)), load_coef 0.1, against tests/credit_ref.py over the float64 oracle: max |D_dev - D_ref|
in the default mode and strict, next to the contract's bound on a difference and the median |D|.
Run from the repo root on an MI355X:  python tools/credit_timing.py [reps, default 10] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools.ext_timing import plain_loop_ms  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
LAYOUTS = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "credit_timing.json")
ENV = dict(yaw_lo=-40.0, yaw_hi=40.0, actuator_rate=0.3, dt=60.0, budget=0.1, load_coef=0.1)
YAW_STEP = {False: 5.0, True: 1.0}  # discrete: 1 deg, a step the actuation budget (1.8 deg per env step) leaves every gate open for
GRAD_GLUE_SHARE = {"HornsRev1_": 0.0112, "Ablaincourt_": 0.139}  # profiles/grad_timing.json: glue over step time


def torch_transition(st, a, discrete):
    """The fused step's gate, increment and clip restated in torch (tensor / tensor divisions: a Python scalar would be
    turned into a multiplication by its reciprocal)."""
    c = torch.tensor([ENV["actuator_rate"], ENV["dt"], ENV["budget"]], dtype=torch.float32, device=a.device)
    shape = (-1, 1) + (1,) * (a.dim() - 2)
    y, acc = st["yaw"].reshape(a.shape[:2] + shape[2:]), st["acc"].reshape(a.shape[:2] + shape[2:])
    frac = acc / c[0] / (st["moves"] + 1).float().reshape(shape) / c[1]
    a = torch.where(frac >= c[2], torch.zeros_like(a), a)
    a = (a - 1.0) * YAW_STEP[discrete] if discrete else a.clamp(-YAW_STEP[discrete], YAW_STEP[discrete])
    return (y + a).clamp(ENV["yaw_lo"], ENV["yaw_hi"])


def python_way(w, w2, actions, alt, discrete):
    """Difference rewards with the API the project had before: rows laid out in torch, one step of a B R handle, torch sums."""
    B, N, K = alt.shape
    R = 1 + N * K
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = w.env_get_state(as_torch=True)
    ws, wd = w.get_wind(as_torch=True)
    base, ya = torch_transition(st, actions, discrete), torch_transition(st, alt, discrete)
    blk = base[:, None, :].repeat(1, R, 1)
    blk[:, torch.arange(1, R, device=blk.device), torch.arange(N, device=blk.device).repeat_interleave(K)] = ya.reshape(B, N * K)
    w2.set_wind(ws.repeat_interleave(R), wd.repeat_interleave(R))
    out = w2.step(blk.reshape(B * R, N))
    psum = out["power"].double().sum(dim=1)
    lsum = out["load"].double().abs().reshape(B * R, 4 * N).sum(dim=1)
    wr = ws.repeat_interleave(R)
    r = (psum / N / 1.0e6 * 1.0e3 / (wr * wr * wr) - float(np.float32(ENV["load_coef"])) * lsum / (4.0 * N)).reshape(B, R)
    diff = (r[:, :1] - r[:, 1:]).reshape(B, N, K)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r, diff


def workload(label, name, B, K, discrete, strict):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    R = 1 + N * K
    rng = np.random.default_rng(7)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(0.0, 360.0, B))
    w.env_config(discrete=discrete, yaw_step=YAW_STEP[discrete], **ENV)
    w.env_reset()

    def draw():
        a = rng.integers(0, 3, (B, N)) if discrete else rng.uniform(-5.0, 5.0, (B, N))
        return torch.from_numpy(a.astype(np.float32)).cuda()

    for _ in range(3):
        w.env_step(draw(), want=("reward",))
    actions = draw()
    alt = torch.from_numpy(np.broadcast_to(np.float32([0.0, 1.0, 2.0]) if discrete else np.float32([0.0]), (B, N, K)).copy()).cuda()
    w2 = WfStep(x, y, env_batch=B * R)  # the hand-written way's second handle
    w2.set_risk_resolve(2 if strict else 1)
    out = {"reward": torch.empty((B, R), dtype=torch.float64, device="cuda"), "difference": torch.empty((B, N, K), dtype=torch.float64, device="cuda")}
    per_chunk = min(B, 65536 // R)
    chunks = -(-B // per_chunk)
    n_eval = per_chunk * R
    kw = dict(base_kind="action", alt_kind="action", strict=strict, out=out)
    for _ in range(2):
        w.counterfactual_rewards(actions, alt, **kw)
        w.credit_timing()
        plain_loop_ms(w, w._credit(), chunks, n_eval, load=True)
        python_way(w, w2, actions, alt, discrete)
    total, plain, hand = [], [], []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        w.counterfactual_rewards(actions, alt, **kw)
        total.append(w.credit_timing()["total_ms"])
        plain.append(plain_loop_ms(w, w._credit(), chunks, n_eval, load=True))
        ms, r_hand, d_hand = python_way(w, w2, actions, alt, discrete)
        hand.append(ms)
    w.credit_timing(detail=True)
    det = []
    for _ in range(REPS):
        w.counterfactual_rewards(actions, alt, **kw)
        det.append(w.credit_timing())
    w.credit_timing(detail=False)
    torch.cuda.synchronize()
    agree = {"reward_max_abs_diff": float((out["reward"] - r_hand).abs().max().item()),
             "difference_max_abs_diff": float((out["difference"] - d_hand).abs().max().item()),
             "difference_median_abs": float(out["difference"].abs().median().item())}
    kernels = w.credit_kernel_info()
    w.close()
    w2.close()
    t, p, q = float(np.median(total)), float(np.median(plain)), float(np.median(hand))
    step, glue = float(np.median([d["step_ms"] for d in det])), float(np.median([d["glue_ms"] for d in det]))
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "alternatives": K, "control": "discrete" if discrete else "continuous",
         "mode": "strict" if strict else "default", "wind": "per farm", "rows_per_farm": R, "chunks": chunks, "evaluator_farms": n_eval,
         "reps": REPS, "total_ms": t, "total_ms_min": float(np.min(total)), "total_ms_max": float(np.max(total)),
         "total_detail_ms": float(np.median([d["total_ms"] for d in det])), "step_ms": step, "glue_ms": glue,
         "glue_share_of_step": glue / step, "grad_glue_share_of_step": GRAD_GLUE_SHARE[name],
         "plain_loop_ms": p, "plain_loop_ms_min": float(np.min(plain)), "ratio_total_over_plain_loop": t / p,
         "python_way_ms": q, "python_way_ms_min": float(np.min(hand)), "ratio_total_over_python_way": t / q,
         "farm_credits_per_s": B / (t * 1e-3), "farm_steps_per_s": B * R / (t * 1e-3), "against_python_way": agree, "kernels": kernels}
    print(json.dumps(r), flush=True)
    return r


def accuracy():
    import credit_ref
    import parity
    import yawopt_ref

    x, y, ws, wd = yawopt_ref.gpu_case(yawopt_ref.layouts(), "HornsRev1_", n_farms=4)
    B, N, lc = 4, len(x), 0.1
    rng = np.random.default_rng(51)
    yaw = rng.uniform(-20.0, 20.0, (B, N)).astype(np.float32)
    yaw[0] = 0.0
    alt = np.stack([np.zeros_like(yaw), np.clip(yaw + np.float32(5.0), -25.0, 25.0).astype(np.float32)], axis=2)
    ref = credit_ref.counterfactual(x, y, ws, wd, yaw, alt, lc)
    live = ~ref["same"]
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    w.env_config(load_coef=lc)
    r = {"workload": "accuracy of a difference: HornsRev1 x 4, K = 2, load_coef 0.1, against the float64 oracle", "turbines": N, "farms": B,
         "median_abs_difference": float(np.median(np.abs(ref["difference"][live])))}
    for tag, strict, tol in (("default", False, parity.TOL), ("strict", True, parity.TOL_F64)):
        got = w.counterfactual_rewards(yaw, alt, strict=strict)
        b = credit_ref.bound(ref["out"], ref["wr_rows"], lc, tol).reshape(B, -1)
        db = (b[:, :1] + b[:, 1:]).reshape(B, N, 2)
        err = np.abs(got["difference"] - ref["difference"])
        r[tag] = {"max_abs_error": float(err[live].max()), "median_abs_error": float(np.median(err[live])),
                  "median_bound": float(np.median(db[live])), "max_error_over_bound": float((err[live] / db[live]).max()),
                  "max_abs_error_over_median_abs_difference": float(err[live].max() / r["median_abs_difference"]),
                  "reward_max_abs_error": float(np.abs(got["reward"] - ref["reward"]).max())}
    w.close()
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 1 (hold), a wind per farm, default mode", "HornsRev1_", 256, 1, False, False),
           workload("HornsRev1 x 256, K = 1 (hold), a wind per farm, strict", "HornsRev1_", 256, 1, False, True),
           workload("Ablaincourt x 4096, K = 3 (down / hold / up), a wind per farm, default mode", "Ablaincourt_", 4096, 3, True, False)]
    acc = accuracy()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up runs, median of `reps`; "
                   "device call, plain wf_step loop on the evaluator and the hand-written torch way alternate",
                   "workloads": res, "accuracy": acc}, f, indent=1)
        f.write("\n")
