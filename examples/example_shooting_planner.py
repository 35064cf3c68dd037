"""A receding-horizon random-shooting planner in the simulator, on a row of three turbines 5 D apart under (8 m/s, 270 deg):
at every step K candidate action sequences of H steps are scored by their discounted return from the env's CURRENT state
(backend.WfStep.lookahead_returns, include/wflookahead.h: the K H farm solves of a farm are rows of one batched step on the
device; VecWindFarmEnv.lookahead_returns is the same call on a batched env), and the first action of the best one is
executed.  The yaw moves at most 5 deg per step and the actuation budget then silences a turbine for a while, so steering
the front turbines towards the wake-steering optimum takes several steps.  The GREEDY planner (H = 1) scores one step, the
other one (H = 6) the manoeuvre; both are compared with the optimum of `optimize_yaw`, which ignores the actuator.  Which
of the two collects more depends on K, H, gamma and the candidates drawn: the output is illustrative.  The project's own
definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_shooting_planner.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, STEPS, GAMMA = 4, 64, 24, 0.97  # four farms = four independent runs of the planner
N = len(x)


def episode(w, horizon, seed):
    """One episode of the planner with look-ahead `horizon` from zero yaw: (episode return (B,), final yaw (B, N), final farm
    power (B,) W)."""
    w.env_reset()
    gen = torch.Generator().manual_seed(seed)
    total = torch.zeros(B, dtype=torch.float64, device="cuda")
    rows = torch.arange(B, device="cuda")
    for _ in range(STEPS):
        # candidates: one random joint action held over the horizon, jittered per step; sequence 0 holds
        first = torch.rand((B, K, 1, N), generator=gen) * 10.0 - 5.0
        seqs = (first + torch.randn((B, K, horizon, N), generator=gen)).clamp(-5.0, 5.0)
        seqs[:, 0] = 0.0
        seqs = seqs.cuda()
        plan = w.lookahead_returns(seqs, gamma=GAMMA)  # BEFORE the step; the env state is read, never changed
        action = seqs[rows, plan["best"].long(), 0]  # execute the first action of the best sequence, then plan again
        out = w.env_step(action, want=("reward", "power"))
        total += out["reward"].double()
    return total, torch.as_tensor(w.env_get_state()["yaw"]), out["power"].double().sum(dim=1)


w = WfStep(x, y, env_batch=B)
w.set_wind(8.0, 270.0)  # along the row: turbine 0 is upstream
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
results = {label: episode(w, horizon, seed=1) for label, horizon in (("greedy (H = 1)", 1), ("look-ahead (H = 6)", 6))}
opt = w.optimize_yaw(np.zeros((B, N), np.float32))  # the optimum of the steady problem: no actuator, no budget

print(f"row of three, 5 D apart, 8 m/s along the row; {STEPS} steps, K = {K} candidate sequences per step, gamma = {GAMMA}")
print("optimize_yaw (no actuator): yaw", [round(float(v), 1) for v in opt["yaw"][0]],
      f"farm power {float(opt['power'][0]) / 1e6:.3f} MW (at zero yaw {float(opt['power_initial'][0]) / 1e6:.3f} MW)")
for label, (total, yaw, power) in results.items():
    print(f"{label:>20}: episode return {total.mean().item():.4f} (farms: {[round(v, 4) for v in total.tolist()]}), "
          f"final yaw of farm 0 {[round(v, 1) for v in yaw[0].tolist()]}, final farm power {power.mean().item() / 1e6:.3f} MW")
print("last look-ahead run:", w.lookahead_timing(), w.lookahead_kernel_info())
w.close()
