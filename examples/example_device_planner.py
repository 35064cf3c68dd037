"""A receding-horizon planner that runs on the device, on the row of three turbines of example_shooting_planner.py (5 D apart
under 8 m/s along the row): at every env step ONE call plans for every farm — the cross-entropy method over K candidate
action sequences of H steps, I iterations of draw, score and refit with one glue kernel between two batched steps and no
host read (backend.WfStep.plan_actions, include/wfplan.h; VecWindFarmEnv.plan_actions is the same call on a batched env) —,
the first action of the plan is executed, and the mean, shifted by one step, warm-starts the next call.  The shooting
example draws its candidates with torch on the host and scores them once; this one refines them on the device under the
env's own transition: the yaw moves at most 5 deg per step and the actuation budget then silences a turbine for a while.
Both planners are compared with the optimum of `optimize_yaw`, which ignores the actuator.  The output is illustrative.
The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_device_planner.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, E, STEPS, GAMMA = 4, 64, 8, 24, 0.97  # four farms = four independent runs of the planner (their draws differ)
N = len(x)
WANT = ("first_action", "mean", "plan_return", "hold_return")


def episode(w, horizon, seed):
    """One episode of the planner with look-ahead `horizon` from zero yaw: (episode return (B,), final yaw (B, N), final farm
    power (B,) W, mean gain of the last plan over holding)."""
    w.env_reset()
    total = torch.zeros(B, dtype=torch.float64, device="cuda")
    mean = torch.zeros((B, horizon, N), dtype=torch.float32, device="cuda")
    for t in range(STEPS):
        plan = w.plan_actions(horizon, candidates=K, elites=E, seed=seed + t, gamma=GAMMA, mean=mean, want=WANT)  # BEFORE the step
        out = w.env_step(plan["first_action"], want=("reward", "power"))  # execute the plan's first action, then plan again
        total += out["reward"].double()
        mean = torch.cat([plan["mean"][:, 1:], plan["mean"][:, -1:]], dim=1)  # the receding horizon: shifted by one step
    gain = (plan["plan_return"] - plan["hold_return"]).mean().item()
    return total, torch.as_tensor(w.env_get_state()["yaw"]), out["power"].double().sum(dim=1), gain


w = WfStep(x, y, env_batch=B)
w.set_wind(8.0, 270.0)  # along the row: turbine 0 is upstream
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
results = {label: episode(w, horizon, seed=1) for label, horizon in (("greedy (H = 1)", 1), ("look-ahead (H = 6)", 6))}
opt = w.optimize_yaw(np.zeros((B, N), np.float32))  # the optimum of the steady problem: no actuator, no budget

print(f"row of three, 5 D apart, 8 m/s along the row; {STEPS} steps, K = {K} candidates, {E} elites, 3 iterations per step, gamma = {GAMMA}")
print("optimize_yaw (no actuator): yaw", [round(float(v), 1) for v in opt["yaw"][0]],
      f"farm power {float(opt['power'][0]) / 1e6:.3f} MW (at zero yaw {float(opt['power_initial'][0]) / 1e6:.3f} MW)")
for label, (total, yaw, power, gain) in results.items():
    print(f"{label:>20}: episode return {total.mean().item():.4f} (farms: {[round(v, 4) for v in total.tolist()]}), "
          f"final yaw of farm 0 {[round(v, 1) for v in yaw[0].tolist()]}, final farm power {power.mean().item() / 1e6:.3f} MW, "
          f"last plan's gain over holding {gain:.4f}")
print("last planning run:", w.plan_timing(), w.plan_kernel_info())
w.close()
