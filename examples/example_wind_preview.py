"""Planning with a preview of the wind, on a time-series episode: the row of three turbines of example_device_planner.py (5 D
apart) under a wind whose direction ramps from 20 deg off the row onto the row and on to the other side, 1.5 deg per step.
The yaw that pays changes sign while the wind turns, a yaw moves at most 5 deg per step and the actuation budget then
silences the turbine for a while: a planner that holds the CURRENT wind over its horizon steers for a wind that is gone by
the time the yaw arrives.  The series, every farm's start row and the tick live on the device; wind="series" lets
backend.WfStep.plan_actions (include/wfplan.h) solve step h of its horizon under the series' row of tick t + 1 + h, read by
one kernel, no host round trip (include/wfseries.h) — and wind_preview(H) is the same window as an observation, what a
feed-forward controller would be given.  Both planners run the same episode from the same state with the same draws; the
output is illustrative.  The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_wind_preview.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, E, H, STEPS, GAMMA = 4, 64, 8, 6, 24, 0.97  # four farms = four independent runs of the planner (their draws differ)
N = len(x)
T = STEPS + 2  # rows: one for the series' own first tick, one for the reset's tick, one per step
series = np.stack([np.full(T, 8.0), 250.0 + 1.5 * np.arange(T)], axis=1)  # the direction ramp: 250 deg .. 287.5 deg
WANT = ("first_action", "mean", "plan_return", "hold_return")


def episode(w, wind, seed):
    """One episode from zero yaw at the series' start: (episode return (B,), final yaw (B, N))."""
    w.set_wind_series(series, start=np.zeros(B, np.int32))
    w.env_reset()
    w.wind_series_step()  # what VecWindFarmEnv.reset does: a tick, then the warm-up solve
    w.env_step(None, want=("yaw",))
    total = torch.zeros(B, dtype=torch.float64, device="cuda")
    mean = torch.zeros((B, H, N), dtype=torch.float32, device="cuda")
    for t in range(STEPS):
        plan = w.plan_actions(H, candidates=K, elites=E, seed=seed + t, gamma=GAMMA, wind=wind, mean=mean, want=WANT)  # BEFORE the tick
        w.wind_series_step()  # the env ticks, then steps
        total += w.env_step(plan["first_action"], want=("reward",))["reward"].double()
        mean = torch.cat([plan["mean"][:, 1:], plan["mean"][:, -1:]], dim=1)  # the receding horizon: shifted by one step
    return total, torch.as_tensor(w.env_get_state()["yaw"])


w = WfStep(x, y, env_batch=B)
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
results = {label: episode(w, wind, seed=1) for label, wind in (("holding the current wind", None), ('wind="series"', "series"))}
preview, available = w.wind_preview(4, as_torch=True)  # at the end of the episode: nothing is left, the last row held

print(f"row of three, 5 D apart, 8 m/s, the direction ramping 250 -> {series[-1, 1]:.1f} deg by 1.5 deg per step; {STEPS} steps, "
      f"H = {H}, K = {K} candidates, {E} elites, 3 iterations per step, gamma = {GAMMA}")
for label, (total, yaw) in results.items():
    print(f"{label:>26}: episode return {total.mean().item():.4f} (farms: {[round(v, 4) for v in total.tolist()]}), "
          f"final yaw of farm 0 {[round(v, 1) for v in yaw[0].tolist()]}")
held, ahead = (results[k][0].mean().item() for k in results)
print(f"the preview is worth {ahead - held:+.4f} of episode return ({(ahead / held - 1.0) * 100.0:+.2f} %)")
print(f"wind_preview(4) after the last step: {available} rows left, directions {preview[0, :, 1].tolist()}")
print("last planning run:", w.plan_timing(), w.series_kernel_info())
w.close()
