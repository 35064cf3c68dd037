"""Planning under a wind that changes, on a synthetic wind episode: 64 farms of the row of three turbines of
example_wind_preview.py (5 D apart), every farm under a wind realisation of ITS OWN — generated on the device from one seed
(include/wfwindgen.h): a mean-reverting speed around 8 m/s, a direction that starts near the row's axis and ramps at a rate the
farm draws from +-1.5 deg per step, with a little noise on both.  example_wind_preview.py makes its point on one hand-made
series; here the same comparison is a sample of 64: backend.WfStep.plan_actions with wind="series" — step h of the horizon
solved under the farm's own row of tick t + 1 + h, read by one kernel — against the same planner holding the current wind,
from the same state, under the same winds and with the same draws.  Mean and spread over the farms; the output is
ILLUSTRATIVE, not a result.  The project's own definitions; PARITY UNPINNED beyond the NumPy restatement.
Run from the repo root on an MI355X:  python examples/example_synthetic_wind.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, E, H, STEPS, GAMMA = 64, 64, 8, 6, 24, 0.97
N = len(x)
T = STEPS + 2  # ticks: tick 0, one for the reset's tick, one per step
SEED = 7
PROCESS = dict(ws_revert=0.1, ws_sigma=0.1, wd_revert=0.5, wd_sigma=0.3, wd_ramp=1.5)
DIST = dict(ws_scale=8.5, ws_shape=20.0, ws_lo=6.0, ws_hi=11.0, wd_mean=270.0, wd_std=8.0, wd_lo=240.0, wd_hi=300.0)
WANT = ("first_action", "mean", "plan_return", "hold_return")


def episode(w, wind, seed):
    """One episode from zero yaw at tick 0 of the same generated series: episode return (B,)."""
    w.generate_wind(T, SEED, PROCESS, dist=DIST)  # the same seed: the same bits
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
    return total.cpu().numpy()


w = WfStep(x, y, env_batch=B)
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
held = episode(w, None, seed=1)
ahead = episode(w, "series", seed=1)
rows = w.generated_wind()  # (B, T, 2): what the farms saw
turn = rows[:, -1, 1] - rows[:, 0, 1]
turn = (turn + 180.0) % 360.0 - 180.0
gain = ahead - held

print(f"{B} farms of a row of three, 5 D apart; {STEPS} steps, H = {H}, K = {K} candidates, {E} elites, gamma = {GAMMA}")
print(f"generated winds (seed {SEED}): speed {rows[:, :, 0].min():.2f} .. {rows[:, :, 0].max():.2f} m/s, direction at tick 0 "
      f"{rows[:, 0, 1].min():.1f} .. {rows[:, 0, 1].max():.1f} deg, turned by {turn.min():+.1f} .. {turn.max():+.1f} deg over the episode")
for label, r in (("holding the current wind", held), ('wind="series"', ahead)):
    print(f"{label:>26}: episode return mean {r.mean():.4f}, std over the farms {r.std(ddof=1):.4f}, min {r.min():.4f}, max {r.max():.4f}")
print(f"the preview is worth {gain.mean():+.4f} of episode return on average ({(ahead.mean() / held.mean() - 1.0) * 100.0:+.2f} %), "
      f"std over the farms {gain.std(ddof=1):.4f}, standard error {gain.std(ddof=1) / np.sqrt(B):.4f}; ahead on {(gain > 0).sum()} of {B} farms")
fast = np.abs(turn) > np.median(np.abs(turn))
print(f"farms whose wind turned more than the median ({np.median(np.abs(turn)):.1f} deg): {gain[fast].mean():+.4f}; the others: {gain[~fast].mean():+.4f}")
print("illustrative: one seed, one layout, one process.  last planning run:", w.plan_timing(), w.windgen_kernel_info())
w.close()
