"""Stochastic model-predictive control on the device: the synthetic-wind example's row of three (64 farms, every farm under a
generated wind of its own, include/wfwindgen.h, one seed), controlled in a receding horizon — at every step a plan of H
steps is searched with the cross-entropy method, its first action applied, the mean shifted by one step — four ways, from
the same state, under the same winds, with the same planner seed:
    plan_actions, the wind held       the search under a persistence forecast with no uncertainty — blind
    plan_scenarios, expected return   every candidate scored over M wind futures drawn on the device from the episode's PROCESS,
                                      not from its realisation (include/wfscenplan.h): what a controller can know
    plan_scenarios, half on the tail  the same, with half the weight on the mean of the worst quarter of the futures
    plan_actions(wind="series")       the search under the rows the episode will play: perfect foresight — it cheats
The scenario planner is the baseline a learned wake-steering policy is compared with on wind_process episodes: it knows the
wind's law and nothing about its future.  Mean episode return, standard error over the farms and the count of farms ahead;
the figures are ILLUSTRATIVE, NOT A RESULT: one seed, one layout, one process.  The project's own definitions; PARITY
UNPINNED beyond the NumPy restatements.
Run from the repo root on an MI355X:  python examples/example_scenario_mpc.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, E, M, H, STEPS, GAMMA = 64, 32, 6, 8, 6, 24, 0.97
N = len(x)
T = STEPS + 2  # ticks: tick 0, one for the reset's tick, one per step
SEED = 7
PROCESS = dict(ws_revert=0.1, ws_sigma=0.1, wd_revert=0.5, wd_sigma=0.3, wd_ramp=1.5)
DIST = dict(ws_scale=8.5, ws_shape=20.0, ws_lo=6.0, ws_hi=11.0, wd_mean=270.0, wd_std=8.0, wd_lo=240.0, wd_hi=300.0)


def episode(w, plan):
    """One episode from zero yaw at tick 0 of the same generated series: episode return (B,)."""
    w.generate_wind(T, SEED, PROCESS, dist=DIST)  # the same seed: the same bits
    w.env_reset()
    w.wind_series_step()  # what VecWindFarmEnv.reset does: a tick, then the warm-up solve
    w.env_step(None, want=("yaw",))
    total = torch.zeros(B, dtype=torch.float64, device="cuda")
    mean = torch.zeros((B, H, N), dtype=torch.float32, device="cuda")
    for t in range(STEPS):
        r = plan(w, mean, t)  # BEFORE the tick
        mean = torch.cat([r["mean"][:, 1:], r["mean"][:, -1:]], dim=1).contiguous()  # the receding horizon: shifted by one step
        w.wind_series_step()  # the env ticks, then steps
        total += w.env_step(r["first_action"].contiguous(), want=("reward",))["reward"].double()
    return total.cpu().numpy()


def planner(wind):
    def plan(w, mean, t):
        return w.plan_actions(H, candidates=K, elites=E, seed=100 + t, gamma=GAMMA, wind=wind, mean=mean, want=("first_action", "mean"))
    return plan


def scenario_planner(weight):
    def plan(w, mean, t):
        return w.plan_scenarios(H, candidates=K, elites=E, members=M, process=PROCESS, seed=100 + t, scenario_seed=1000 + t, gamma=GAMMA,
                                tail=M // 4, risk_weight=weight, bounds=(DIST["ws_lo"], DIST["ws_hi"]), mean=mean,
                                want=("first_action", "mean"))
    return plan


PLANNERS = (
    ("plan_actions, the wind held", planner(None)),
    (f"plan_scenarios, {M} futures, expected return", scenario_planner(0.0)),
    (f"plan_scenarios, {M} futures, half on the worst {M // 4}", scenario_planner(0.5)),
    ('plan_actions(wind="series") (foresight)', planner("series")),
)

w = WfStep(x, y, env_batch=B)
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
ret = {label: episode(w, plan) for label, plan in PLANNERS}
rows = w.generated_wind()  # (B, T, 2): what the farms saw

print(f"{B} farms of a row of three, 5 D apart; {STEPS} steps, H = {H}, K = {K} candidates, {E} elites, 3 iterations per step, gamma = {GAMMA}")
print(f"generated winds (seed {SEED}): speed {rows[:, :, 0].min():.2f} .. {rows[:, :, 0].max():.2f} m/s, direction at tick 0 "
      f"{rows[:, 0, 1].min():.1f} .. {rows[:, 0, 1].max():.1f} deg")
held = ret[PLANNERS[0][0]]
for label, _ in PLANNERS:
    r = ret[label]
    gain = r - held
    print(f"{label:>48}: episode return mean {r.mean():.4f}, std over the farms {r.std(ddof=1):.4f}; against holding "
          f"{gain.mean():+.4f} (standard error {gain.std(ddof=1) / np.sqrt(B):.4f}), ahead on {(gain > 0).sum()} of {B} farms")
print("illustrative, not a result: one seed, one layout, one process.  last scenario plan:", w.plan_scenarios_timing(),
      w.plan_scenarios_kernel_info())
w.close()
