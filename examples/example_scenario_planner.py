"""Planning under a wind that is known only as a process: the synthetic-wind example's row of three (64 farms, every farm
under a generated wind of its own, include/wfwindgen.h), controlled by receding-horizon random shooting — K random action
sequences per farm and step, the first action of the best one applied — with the candidates scored three ways, from the same
state, under the same winds and with the same candidates:
    holding the current wind     lookahead_returns(wind=None): a persistence forecast with no uncertainty — blind
    an ensemble of wind futures  scenario_returns: M paths per farm drawn on the device from the episode's PROCESS, not from its
                                 realisation (include/wfscenario.h), the candidates picked by expected return, or by a score
                                 that weighs in the mean of the worst quarter of the members
    the rows the episode plays   lookahead_returns(wind="series"): perfect foresight — it cheats
The ensemble planner is the baseline a controller is held to under uncertainty: it knows what the other two know about the
wind's law and nothing about its future.  Mean and spread over the farms; the figures are ILLUSTRATIVE, NOT A RESULT: one
seed, one layout, one process.  The project's own definitions; PARITY UNPINNED beyond the NumPy restatements.
Run from the repo root on an MI355X:  python examples/example_scenario_planner.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, K, M, H, STEPS, GAMMA = 64, 32, 8, 6, 24, 0.97
N = len(x)
T = STEPS + 2  # ticks: tick 0, one for the reset's tick, one per step
SEED = 7
PROCESS = dict(ws_revert=0.1, ws_sigma=0.1, wd_revert=0.5, wd_sigma=0.3, wd_ramp=1.5)
DIST = dict(ws_scale=8.5, ws_shape=20.0, ws_lo=6.0, ws_hi=11.0, wd_mean=270.0, wd_std=8.0, wd_lo=240.0, wd_hi=300.0)


def episode(w, pick):
    """One episode from zero yaw at tick 0 of the same generated series, the same candidates at every step: episode return (B,)."""
    w.generate_wind(T, SEED, PROCESS, dist=DIST)  # the same seed: the same bits
    w.env_reset()
    w.wind_series_step()  # what VecWindFarmEnv.reset does: a tick, then the warm-up solve
    w.env_step(None, want=("yaw",))
    gen = torch.Generator(device="cuda").manual_seed(1)
    total = torch.zeros(B, dtype=torch.float64, device="cuda")
    rows = torch.arange(B, device="cuda")
    for t in range(STEPS):
        cand = (torch.rand((B, K, H, N), generator=gen, device="cuda") * 10.0 - 5.0).contiguous()
        cand[:, 0] = 0.0  # holding still is always a candidate
        best = pick(w, cand, t).long()  # BEFORE the tick
        w.wind_series_step()  # the env ticks, then steps
        total += w.env_step(cand[rows, best, 0].contiguous(), want=("reward",))["reward"].double()
    return total.cpu().numpy()


def scenario(weight):
    def pick(w, cand, t):
        return w.scenario_returns(cand, M, PROCESS, seed=1000 + t, gamma=GAMMA, tail=M // 4, risk_weight=weight,
                                  bounds=(DIST["ws_lo"], DIST["ws_hi"]), want="best")["best"]
    return pick


PLANNERS = (
    ("holding the current wind", lambda w, cand, t: w.lookahead_returns(cand, gamma=GAMMA, want="best")["best"]),
    (f"{M} wind futures, expected return", scenario(0.0)),
    (f"{M} wind futures, half on the worst {M // 4}", scenario(0.5)),
    ('wind="series" (foresight)', lambda w, cand, t: w.lookahead_returns(cand, gamma=GAMMA, wind="series", want="best")["best"]),
)

w = WfStep(x, y, env_batch=B)
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
ret = {label: episode(w, pick) for label, pick in PLANNERS}
rows = w.generated_wind()  # (B, T, 2): what the farms saw

print(f"{B} farms of a row of three, 5 D apart; {STEPS} steps, H = {H}, K = {K} random sequences per step, gamma = {GAMMA}")
print(f"generated winds (seed {SEED}): speed {rows[:, :, 0].min():.2f} .. {rows[:, :, 0].max():.2f} m/s, direction at tick 0 "
      f"{rows[:, 0, 1].min():.1f} .. {rows[:, 0, 1].max():.1f} deg")
held = ret[PLANNERS[0][0]]
for label, _ in PLANNERS:
    r = ret[label]
    gain = r - held
    print(f"{label:>34}: episode return mean {r.mean():.4f}, std over the farms {r.std(ddof=1):.4f}; against holding "
          f"{gain.mean():+.4f} (standard error {gain.std(ddof=1) / np.sqrt(B):.4f}), ahead on {(gain > 0).sum()} of {B} farms")
print("illustrative, not a result: one seed, one layout, one process.  last scenario run:", w.scenario_timing(), w.scenario_kernel_info())
w.close()
