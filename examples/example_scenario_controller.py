"""Tuning and selecting yaw-table controllers under a wind PROCESS: the synthetic-wind example's row of three (every farm under a
generated wind of its own, include/wfwindgen.h).  The yaw look-up table comes from the project's coordinate search
(backend.WfStep.build_yaw_table); a controller filters the wind with gain alpha, holds inside a deadband and may preview `lead`
steps (include/wfrollout.h).  controller_scenarios (include/wfrollscen.h) runs a whole grid of such controllers in closed loop
under M wind futures drawn on the device from the process, per farm, from the farm's own state, in ONE call.
  (a) tuning   a 4 x 4 x 2 grid, H steps from the reset state of farm 0: the winner by EXPECTED return over M = 16 futures
               against the winner on ONE realisation — controller_returns(wind="series") on farm 0's own series, which uses that
               realisation's foresight.  Both winners are then replayed through env_step on 64 fresh realisations.
  (b) selecting   a receding horizon over the policy class: at every step every farm takes the first action of ITS best
               controller by expected return (the filters restart at the current wind at every call), against the best FIXED
               controller without preview, on the same fresh realisations.  The selector picks among the 16 controllers with
               lead 0 only: their first action is the same under every member, so it can be executed; a controller with lead 1
               previews its own member's future inside each scenario — a perfect forecast there —, its `first_action` is member
               0's, and in the replays of (a) it previews the realisation's.
Mean episode return, standard error over the farms and the count of farms ahead; the figures are ILLUSTRATIVE, NOT A RESULT:
one seed, one layout, one process.  The project's own definitions; PARITY UNPINNED beyond the NumPy restatements.
Run from the repo root on an MI355X:  python examples/example_scenario_controller.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, M, H, STEPS, GAMMA = 64, 16, 8, 24, 0.97
N = len(x)
T = STEPS + 2  # ticks: tick 0, one for the reset's tick, one per step
TUNE_SEED, FRESH_SEED = 7, 8
PROCESS = dict(ws_revert=0.1, ws_sigma=0.1, wd_revert=0.5, wd_sigma=0.3, wd_ramp=1.5)
DIST = dict(ws_scale=8.5, ws_shape=20.0, ws_lo=6.0, ws_hi=11.0, wd_mean=270.0, wd_std=8.0, wd_lo=240.0, wd_hi=300.0)
BOUNDS = (DIST["ws_lo"], DIST["ws_hi"])


def start(w, seed):
    """Zero yaw at tick 1 of the series generated from `seed`: what VecWindFarmEnv.reset does."""
    w.generate_wind(T, seed, PROCESS, dist=DIST)
    w.env_reset()
    w.wind_series_step()
    w.env_step(None, want=("yaw",))


def one(params):
    return {k: np.array([params[k]]) for k in ("slot", "alpha", "deadband", "lead")}


def replay(w, seed, params):
    """Episode return (B,) of one fixed controller on the realisations of `seed`, its actions stepped through env_step."""
    start(w, seed)
    actions = w.controller_returns(one(params), STEPS, wind="series", want=("actions",))["actions"]  # BEFORE step: nothing changes
    total = np.zeros(B)
    for t in range(STEPS):
        w.wind_series_step()
        total += w.env_step(actions[:, 0, t].copy(), want=("reward",))["reward"]
    return total


def select(w, seed, grid):
    """Episode return (B,) of the receding-horizon selector, and how often each controller was picked."""
    start(w, seed)
    total, picks = np.zeros(B), np.zeros(len(grid["alpha"]), int)
    for t in range(STEPS):
        r = w.controller_scenarios(grid, H, M, PROCESS, seed=1000 + t, gamma=GAMMA, bounds=BOUNDS, want=("first_action", "best"))
        picks += np.bincount(r["best"], minlength=picks.size)
        w.wind_series_step()
        total += w.env_step(r["first_action"][np.arange(B), r["best"]].copy(), want=("reward",))["reward"]
    return total, picks


w = WfStep(x, y, env_batch=B)
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
wd_axis, ws_axis = np.arange(235.0, 305.1, 2.5), np.array([6.0, 8.5, 11.0])
w.set_wind(8.5, 270.0)
table = w.build_yaw_table(wd_axis, ws_axis)  # the optimiser ignores the actuator: the steady optimum per (direction, speed)
w.set_yaw_table(table["table"], wd_axis, ws_axis, interp="linear")
grid, params = WfStep.controller_grid([1.0, 0.5, 0.25, 0.1], [0.0, 2.5, 5.0, 7.5], [0, 1])

# (a) the same grid tuned two ways from farm 0's reset state
start(w, TUNE_SEED)
ens = w.controller_scenarios(grid, H, M, PROCESS, seed=1, gamma=GAMMA, bounds=BOUNDS, farms=[0], want=("expected_returns", "cvar", "best"))
real = w.controller_returns(grid, H, gamma=GAMMA, wind="series", farms=[0], want=("returns", "best"))
by_ensemble, by_realisation = int(ens["best"][0]), int(real["best"][0])
print(f"{len(params)} controllers, H = {H}, gamma = {GAMMA}, tuned on farm 0 from its reset state")
print(f"  by expected return over {M} futures: {params[by_ensemble]}  (expected {ens['expected_returns'][0, by_ensemble]:.4f}, "
      f"its return on the realisation {real['returns'][0, by_ensemble]:.4f})")
print(f"  on the one realisation:              {params[by_realisation]}  (return {real['returns'][0, by_realisation]:.4f}, "
      f"its expected return {ens['expected_returns'][0, by_realisation]:.4f})")
untuned = next(i for i, p in enumerate(params) if (p["alpha"], p["deadband"], p["lead"]) == (1.0, 0.0, 0))
ret = {"untuned (what lut_action does)": replay(w, FRESH_SEED, params[untuned]),
       f"tuned over {M} futures": replay(w, FRESH_SEED, params[by_ensemble]),
       "tuned on one realisation": replay(w, FRESH_SEED, params[by_realisation])}

# (b) the receding-horizon selector over the controllers without preview, on the same fresh realisations
grid0, params0 = WfStep.controller_grid([1.0, 0.5, 0.25, 0.1], [0.0, 2.5, 5.0, 7.5], [0])
lead0 = [i for i, p in enumerate(params) if p["lead"] == 0]
fixed0 = lead0[int(np.argmax(ens["expected_returns"][0, lead0]))]
ret[f"tuned over {M} futures, lead 0 only"] = replay(w, FRESH_SEED, params[fixed0])
ret["selector: every step, every farm its best of lead 0"], picks = select(w, FRESH_SEED, grid0)
base = ret[f"tuned over {M} futures"]
print(f"{B} fresh realisations (seed {FRESH_SEED}), {STEPS} steps, undiscounted episode return")
for label, r in ret.items():
    gain = r - base
    print(f"{label:>52}: mean {r.mean():.4f}, std over the farms {r.std(ddof=1):.4f}; against the ensemble-tuned controller "
          f"{gain.mean():+.4f} (standard error {gain.std(ddof=1) / np.sqrt(B):.4f}), ahead on {(gain > 0).sum()} of {B} farms")
gain = ret["selector: every step, every farm its best of lead 0"] - ret[f"tuned over {M} futures, lead 0 only"]
print(f"the selector against the fixed controller without preview {params[fixed0]}: {gain.mean():+.4f} (standard error "
      f"{gain.std(ddof=1) / np.sqrt(B):.4f}), ahead on {(gain > 0).sum()} of {B} farms")
top = np.argsort(-picks)[:3]
print("the selector's three most frequent picks:", [(params0[i], int(picks[i])) for i in top])
print("illustrative, not a result: one seed, one layout, one process.  last call:", w.controller_scenarios_timing(),
      w.controller_scenarios_kernel_info())
w.close()
