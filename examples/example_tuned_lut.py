"""Tuning the industry-baseline yaw controller under the env's own actuator: a row of three turbines under a noisy wind-direction
series (a slow swing of +-14 deg around 262 deg plus AR(1) noise of 2 deg, 8 m/s).  The yaw look-up table comes from the
project's coordinate search on a 2.5 deg grid (backend.WfStep.build_yaw_table, NEAREST).  `lut_action` chases every direction
change; the env moves a yaw at most 5 deg per step and its actuation budget then silences the turbine for a while, so how
much of the table's gain survives depends on the controller's filter gain alpha, its deadband and on whether it previews the
coming wind.  VecWindFarmEnv.controller_returns (include/wfrollout.h) scores a whole grid of such controllers over the
episode in ONE call from the env's current state, which it never changes: every (controller, step) is a row of one batched
step on the device.  The untuned controller (alpha 1, deadband 0, lead 0 — what stepping with lut_action does) is compared
with the best of a 4 x 4 x 2 grid and with holding zero yaw; then the best controller's `actions` are replayed through
env.step and both returns are printed.  What is printed is what this run measures on one synthetic series: illustrative, not
a result.  The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_tuned_lut.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

T = 120
rng = np.random.default_rng(3)
noise = np.zeros(T)
for i in range(1, T):
    noise[i] = 0.8 * noise[i - 1] + rng.normal(0.0, 2.0 * np.sqrt(1.0 - 0.8 ** 2))
series = np.stack([np.full(T, 8.0), 262.0 + 14.0 * np.sin(2.0 * np.pi * np.arange(T) / 60.0) + noise], axis=1)

with tempfile.TemporaryDirectory() as tmp:
    csv = os.path.join(tmp, "wind.csv")
    with open(csv, "w") as f:
        f.write("ws,wd\n" + "\n".join(f"{a!r},{b!r}" for a, b in series.tolist()) + "\n")
    env = envs.make("Turb3_Row1_Floris", env_batch=1, max_num_steps=T, wind_time_series=csv, return_torch=False)
    env.reset(seed=0)
    state = env.get_state()
    state["series_start"] = np.zeros(1, np.int32)  # the episode starts at the series' first row
    env.set_state(state)

    wd_axis, ws_axis = np.arange(240.0, 300.1, 2.5), np.array([8.0])
    table = env.fi.build_yaw_table(wd_axis, ws_axis)  # the optimiser ignores the actuator: the steady optimum per direction
    env.fi.set_yaw_table(table["table"], wd_axis, ws_axis, interp="nearest")

    H = T - 1 - env.fi.series_state()["t"]  # the steps the series has left
    grid, params = WfStep.controller_grid([1.0, 0.5, 0.25, 0.1], [0.0, 2.5, 5.0, 7.5], [0, 1])
    hold = len(params)  # one more controller that never moves: a deadband no error reaches
    ctl = {k: np.append(v, {"slot": 0, "alpha": 1.0, "deadband": 1e9, "lead": 0}[k]).astype(v.dtype) for k, v in grid.items()}
    r = env.controller_returns(ctl, H, wind="series", want=("returns", "actions", "gated", "best"))  # BEFORE step: nothing changes
    ret, gated = r["returns"][0], r["gated"][0]
    untuned = next(i for i, p in enumerate(params) if (p["alpha"], p["deadband"], p["lead"]) == (1.0, 0.0, 0))
    best = int(np.argmax(ret[:hold]))

    def gain(i):
        return 100.0 * (ret[i] - ret[hold]) / abs(ret[hold])

    print(f"row of three under a direction series of {T} rows, {H} steps, {hold} controllers + hold in one call")
    print(f"hold zero yaw:                  return {ret[hold]:.4f}")
    print(f"untuned (what lut_action does): return {ret[untuned]:.4f}  gain over hold {gain(untuned):+.2f} %  closed gates {int(gated[untuned])}")
    print(f"best of the grid {params[best]}: return {ret[best]:.4f}  gain over hold {gain(best):+.2f} %  closed gates {int(gated[best])}")
    for a in (1.0, 0.5, 0.25, 0.1):
        row = [f"{gain(i):+.2f}" for i, p in enumerate(params) if p["alpha"] == a]
        print(f"  alpha {a:<4}: gain % over (deadband 0 / 2.5 / 5 / 7.5) x (lead 0, 1): {row}")
    paid = 0.0
    for h in range(H):  # the best controller's actions through the env itself
        paid += float(env.step({"yaw": r["actions"][:, best, h].copy()})[1][0])
    print(f"replayed through env.step: return {paid:.4f} (the rollout said {ret[best]:.4f})")
    print("last rollout:", env.fi.rollout_timing(), env.fi.rollout_kernel_info())
    env.close()
