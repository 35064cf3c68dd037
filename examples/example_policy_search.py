"""Searching the parameters of a small network policy on the device: a row of three turbines under a held wind along the row
(8 m/s, 270 deg), a parameter-SHARED policy 3 -> 8 -> 1 — every turbine feeds its own (yaw, local wind speed, local wind
direction) through the same 41 weights and gets its yaw increment — and a few iterations of the cross-entropy method over
those weights.  Every iteration scores K = 32 parameter vectors over H steps in ONE call of VecWindFarmEnv.policy_returns
(include/wfpolicy.h) from the env's current state, which it never changes: one batched step per env step, 32 rows per farm,
the network evaluated between two steps on the device.  Beside it: holding zero yaw, and the untuned yaw-table controller
scored by controller_returns (include/wfrollout.h).  The policy sees only local measurements, so what it can learn here is
"the turbine with the fastest wind steers, the others hold".  What is printed is what this run measures on one wind and one
seed: illustrative, not a result.  The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_policy_search.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402
from wfcrl_env_amd import policy as P  # noqa: E402

H, K, ELITES, ITERATIONS = 24, 32, 6, 6
env = envs.make("Turb3_Row1_Floris", env_batch=1, max_num_steps=H + 4, return_torch=False)
env.reset(seed=0, options={"wind_speed": 8.0, "wind_direction": 270.0})

widths = (3, 8, 1)
spec = P.mlp_spec("shared", widths, "tanh", "tanh", out_scale=5.0, shift=[0.0, 7.0, 270.0], scale=[1 / 20.0, 1.0, 1 / 5.0])
n_par = P.param_count(widths)
rng = np.random.default_rng(0)
mean, sigma = np.zeros(n_par), np.full(n_par, 1.0)
hold = np.zeros((1, n_par), np.float32)  # weights and biases 0: the action is 0, the turbines hold
r_hold = env.policy_returns((hold, spec), H, want=("returns",))["returns"][0, 0]
print(f"row of three, {H} steps, shared policy {widths} ({n_par} parameters), CEM with K = {K}, {ELITES} elites")
print(f"hold zero yaw:                       return {r_hold:.4f}")
for it in range(ITERATIONS):
    cand = mean + sigma * rng.standard_normal((K, n_par))
    cand[0] = mean  # the incumbent stays a candidate: the best return never falls
    r = env.policy_returns((cand.astype(np.float32), spec), H, want=("returns", "best", "gated", "final_yaw"))  # BEFORE step: nothing changes
    ret = r["returns"][0]
    order = np.argsort(-ret)[:ELITES]
    mean, sigma = cand[order].mean(axis=0), cand[order].std(axis=0) + 0.05
    b = int(r["best"][0])
    print(f"iteration {it}: best of {K} {ret[b]:.4f} ({100.0 * (ret[b] - r_hold) / abs(r_hold):+.2f} % over hold), mean of the elites "
          f"{ret[order].mean():.4f}, final yaw {[round(float(v), 1) for v in r['final_yaw'][0, b]]}, closed gates {int(r['gated'][0, b])}")

wd_axis, ws_axis = np.arange(260.0, 280.1, 2.5), np.array([8.0])
table = env.fi.build_yaw_table(wd_axis, ws_axis)
env.fi.set_yaw_table(table["table"], wd_axis, ws_axis, interp="nearest")
r_lut = env.controller_returns({"slot": 0}, H, want=("returns",))["returns"][0, 0]
print(f"untuned yaw-table controller:        return {r_lut:.4f} ({100.0 * (r_lut - r_hold) / abs(r_hold):+.2f} % over hold)")
best = mean.astype(np.float32)[None]
r = env.policy_returns((best, spec), H, want=("returns", "actions"))
paid = 0.0
for h in range(H):  # the found policy's actions through the env itself
    paid += float(env.step({"yaw": r["actions"][:, 0, h].copy()})[1][0])
print(f"the elites' mean replayed through env.step: return {paid:.4f} (the rollout said {r['returns'][0, 0]:.4f})")
print("last rollout:", env.fi.policy_timing(), env.fi.policy_kernel_info())
env.close()
