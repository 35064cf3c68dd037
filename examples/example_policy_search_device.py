"""examples/example_policy_search.py with the Python loop replaced by ONE call: a row of three turbines under a held wind
along the row (8 m/s, 270 deg), a parameter-SHARED policy 3 -> 8 -> 1, and a cross-entropy search over its 41 weights by
VecWindFarmEnv.search_policy (include/wfpolsearch.h).  The candidates are drawn on the device (a Philox block per weight), every
iteration's K = 32 vectors are scored by the policy extension's closed-loop rollouts, the fitness is aggregated and mean and
width per weight are refitted on the device; nothing is read back between two iterations, and the env state is never changed.
The draws are the device's counter-based ones, not NumPy's, so the numbers differ from the hand-written example's.  What is
printed is what this run measures on one wind and one seed: illustrative, not a result.  The project's own definition; PARITY
UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_policy_search_device.py"""
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
start = np.zeros(n_par, np.float32)  # weights and biases 0: the action is 0, the turbines hold
print(f"row of three, {H} steps, shared policy {widths} ({n_par} parameters), CEM on the device with K = {K}, {ELITES} elites")
r = env.search_policy((start, spec), H, sigma=1.0, candidates=K, elites=ELITES, iterations=ITERATIONS, sigma_min=0.05, seed=0,
                      want=("best_params", "best_fitness", "init_fitness", "fitness", "winner", "sigma"))  # BEFORE step: nothing changes
r_hold = float(r["init_fitness"])
print(f"hold zero yaw (the start vector):    return {r_hold:.4f}")
for it in range(ITERATIONS):
    f = r["fitness"][it]
    print(f"iteration {it}: best of {K} {f.max():.4f} ({100.0 * (f.max() - r_hold) / abs(r_hold):+.2f} % over hold), candidate "
          f"{int(r['winner'][it])}, mean of the elites {np.sort(f)[-ELITES:].mean():.4f}")
print(f"best vector:                         return {float(r['best_fitness']):.4f} "
      f"({100.0 * (float(r['best_fitness']) - r_hold) / abs(r_hold):+.2f} % over hold), widths now {r['sigma'].min():.3f} .. {r['sigma'].max():.3f}")
print("the search:", env.fi.search_policy_timing(), env.fi.search_policy_kernel_info())
best = r["best_params"][None]
ro = env.policy_returns((best, spec), H, want=("returns", "actions"))
paid = 0.0
for h in range(H):  # the best vector's actions through the env itself
    paid += float(env.step({"yaw": ro["actions"][:, 0, h].copy()})[1][0])
print(f"the best vector replayed through env.step: return {paid:.4f} (the rollout said {ro['returns'][0, 0]:.4f})")
env.close()
