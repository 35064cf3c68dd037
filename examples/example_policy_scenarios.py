"""Picking among a handful of network policies under an UNCERTAIN wind: the policy-search example's row of three turbines and
its parameter-shared policy 3 -> 8 -> 1, now on a wind_process episode — the wind wanders around 270 deg along the row —, and
K = 6 parameter vectors (vector 0 holds: all weights 0) scored in ONE call of VecWindFarmEnv.policy_scenarios
(include/wfpolscen.h) over M = 16 wind futures drawn from the env's own process: per policy the mean return over the futures,
the mean of its worst quarter (CVaR), and the choice by either — risk_weight 0 picks by the mean, 0.5 puts half the weight on
the tail.  A network is a feedback law: it moves the yaw differently under every future, so its K M closed loops are K M rows
of one batched step per env step, and nothing is read back in between; the env state is never changed.  The winner's actions
under future 0 are then replayed through the env's own fused step (env.fi.env_step) under that future's wind, step after
step, and the return is compared with the rollout's.  What is printed is what this run measures on one seed: illustrative, not
a result.  The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_policy_scenarios.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402
from wfcrl_env_amd import policy as P  # noqa: E402

H, K, M, TAIL = 12, 6, 16, 4
process = dict(ws_revert=0.1, ws_sigma=0.3, wd_revert=0.1, wd_sigma=1.5, wd_ramp=0.5, dist=dict(wd_mean=270.0, wd_std=3.0))
env = envs.make("Turb3_Row1_Floris", env_batch=1, max_num_steps=H + 4, return_torch=False, wind_process=process)
env.reset(seed=0)

widths = (3, 8, 1)
spec = P.mlp_spec("shared", widths, "tanh", "tanh", out_scale=5.0, shift=[0.0, 7.0, 270.0], scale=[1 / 20.0, 1.0, 1 / 5.0])
rng = np.random.default_rng(0)
params = rng.standard_normal((K, P.param_count(widths))).astype(np.float32)
params[0] = 0.0  # weights and biases 0: the action is 0, the turbines hold

want = ("expected_returns", "cvar", "score", "best", "member_returns", "actions", "wind_paths", "first_action")
by_mean = env.policy_scenarios((params, spec), H, members=M, seed=1, tail=TAIL, risk_weight=0.0, want=want)  # BEFORE step: nothing changes
by_tail = env.policy_scenarios((params, spec), H, members=M, seed=1, tail=TAIL, risk_weight=0.5, want=("score", "best"))
print(f"row of three, {H} steps, shared policy {widths}, K = {K} parameter vectors over M = {M} futures (illustrative, not a result)")
for k in range(K):
    print(f"  policy {k}{' (hold)' if k == 0 else '       '}: expected return {by_mean['expected_returns'][0, k]:.4f}, worst quarter "
          f"{by_mean['cvar'][0, k]:.4f}, score at half weight on the tail {by_tail['score'][0, k]:.4f}")
b0, b1 = int(by_mean["best"][0]), int(by_tail["best"][0])
print(f"picked by expected return: policy {b0}; with half the weight on the tail: policy {b1}")

# the winner under future 0, replayed: every tick the member's wind is set, the speed of the step before is left as the one the
# reward is normalised by (step 0: the current speed), and the fused step takes the rollout's raw action
fi = env.fi
speed_before = float(np.asarray(fi.get_wind()[0]).reshape(-1)[0])
paid = 0.0  # (gamma is 1: the return is the plain sum)
for h in range(H):
    ws, wd = by_mean["wind_paths"][0, 0, h]
    fi.set_wind(ws, wd)
    fi.env_set_prev_wind(speed_before)
    paid += float(fi.env_step(by_mean["actions"][:, b0, 0, h].copy(), want=("reward",))["reward"][0])
    speed_before = ws
said = float(by_mean["member_returns"][0, b0, 0])
print(f"policy {b0} under future 0 replayed through the env's fused step: return {paid:.4f}; the rollout said {said:.4f} "
      f"({'they match' if abs(paid - said) <= 1e-4 * max(1.0, abs(said)) else 'THEY DIFFER'}: the step's reward is float32)")
print("last call:", fi.policy_scenarios_timing(), fi.policy_scenarios_kernel_info())
env.close()
