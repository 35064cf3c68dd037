"""Per-agent credit on a row of three turbines: the DIFFERENCE REWARD of every turbine-agent for one joint action —
D_i = r(a) - r(a_-i, c_i), what the farm's reward owes to agent i's own action against "it held its yaw" — and the
advantage of a COMA critic's counterfactual baseline from the rewards of all three discrete actions
(VecWindFarmEnv.counterfactual_rewards, include/wfcredit.h): 1 + N K farm solves per farm in one batched step on the
device.  The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_difference_rewards.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402

B = 2
# actions 0 / 1 / 2 = down / hold / up by 1 deg: a step the actuation budget (1.8 deg per 60 s step) lets an agent take every
# time; with the default 5 deg the env's own gate would turn most actions — base and alternatives alike — into "down"
env = envs.make("Turb3_Row1_Floris", controls={"yaw": (-40, 40, 1)}, env_batch=B, continuous_control=False, max_num_steps=40)
env.reset(seed=0, options={"wind_speed": 8.0, "wind_direction": 270.0})  # along the row: turbine 0 is upstream
N = env.num_turbines
up = torch.full((B, N), 2.0).cuda()
for _ in range(10):  # steer everybody 10 deg, so that "down" and "up" are not mirror images
    env.step({"yaw": up})

# 1. difference rewards for one joint action, BEFORE the env takes it: the first turbine steers on, the others hold
actions = torch.tensor([[2.0, 1.0, 1.0]] * B).cuda()
cf = env.counterfactual_rewards(actions, "hold", strict=True)
print("joint action", actions[0].tolist(), "-> farm reward", round(cf["reward_base"][0].item(), 5))
for i in range(N):
    print(f"  turbine_{i + 1}: reward had it held {cf['reward_alt'][0, i, 0].item():.5f}, difference reward {cf['difference'][0, i, 0].item():+.5f}")
print("  (an agent that holds is owed exactly 0; turbine_1's steering pays through the turbines behind it)")

# 2. COMA: the advantage of the action taken against the policy's own expectation over agent i's three actions, the others'
#    actions fixed.  One call gives r(a_-i, a'_i) for every agent and every a'_i; the baseline is one line of torch.
allr = env.counterfactual_rewards(actions, "all", strict=True)  # reward_alt (B, N, 3)
pi = torch.softmax(torch.zeros((B, N, 3), dtype=torch.float64, device="cuda"), dim=2)  # a uniform policy pi(k | agent i)
advantage = allr["reward_base"][:, None] - (pi * allr["reward_alt"]).sum(dim=2)
print("\nrewards of turbine_1's three actions (down, hold, up):", [round(v, 5) for v in allr["reward_alt"][0, 0].tolist()])
print("COMA advantage r_base - sum_k pi(k) r_alt[i][k] per agent:", [round(v, 5) for v in advantage[0].tolist()])

# 3. the env has not moved: the step pays what row 0 said it would
reward = env.step({"yaw": actions})[1]
print(f"\nstep(actions) pays {reward[0].item():.5f}; reward_base was {cf['reward_base'][0].item():.5f}")
print("last credit run:", env.fi.credit_timing(), env.fi.credit_kernel_info())
env.close()
