"""First-order trajectory optimisation in the simulator, on a row of three turbines 5 D apart under (8 m/s, 270 deg): ONE
action sequence of H steps per farm is improved by gradient ascent (torch Adam) on its discounted return from the env's
CURRENT state, through autograd.differentiable_return (include/wfretgrad.h: the return and its derivative with respect to
every action of the sequence come out of one batched step of H (2 N + 1) rows per farm; the derivative is a difference
quotient at a finite step chained through the transition's 0/1 Jacobian — where the budget gate or a clip takes, it is 0).
It is compared with backend.WfStep.plan_actions, the zeroth-order sibling (the cross-entropy method over the same returns),
at an EQUAL COUNT of evaluated rows: 24 gradient iterations x 56 rows = 3 CEM iterations x 56 candidates x 8 steps = 1344 rows
per farm.  Both start from holding still; the four farms start from different yaws.  Which of the two finds the better
sequence depends on H, gamma, the learning rate, the CEM widths and the start: the output is illustrative, not a result.
The project's own definition; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_gradient_planner.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import autograd  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
B, H, GAMMA, ITERS, LR = 4, 8, 0.97, 24, 1.0
N = len(x)
CEM_ITERS, CEM_K = 3, 56
assert ITERS * H * (2 * N + 1) == CEM_ITERS * CEM_K * H  # the same number of evaluated rows per farm

w = WfStep(x, y, env_batch=B)
w.set_wind(8.0, 270.0)  # along the row: turbine 0 is upstream
w.env_config()  # +-40 deg, 5 deg per step, 0.3 deg/s, 60 s steps, budget 0.1, continuous control
w.env_reset()
state = w.env_get_state()
state["yaw"] = np.float32([[0.0, 0.0, 0.0], [10.0, 5.0, 0.0], [-10.0, -5.0, 0.0], [20.0, 0.0, 0.0]])
w.env_set_state(state)  # (read by both planners, changed by neither)

# gradient ascent on one sequence per farm, from holding still; the best sequence seen is kept
actions = torch.zeros((B, 1, H, N), dtype=torch.float32, device="cuda", requires_grad=True)
opt = torch.optim.Adam([actions], lr=LR)
best_ret = torch.full((B,), -float("inf"), dtype=torch.float64, device="cuda")
best_seq = torch.zeros((B, H, N), dtype=torch.float32, device="cuda")
first = None
for it in range(ITERS):
    opt.zero_grad()
    ret = autograd.differentiable_return(w, actions, gamma=GAMMA)  # (B, 1) float64: ONE run, the gradient is kept for backward
    (-ret.sum()).backward()
    with torch.no_grad():
        r = ret[:, 0].detach()
        first = r.clone() if first is None else first
        better = r > best_ret
        best_ret = torch.where(better, r, best_ret)
        best_seq[better] = actions[better, 0]
    opt.step()
    with torch.no_grad():
        actions.clamp_(-5.0, 5.0)  # beyond +-yaw_step the clip takes and the derivative is 0

cem = w.plan_actions(H, candidates=CEM_K, elites=8, gamma=GAMMA, want=("plan", "plan_return", "hold_return", "final_yaw"))
walk = w.return_gradient(best_seq[:, None].contiguous(), gamma=GAMMA, want=("returns", "final_yaw", "pass_mask"))

print(f"row of three, 5 D apart, 8 m/s along the row; H = {H}, gamma = {GAMMA}; {ITERS * H * (2 * N + 1)} evaluated rows per farm each")
print("  hold still          :", [round(float(v), 4) for v in np.asarray(cem["hold_return"])])
print("  gradient ascent     :", [round(v, 4) for v in best_ret.tolist()], f"(Adam, lr {LR}, {ITERS} iterations; first iterate",
      [round(v, 4) for v in first.tolist()], ")")
print("  cross-entropy method:", [round(float(v), 4) for v in np.asarray(cem["plan_return"])], f"({CEM_ITERS} iterations of {CEM_K} candidates)")
print("  final yaw, gradient :", [[round(v, 1) for v in row] for row in walk["final_yaw"][:, 0].tolist()])
print("  final yaw, CEM      :", [[round(float(v), 1) for v in row] for row in np.asarray(cem["final_yaw"])])
print("  share of the best sequence's actions that pass gate and clips:", round(float((walk["pass_mask"] & 1).double().mean().item()), 2))
print("illustrative, not a result.  last run:", w.return_gradient_timing(), w.return_gradient_kernel_info())
w.close()
