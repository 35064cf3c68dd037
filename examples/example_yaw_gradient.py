"""Yaw sensitivities on a row of turbines: how the power of every turbine changes when turbine i turns
(backend.WfStep.yaw_gradient, include/wfgrad.h), and gradient ascent on the farm power through torch autograd
(autograd.differentiable_power) next to the coordinate search (WfStep.optimize_yaw).  The derivative is the project's own
DIFFERENCE QUOTIENT at a finite step — 2 N + 1 farm solves per farm in one batched step on the device, what FLORIS' scipy
optimiser gets from 2 N sequential solves; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_yaw_gradient.py [gradient steps, default 30]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.autograd import differentiable_power  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
ws, wd = np.array([8.0, 8.0, 8.0]), np.array([270.0, 264.0, 90.0])
w = WfStep(x, y, env_batch=len(wd))
w.set_wind(ws, wd)

# 1. the Jacobian's structure: J[i, j] = d P_j / d yaw_i [kW/deg].  A turbine's yaw does not reach upwind: under 270 deg the
#    matrix is upper triangular, under 90 deg lower triangular; turning costs the turbine itself and pays behind it.
yaw = np.tile(np.float32([10.0, 5.0, 0.0]), (len(wd), 1))
r = w.yaw_gradient(yaw, jacobian=True)
for b in range(len(wd)):
    print(f"wind {ws[b]:.0f} m/s from {wd[b]:.0f} deg, yaw {yaw[b]}: power {np.round(r['power'][b] / 1e3, 1)} kW, "
          f"d(farm power)/d(yaw) {np.round(r['gradient'][b] / 1e3, 2)} kW/deg")
    for i in range(3):
        print("      d P_j / d yaw_%d [kW/deg]: " % i + "  ".join(f"{v / 1e3:8.2f}" for v in r["jacobian"][b, i]))
credit = w.yaw_gradient(yaw, np.tile(np.float32([0.0, 0.0, 1.0]), (len(wd), 1)))["gradient"]
print("credit for the LAST turbine's power (cotangent e_2) [kW/deg]:", np.round(credit[0] / 1e3, 2), "under 270 deg")

# 2. projected gradient ascent from zero yaw through torch autograd, bounds (-25, 25)
lo, hi = -25.0, 25.0
ty = torch.zeros((len(wd), 3), dtype=torch.float32, device="cuda", requires_grad=True)
opt = torch.optim.Adam([ty], lr=2.0)
p0 = differentiable_power(w, ty, bounds=(lo, hi)).detach().sum(dim=1)
for k in range(steps):
    opt.zero_grad()
    (-differentiable_power(w, ty, bounds=(lo, hi)).sum() / 1e6).backward()  # MW: the loss of a learning loop
    opt.step()
    with torch.no_grad():
        ty.clamp_(lo, hi)  # the projection; at a bound the quotient is one-sided by itself
pg = differentiable_power(w, ty, bounds=(lo, hi)).detach().sum(dim=1)
search = w.optimize_yaw(bounds=(lo, hi))
print(f"\n{steps} steps of Adam on -farm power [MW] from zero yaw        |  optimize_yaw (coordinate search, passes (5, 4))")
for b in range(len(wd)):
    print(f"  {wd[b]:5.0f} deg: yaw {np.round(ty[b].detach().cpu().numpy(), 1)}  {pg[b].item() / 1e6:.4f} MW ({100 * (pg[b].item() / p0[b].item() - 1):+.2f} %)"
          f"  |  yaw {search['yaw'][b]}  {search['power'][b] / 1e6:.4f} MW ({100 * (search['power'][b] / search['power_initial'][b] - 1):+.2f} %)")
print("last gradient run:", w.grad_timing(), w.grad_kernel_info())
w.close()
