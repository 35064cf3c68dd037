"""Wake steering under wind-direction uncertainty on a row of turbines: the NOMINAL yaw table (every node optimised for a
sharp direction) next to the ROBUST one (every node optimised for the expected power over a Gaussian set of direction
errors), each scored with and without uncertainty (backend.WfStep.build_yaw_table / optimize_yaw with wd_uncertainty=...,
WfStep.uncertain_power; VecWindFarmEnv.optimal_yaw takes the same keyword).  The nominal table over-steers: scored under
uncertainty it gives part of its promised gain back.  The project's own definition (include/wfrobust.h), what FLORIS users
reach through UncertaintyInterface; PARITY UNPINNED beyond the oracle.
Run from the repo root on an MI355X:  python examples/example_robust_yaw.py [std of the direction error in deg, default 3]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep, wd_uncertainty_members  # noqa: E402

D = 126.0
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
std = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
unc = dict(std=std, resolution=std, cutoff=0.95, frame="fixed")  # five members at -2 std .. 2 std; the nacelle stays put
delta, weight, _ = wd_uncertainty_members(unc)
print(f"members {delta} deg, weights {np.round(weight / weight.sum(), 4)}")

wd_axis, ws = np.arange(258.0, 283.0, 2.0), 8.0
w = WfStep(x, y, env_batch=len(wd_axis))
nominal = w.build_yaw_table(wd_axis, [ws])
robust = w.build_yaw_table(wd_axis, [ws], wd_uncertainty=unc)
w.set_wind(np.full(len(wd_axis), ws), wd_axis)  # one farm per table node: score every node's yaw at its own direction
zero = np.zeros((len(wd_axis), 3), np.float32)
sharp = {k: w.step(t)["power"].astype(np.float64).sum(axis=1) for k, t in
         (("zero", zero), ("nominal", nominal["table"][:, 0]), ("robust", robust["table"][:, 0]))}
blurred = {k: w.uncertain_power(t, wd_uncertainty=unc)["expected_power"] for k, t in
           (("zero", zero), ("nominal", nominal["table"][:, 0]), ("robust", robust["table"][:, 0]))}
print("                  nominal table            robust table        gain over zero yaw [%]: sharp direction | under uncertainty")
print(" wind dir     yaw 0     1     2       yaw 0     1     2           nominal   robust   |   nominal   robust")
for k, d in enumerate(wd_axis):
    a, b = nominal["table"][k, 0], robust["table"][k, 0]
    g = [100.0 * (s[n][k] / s["zero"][k] - 1.0) for s in (sharp, blurred) for n in ("nominal", "robust")]
    print(f"  {d:6.1f}   {a[0]:7.2f} {a[1]:5.1f} {a[2]:5.1f}   {b[0]:7.2f} {b[1]:5.1f} {b[2]:5.1f}         {g[0]:7.3f}  {g[1]:7.3f}   |   {g[2]:7.3f}  {g[3]:7.3f}")
tot = {k: (sharp[k].sum(), blurred[k].sum()) for k in sharp}
for n in ("nominal", "robust"):
    print(f"{n:8s} table, all directions: gain {100 * (tot[n][0] / tot['zero'][0] - 1):.3f} % for a sharp direction, "
          f"{100 * (tot[n][1] / tot['zero'][1] - 1):.3f} % under uncertainty")
print("last robust evaluation:", w.robust_timing())
w.close()
