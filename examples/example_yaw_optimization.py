"""The static wake-steering baseline for HornsRev1: the best yaw for a handful of wind directions, all optimised at once —
one farm of the batch per direction (backend.WfStep.optimize_yaw; VecWindFarmEnv.optimal_yaw does the same for the winds
an env currently holds).  The project's own coordinate search, in the spirit of "serial refine"; not pinned to FLORIS'
optimiser (include/wfyawopt.h).
Run from the repo root on an MI355X:  python examples/example_yaw_optimization.py [wind speed, default 8]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

lay = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))["HornsRev1_"]
ws = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
wd = np.array([255.0, 262.0, 270.0, 278.0, 285.0, 180.0, 173.0, 221.0])  # along the rows, a few degrees off them, the columns, a diagonal
w = WfStep(lay["xcoords"], lay["ycoords"], env_batch=len(wd))
w.set_wind(np.full(len(wd), ws), wd)
r = w.optimize_yaw(bounds=(-25.0, 25.0), passes=(5, 4))
print(f"HornsRev1, {ws:g} m/s, passes (5, 4), bounds +-25 deg")
print(" wind dir   baseline MW   optimised MW    gain   turbines yawed   largest |yaw|")
for k in range(len(wd)):
    y = r["yaw"][k]
    print(f"  {wd[k]:6.1f}   {r['power_initial'][k] / 1e6:11.3f}   {r['power'][k] / 1e6:12.3f}   {100 * (r['power'][k] / r['power_initial'][k] - 1):5.2f} %"
          f"   {int((y != 0).sum()):14d}   {np.abs(y).max():13.2f}")
print("last run:", w.yawopt_timing())
w.close()
