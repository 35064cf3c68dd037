"""Domain randomisation of the wake model on a row of three turbines at 270 deg: 64 farms, each under its own wake-model
parameter set — ambient turbulence intensity in (0.04, 0.12), the wake-growth coefficient ka within +-30 % of the model's —
all under ONE wind, all holding the static optimal yaw found under the NOMINAL model (include/wfmodelset.h;
backend.WfStep.set_model_sets; VecWindFarmEnv(model_randomization=...) draws such sets per reset).  Printed: the spread of
the power gain over zero yaw across the sets — how much of the nominal optimum's promise survives another wake model.
COST: while sets are held every farm is solved by the float64 kernels on every step.
The numbers are illustrative, not a result.
Run from the repo root on an MI355X:  python examples/example_model_randomization.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D, B = 126.0, 64
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
w = WfStep(x, y, env_batch=B)
w.set_wind(8.0, 270.0)
nominal = w.optimize_yaw(None)  # under the handle's one model (the search refuses a handle that holds sets)
yaw_opt = np.asarray(nominal["yaw"], np.float32)[0]
print(f"nominal model: optimal yaw {np.round(yaw_opt, 2)} deg, gain over zero yaw "
      f"{100 * (float(nominal['power'][0]) / float(nominal['power_initial'][0]) - 1):.2f} %")

base = w.model_set_from_model()
rng = np.random.default_rng(0)
sets = {"ambient_ti": rng.uniform(0.04, 0.12, B), "ka": base["ka"] * rng.uniform(0.7, 1.3, B)}
w.set_model_sets(sets)  # no set_of: farm b takes set b
p_zero = w.step(np.zeros((B, 3), np.float32))["power"].astype(np.float64).sum(axis=1)
p_opt = w.step(np.tile(yaw_opt, (B, 1)))["power"].astype(np.float64).sum(axis=1)
gain = 100.0 * (p_opt / p_zero - 1.0)
print(f"{B} parameter sets (risk_resolve() = {w.risk_resolve()}: every farm in float64), gain of the NOMINAL optimum over zero yaw [%]:")
print(f"  min {gain.min():.2f}   5 % {np.percentile(gain, 5):.2f}   median {np.median(gain):.2f}   95 % {np.percentile(gain, 95):.2f}   max {gain.max():.2f}")
for k in np.argsort(gain)[[0, B // 2, -1]]:
    print(f"  ambient_ti {sets['ambient_ti'][k]:.3f}  ka {sets['ka'][k]:.3f}:  {p_zero[k] / 1e6:.3f} MW -> {p_opt[k] / 1e6:.3f} MW  ({gain[k]:+.2f} %)")
print("illustrative, not a result")
w.close()
