"""Calibration of the wake model to measured turbine powers, as a TWIN EXPERIMENT on a row of three turbines
(include/wfcalib.h; backend.WfStep.calibrate_model).  The "measurements" are what a farm under a hidden TRUE parameter set
produces — WfStep(model_sets=truth) — under a handful of winds and yaws; the fit starts from the default model and searches
ambient_ti, ka, kb, alpha and beta on the device: 64 candidate sets per iteration, each solved under all the conditions in one
step, their constants written by the glue kernel, nothing read back in between.  Printed: the loss at the start and at the
end, and the recovered fields beside the truth (the five are not all identifiable from twelve conditions: several sets
explain the powers equally well — the loss says how well, not the fields).  The fitted set then goes where
domain randomisation starts: VecWindFarmEnv(model_randomization=dict(sets=..., set_of=...)).
The numbers are illustrative, not a result.
Run from the repo root on an MI355X:  python examples/example_model_calibration.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

D, C = 126.0, 12
x, y = np.arange(3) * 5 * D, np.zeros(3)  # three turbines in a row, 5 D apart, the row along 270 deg
rng = np.random.default_rng(0)
ws, wd = rng.uniform(7.0, 10.5, C), 270.0 + rng.uniform(-10.0, 10.0, C)
yaw = rng.uniform(-20.0, 20.0, (C, 3)).astype(np.float32)

# the "site": one farm per condition under the hidden truth
truth = {"ambient_ti": 0.085, "ka": 0.31, "kb": 0.0055, "alpha": 0.68, "beta": 0.07}
site = WfStep(x, y, env_batch=C, model_sets=[truth], model_set_of=np.zeros(C, np.int32))
site.set_wind(ws, wd)
measured = np.asarray(site.step(yaw)["power"], np.float64)
site.close()

w = WfStep(x, y)  # the default model: where the fit starts
bounds = {"ambient_ti": (0.03, 0.15), "ka": (0.15, 0.6), "kb": (0.001, 0.01), "alpha": (0.3, 0.9), "beta": (0.04, 0.12)}
fit = w.calibrate_model(ws, wd, yaw, measured, bounds, candidates=64, elites=8, sigma=(0.25, 0.12, 0.06, 0.03, 0.015, 0.008), seed=1)
start = w.model_set_from_model()
print(f"{C} conditions x 3 turbines, scale = rated power {w.rated_power() / 1e6:.2f} MW")
print(f"loss at the default model {float(fit['init_loss']):.3e}  ->  after the fit {float(fit['best_loss']):.3e}   "
      f"(per iteration: {', '.join(f'{v:.2e}' for v in fit['history'])}; {int(fit['n_invalid'])} candidates left the model's domain)")
rms = np.sqrt(np.mean((np.asarray(fit["fit_power"], np.float64) - measured) ** 2))
print(f"rms power residual of the fitted set {rms / 1e3:.2f} kW")
print("field         start     fitted    truth")
for f in bounds:
    print(f"  {f:<11} {start[f]:<9.4f} {float(fit['best_set'][f]):<9.4f} {truth[f]:<9.4f}")
w.close()

# the fitted set as the centre of a domain randomisation: here simply every env under it
B = 4
best = {f: np.array([float(v)]) for f, v in fit["best_set"].items()}
env = envs.make("Turb3_Row1_Floris", env_batch=B, max_num_steps=10, model_randomization=dict(sets=best, set_of=np.zeros(B, np.int32)))
env.reset(seed=0)
print(f"VecWindFarmEnv x {B} under the fitted set: ambient_ti {env.model_sets['ambient_ti'][0]:.4f}, ka {env.model_sets['ka'][0]:.4f}")
env.close()
print("illustrative, not a result")
