"""Wake steering over a wind rose for HornsRev1: build a yaw look-up table with the on-device optimiser, quote AEP with and
without it and the gain per direction, then run the table as a controller in the batched env under a wind time series.
The project's own interpolation and reduction (include/wfrose.h) — not FLORIS' AEP routine; PARITY UNPINNED beyond the
oracle.
Run from the repo root on an MI355X:  python examples/example_wind_rose.py"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd import environments as envs  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

lay = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))["HornsRev1_"]
w = WfStep(lay["xcoords"], lay["ycoords"], env_batch=1)

# a westerly sector of the rose: directions every 3 deg, speeds 5 .. 13 m/s, a made-up frequency table
wd = np.arange(240.0, 301.0, 3.0)
ws = np.arange(5.0, 14.0, 1.0)
freq = np.exp(-0.5 * ((wd[:, None] - 270.0) / 20.0) ** 2) * np.exp(-0.5 * ((ws[None, :] - 8.0) / 2.5) ** 2)
freq /= freq.sum()

# the table: the optimiser's yaw on a coarser grid (every 3 deg, three speeds), read by nearest node — a linear blend
# passes through zero where the optimum flips sign across a row's axis (include/wfrose.h)
tab_wd, tab_ws = wd, np.array([6.0, 9.0, 12.0])
built = w.build_yaw_table(tab_wd, tab_ws, bounds=(-25.0, 25.0), passes=(5, 4))
w.set_yaw_table(built["table"], tab_wd, tab_ws, interp="nearest", slot=0)
w.set_yaw_table(built["table"], tab_wd, tab_ws, interp="linear", slot=1)

r = w.expected_power(wd, ws, freq, cases=("zero", ("table", 0), ("table", 1)))
print(f"HornsRev1, {wd.size} directions x {ws.size} speeds; table {tab_wd.size} x {tab_ws.size} nodes")
for label, k in (("zero yaw", 0), ("table, nearest", 1), ("table, linear", 2)):
    print(f"  {label:15s} expected power {r['expected_power'][k] / 1e6:8.3f} MW   AEP {r['aep_gwh'][k]:8.2f} GWh"
          f"   gain {100 * (r['expected_power'][k] / r['expected_power'][0] - 1):5.2f} %")
per_dir = (r["condition_power"].astype(np.float64) * freq[None]).sum(axis=2)  # (cases, directions)
print("  wind dir   gain nearest   gain linear")
for d in range(wd.size):
    print(f"   {wd[d]:6.1f}   {100 * (per_dir[1, d] / per_dir[0, d] - 1):10.2f} %   {100 * (per_dir[2, d] / per_dir[0, d] - 1):9.2f} %")
print("last evaluation:", w.rose_timing())
w.close()

# the table as a controller: 16 farms play a wind series, the look-up-table policy tracks the table under the yaw-rate limit
rng = np.random.default_rng(0)
T = 12
series = np.stack([8.0 + rng.normal(0.0, 0.5, T), 268.0 + np.cumsum(rng.normal(0.0, 1.5, T))], axis=1)
with tempfile.TemporaryDirectory() as tmp:
    csv = os.path.join(tmp, "wind.csv")
    with open(csv, "w") as f:
        f.write("ws,wd\n" + "\n".join(f"{a!r},{b!r}" for a, b in series.tolist()))
    env = envs.make("HornsRev1_Floris", env_batch=16, max_num_steps=T, wind_time_series=csv, actuation_budget=1.0)
    env.fi.set_yaw_table(built["table"], tab_wd, tab_ws, interp="nearest")
    twin = envs.make("HornsRev1_Floris", env_batch=16, max_num_steps=T, wind_time_series=csv, actuation_budget=1.0)
    env.reset(seed=1), twin.reset(seed=1)
    print("  step   farm power with the LUT controller [MW]   at zero yaw [MW]   largest |yaw - target| [deg]")
    for k in range(6):
        _, _, _, _, info = env.step(env.lut_action())
        _, _, _, _, base = twin.step({"yaw": np.zeros((16, env.num_turbines), np.float32)})
        off = (env.fi.env_get_state(as_torch=True)["yaw"] - env.lut_target_yaw()).abs().max().item()
        print(f"  {k:4d}   {info['power'].sum(dim=1).mean().item():41.3f}   {base['power'].sum(dim=1).mean().item():16.3f}   {off:28.2f}")
    env.close(), twin.close()
