"""A hub-height wake map of one farm of a batch, and a virtual met mast for every farm (flow sampling at arbitrary
points: backend.WfStep.sample_flow / horizontal_plane, VecWindFarmEnv.sample_flow).
Run from the repo root on an MI355X:  python examples/example_flow_field.py [env_batch] [out_prefix]
Writes <out_prefix>.npz (x, y, u, v, w of the plane) and, only if matplotlib happens to be installed, <out_prefix>.png."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfcrl_env_amd import environments as envs  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
prefix = sys.argv[2] if len(sys.argv) > 2 else "flow_field"
env = envs.make("HornsRev1_Floris", env_batch=B, max_num_steps=50, wind_sampling="device")
obs = env.reset(seed=0)
for _ in range(5):  # a few steps of a toy wake-steering policy: every turbine creeps towards +20 deg
    obs, reward, terminated, truncated, info = env.step({"yaw": (20.0 - obs["yaw"]).clamp(-5, 5)})

# a met mast 3 rotor diameters west of the layout, at three heights, for every farm — at the envs' current yaw and wind
xs, ys = (np.asarray(env.farm_case.simul_params[k], float) for k in ("xcoords", "ycoords"))
mast = np.array([[xs.min() - 3 * 126.0, ys.mean(), z] for z in (40.0, 90.0, 140.0)])
uvw = env.sample_flow(mast)  # (B, 3, 3): farm, point, (u, v, w)
print("met mast u at 40 / 90 / 140 m, farm 0:", [round(float(v), 3) for v in uvw[0, :, 0]],
      "free wind:", [round(float(v), 3) for v in obs["freewind_measurements"][0]])

# the hub-height plane of farm 0 (the fused env's yaw state: yaw=None)
plane = env.fi.horizontal_plane(0, resolution=(200, 100))
np.savez(prefix + ".npz", **plane, layout_x=xs, layout_y=ys, yaw=env.fi.env_get_state()["yaw"][0],
         wind=np.asarray(obs["freewind_measurements"][0].cpu()))
print(f"plane {plane['u'].shape}: u from {plane['u'].min():.3f} to {plane['u'].max():.3f} m/s -> {prefix}.npz;",
      "kernels:", env.fi.probe_timing(plane=True))
try:
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
except ImportError:
    plt = None
if plt is not None:
    fig, ax = plt.subplots(figsize=(10, 5))
    im = ax.pcolormesh(plane["x"], plane["y"], plane["u"], shading="auto")
    ax.plot(xs, ys, "k.", ms=3)
    ax.set_aspect("equal")
    fig.colorbar(im, label="u [m/s]")
    fig.savefig(prefix + ".png", dpi=120)
    print(f"-> {prefix}.png")
torch.cuda.synchronize()
env.close()
