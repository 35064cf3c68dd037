"""Flow sampling at arbitrary points: times the state and the sample kernel (csrc/probe/) with HIP events on the handle's stream
(wf_probe_last_timing: events around each launch) for the two cases of profiles/probe_timing.txt — (a) one HornsRev1 farm with a
200 x 100 hub-height plane, (b) 4096 farms x 16 points with a wind per farm — after 5 warm-ups, median of 30 repetitions, and
records the kernels' register / LDS footprint as the runtime reports it.
Run from the repo root on an MI355X:  python tools/probe_timing.py [output file, default profiles/probe_timing.txt]"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wfcrl_env_amd.backend import WfStep

lay = json.load(open(os.path.join(ROOT, "wfcrl-env_amd", "environments", "layouts.json")))["HornsRev1_"]
x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
N = len(x)
rng = np.random.default_rng(0)
lines = []

def run(w, yaw, label, reps=30, warm=5):
    st, sm = [], []
    out = None
    for k in range(warm + reps):
        out = w.sample_flow(yaw, out=out)
        t = w.probe_timing()
        if k >= warm:
            st.append(t["state_ms"]); sm.append(t["sample_ms"])
    lines.append(f"{label}: state kernel median {np.median(st)*1e3:.1f} us (min {np.min(st)*1e3:.1f}), sample kernel median {np.median(sm)*1e3:.1f} us (min {np.min(sm)*1e3:.1f}), {reps} repetitions after {warm} warm-ups")
    return out

# (a) one farm, 200 x 100 hub-height plane
w = WfStep(x, y, env_batch=1)
w.set_wind(8.0, 263.0)
X, Y = np.meshgrid(np.linspace(x.min() - 252, x.max() + 1260, 200), np.linspace(y.min() - 252, y.max() + 252, 100))
w.set_probe_points(torch.from_numpy(np.stack([X.ravel(), Y.ravel(), np.full(X.size, 90.0)], 1)).cuda())
yaw = torch.from_numpy(rng.uniform(-30, 30, (1, N)).astype(np.float32)).cuda()
o = run(w, yaw, "(a) HornsRev1, 1 farm x 20000 points (200 x 100 plane)")
lines.append(f"    plane u min {float(o[..., 0].min()):.3f} max {float(o[..., 0].max()):.3f}")
info = w.probe_kernel_info()
w.close()
# (b) 4096 farms x 16 points, a wind per farm
B = 4096
w = WfStep(x, y, env_batch=B)
w.set_wind(np.clip(8 * rng.weibull(8, B), 3, 28), rng.normal(270, 20, B) % 360)
pts = np.stack([rng.uniform(x.min() - 500, x.max() + 1500, (B, 16)), rng.uniform(y.min() - 500, y.max() + 500, (B, 16)), rng.uniform(20, 160, (B, 16))], -1)
w.set_probe_points(torch.from_numpy(pts).cuda(), per_farm=True)
yaw = torch.from_numpy(rng.uniform(-30, 30, (B, N)).astype(np.float32)).cuda()
o = run(w, yaw, "(b) HornsRev1, 4096 farms x 16 points, a wind per farm")
lines.append(f"    finite: {bool(torch.isfinite(o).all())}")
w.close()
lines.append(f"kernel footprint (hipFuncGetAttributes): state {info['state']}, sample {info['sample']} + 160 B dynamic LDS per turbine ({160 * N} B for HornsRev1)")
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probe_timing.txt")
head = ("Flow sampling at arbitrary points (csrc/probe/, tools/probe_timing.py): the two float64 kernels timed with HIP events on the\n"
        "handle's stream, one MI355X.\n")
open(out_path, "w").write(head + "\n".join(lines) + "\n")
print("\n".join(lines))
