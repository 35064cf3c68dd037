"""GPU: flow sampling at arbitrary points (include/wfprobe.h; csrc/probe/) against the numpy oracle with a ghost turbine
(tests/probe_ref.py), against the step itself, and the API's shapes, env path and refusals.

Tolerance 5e-7 of the free-stream speed on u, v and w: tests/parity.py TOL_F64's wind-speed bound, which the existing
float64 kernels meet against the same oracle with float32 outputs."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 5e-7
LAYOUTS = ["Turb3_Row1_", "Ablaincourt_", "Turb16_Row5_"]
WINDS = [270.0, 251.3, 93.0, "per_farm"]


def _ghost_case(layouts, name, wind, veer, model=None):
    """One parity case: B = 4 farms, six ghosts each (four behind turbines, two upstream of the farm) -> 54 points per
    farm as per-farm point sets; returns the device's (B, 54, 3) and the oracle's, plus the oracle's centre deficits."""
    import probe_ref
    from oracle.floris_gch_numpy import ModelParams
    from wfcrl_env_amd.backend import WfStep

    l = layouts[name]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    N, B = len(x), 4
    p0 = ModelParams(veer=veer, **(model or {}))
    rng = np.random.default_rng(zlib.crc32(f"probe/{name}/{wind}/{veer}/{sorted((model or {}).items())}".encode()))
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    if wind == "per_farm":
        ws, wd = rng.uniform(6.0, 12.0, B), rng.normal(270, 20, B) % 360
    else:
        ws, wd = np.full(B, rng.uniform(6.0, 12.0)), np.full(B, float(wind))
    pts = np.empty((B, 6, 3, 3, 3))
    ref = np.empty((B, 6, 3, 3, 3))
    down = np.zeros((B, 6), bool)
    for b in range(B):
        for _ in range(100):  # ghosts over the whole 3 D wide band; a set of which fewer than half of the four sit in a wake is drawn again
            for g, (gx, gy, dn) in enumerate(probe_ref.draw_ghosts(rng, x, y, wd[b])):
                # (exact under the centre-TI rule also where a source's TI grid is not uniform: probe_ref.ghost_uvw)
                ref[b, g], uniform = probe_ref.ghost_uvw(x, y, ws[b], wd[b], yaw[b].astype(np.float64), gx, gy, p0)
                if not uniform:
                    print(f"farm {b} ghost {g}: a source's TI grid is not uniform, side columns from shifted ghosts")
                pts[b, g] = probe_ref.ghost_points(gx, gy, wd[b], p0)
                down[b, g] = dn
            if (1.0 - ref[b, down[b], 1, 1, 0] / ws[b] > 0.05).mean() >= 0.5:
                break
    model = dict(model or {}, **({"veer": veer} if veer else {}))
    w = WfStep(x, y, env_batch=B, model=model or None)
    if wind == "per_farm":
        w.set_wind(ws, wd)
    else:
        w.set_wind(ws[0], wd[0])
    w.set_probe_points(pts.reshape(B, 54, 3), per_farm=True)
    got = w.sample_flow(yaw).reshape(B, 6, 3, 3, 3)
    w.close()
    deficit_c = 1.0 - ref[:, :, 1, 1, 0] / ws[:, None]  # the centre point lies at hub height: Uinit = ws
    return got, ref, ws, down, deficit_c


def _check_ghosts(got, ref, ws, down, deficit_c):
    # (on the oracle's values, so the test cannot be vacuous) at least half of the downstream ghosts sit in a wake
    assert (deficit_c[down] > 0.05).mean() >= 0.5, deficit_c[down]
    err = np.abs(got.astype(np.float64) - ref) / ws[:, None, None, None, None]
    print("max |err| / ws  u, v, w:", err[..., 0].max(), err[..., 1].max(), err[..., 2].max())
    assert err[..., 0].max() <= TOL, err[..., 0].max()
    assert err[..., 1].max() <= TOL, err[..., 1].max()
    assert err[..., 2].max() <= TOL, err[..., 2].max()


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("wind", WINDS)
def test_ghost_parity(layouts, name, wind):
    _check_ghosts(*_ghost_case(layouts, name, wind, 0.0))


def test_ghost_parity_with_veer(layouts):
    _check_ghosts(*_ghost_case(layouts, "Turb16_Row5_", "per_farm", 5.0))


@pytest.mark.parametrize("switch", ["enable_transverse_velocities", "enable_secondary_steering", "enable_yaw_added_recovery"])
def test_ghost_parity_with_a_solver_switch_off(layouts, switch):
    """The state kernel honours the model's switches (case.yaml:46-50); without transverse velocities v = w = 0 exactly."""
    got, ref, ws, down, deficit_c = _ghost_case(layouts, "Ablaincourt_", 251.3, 0.0, {switch: False})
    _check_ghosts(got, ref, ws, down, deficit_c)
    if switch == "enable_transverse_velocities":
        assert np.all(ref[..., 1:] == 0.0) and np.all(got[..., 1:] == 0.0)
    else:
        assert np.abs(ref[..., 1]).max() > 1e-3 * ws.min()


def test_free_stream(layouts):
    """Points upstream of every turbine: u = ws (z / HH)^shear, v = w = 0 exactly."""
    import probe_ref
    from oracle.floris_gch_numpy import ModelParams
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    B, N = 4, len(x)
    rng = np.random.default_rng(7)
    ws, wd = rng.uniform(5.0, 15.0, B), rng.normal(270, 20, B) % 360
    pts = np.empty((B, 12, 3))
    for b in range(B):
        xr, yr, back = probe_ref.wind_frame(x, y, wd[b])
        xp = xr.min() - rng.uniform(0.01, 20.0, 12) * 126.0
        yp = rng.uniform(yr.min() - 500.0, yr.max() + 500.0, 12)
        pts[b, :, 0], pts[b, :, 1] = back(xp, yp)
        pts[b, :, 2] = np.tile([10.0, 90.0, 200.0], 4)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    w.set_probe_points(pts, per_farm=True)
    got = w.sample_flow(rng.uniform(-30, 30, (B, N)).astype(np.float32))
    w.close()
    p0 = ModelParams()
    u_ref = ws[:, None] * (pts[:, :, 2] / p0.HH) ** p0.shear
    assert (np.abs(got[..., 0] - u_ref) / ws[:, None]).max() <= TOL
    assert np.all(got[..., 1] == 0.0) and np.all(got[..., 2] == 0.0)


def test_probes_on_the_rotor_grids_reproduce_the_step(layouts):
    """HornsRev1, 80 turbines: u sampled at the nine rotor-grid points of every turbine gives cbrt(mean u^3) equal to
    wf_step's wind_speed (float64 solve of every farm) within 1e-6 relative — two 5e-7 bounds against the same oracle.
    Only u: a probe ON a turbine has dx ~ +-1e-13 to it, where the dx < 0 mask of the transverse terms is ill-conditioned."""
    import probe_ref
    from wfcrl_env_amd.backend import WfStep

    l = layouts["HornsRev1_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    B, N = 2, len(x)
    rng = np.random.default_rng(11)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    pts = np.stack([probe_ref.ghost_points(x[t], y[t], 263.0) for t in range(N)]).reshape(N * 9, 3)
    w = WfStep(x, y, env_batch=B)
    w.set_risk_resolve(2)
    w.set_wind(8.0, 263.0)
    step = w.step(yaw)
    w.set_probe_points(pts)
    u = w.sample_flow(yaw)[..., 0].astype(np.float64).reshape(B, N, 9)
    w.close()
    ws_probe = np.cbrt((u ** 3).mean(axis=2))
    rel = np.abs(ws_probe / step["wind_speed"].astype(np.float64) - 1.0)
    print("max relative difference to wf_step's wind_speed:", rel.max())
    assert step["wind_speed"].min() < 0.8 * 8.0  # (deep wakes are in the comparison)
    assert rel.max() <= 1e-6, rel.max()


def test_shapes_farm_lists_and_point_sets(layouts):
    """P = 1, 257 (a second block with one live lane), 1000; a farm list returns the listed rows of the full result and a
    shared point set equals the same set repeated per farm, bit for bit; torch tensors give the bits NumPy gives."""
    import torch
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    B, N = 4, len(x)
    rng = np.random.default_rng(3)
    ws, wd = rng.uniform(5.0, 15.0, B), rng.normal(270, 20, B) % 360
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    allp = np.stack([rng.uniform(x.min() - 500, x.max() + 1500, 1000), rng.uniform(y.min() - 500, y.max() + 500, 1000),
                     rng.uniform(10.0, 200.0, 1000)], axis=1)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(ws, wd)
    res = {}
    for P in (1, 257, 1000):
        w.set_probe_points(allp[:P])
        res[P] = w.sample_flow(yaw)
        assert res[P].shape == (B, P, 3) and res[P].dtype == np.float32 and np.isfinite(res[P]).all()
        assert np.array_equal(w.sample_flow(yaw, farms=[2, 0]), res[P][[2, 0]])
        w.set_probe_points(np.repeat(allp[None, :P], B, axis=0), per_farm=True)
        assert np.array_equal(w.sample_flow(yaw), res[P])
    assert np.array_equal(res[1000][:, :257], res[257]) and np.array_equal(res[257][:, :1], res[1])
    assert (res[1000][..., 0] < 0.9 * ws[:, None]).any()  # (some points lie in wakes)
    w.set_probe_points(torch.from_numpy(allp).cuda())
    t = w.sample_flow(torch.from_numpy(yaw).cuda(), farms=[3, 1])
    w.sync()
    assert np.array_equal(t.cpu().numpy(), res[1000][[3, 1]])
    w.close()


def test_one_turbine_farm():
    import probe_ref
    from wfcrl_env_amd.backend import WfStep

    x, y = np.array([0.0]), np.array([0.0])
    ws, wd, yaw = 9.0, 250.0, np.array([[20.0]], np.float32)
    xr, yr, back = probe_ref.wind_frame(x, y, wd)
    gx, gy = back(xr[0] + 4.0 * 126.0, yr[0] + 30.0)
    r = probe_ref.ghost_fields(x, y, ws, wd, yaw[0].astype(np.float64), float(gx), float(gy))
    w = WfStep(x, y, env_batch=1)
    w.set_wind(ws, wd)
    w.set_probe_points(probe_ref.ghost_points(float(gx), float(gy), wd).reshape(9, 3))
    got = w.sample_flow(yaw).reshape(3, 3, 3).astype(np.float64)
    w.close()
    ref = np.stack([r["U"], r["V"], r["W"]], axis=-1)
    assert 1.0 - ref[1, 1, 0] / ws > 0.05
    assert np.abs(got - ref).max() <= TOL * ws, np.abs(got - ref).max()


def test_env_path_reads_the_yaw_state_and_leaves_the_env_alone():
    """After three steps of a batched env, sample_flow at the env's yaw state (the yaw == NULL path) equals sample_flow with
    that state passed explicitly, and the env's next step is bit-identical to a twin's that never sampled."""
    import torch
    from wfcrl_env_amd import environments as envs

    B = 8
    kw = dict(env_batch=B, max_num_steps=20, kernel_choice=dict(calibrate=False))
    env, twin = envs.make("Ablaincourt_Floris", **kw), envs.make("Ablaincourt_Floris", **kw)
    oa, ob = env.reset(seed=5), twin.reset(seed=5)
    gen = torch.Generator().manual_seed(0)
    for _ in range(3):
        a = (torch.rand((B, env.num_turbines), generator=gen) * 10.0 - 5.0).cuda()
        oa, ob = env.step({"yaw": a})[0], twin.step({"yaw": a})[0]
    xs, ys = (np.asarray(env.farm_case.simul_params[k], float) for k in ("xcoords", "ycoords"))
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(xs.min(), xs.max() + 1000, 40), rng.uniform(ys.min(), ys.max(), 40), rng.uniform(20.0, 160.0, 40)], axis=1)
    got = env.sample_flow(pts)
    state = env.fi.env_get_state()["yaw"]
    assert np.abs(state).max() > 1.0
    explicit = env.fi.sample_flow(state)
    assert tuple(got.shape) == (B, 40, 3) and np.array_equal(got.cpu().numpy(), explicit)
    assert (explicit[..., 0] < 0.95 * oa["freewind_measurements"][:, :1].cpu().numpy()).any()
    a = (torch.rand((B, env.num_turbines), generator=gen) * 10.0 - 5.0).cuda()
    ra, rb = env.step({"yaw": a}), twin.step({"yaw": a})
    for k in ra[0]:
        assert torch.equal(ra[0][k], rb[0][k]), k
    assert torch.equal(ra[1], rb[1]) and torch.equal(ra[4]["power"], rb[4]["power"]) and torch.equal(ra[4]["load"], rb[4]["load"])
    env.close()
    twin.close()


def test_env_sample_flow_sees_points_set_on_the_backend_in_between():
    """The env skips the upload of NumPy points the probe already holds; what it holds is remembered by the probe itself,
    so points set directly on env.fi between two env.sample_flow calls do not leave the env sampling at them."""
    from wfcrl_env_amd import environments as envs

    B = 2
    env = envs.make("Ablaincourt_Floris", env_batch=B, max_num_steps=20, kernel_choice=dict(calibrate=False))
    env.reset(seed=3)
    xs, ys = (np.asarray(env.farm_case.simul_params[k], float) for k in ("xcoords", "ycoords"))
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(xs.min(), xs.max() + 1000, 5), rng.uniform(ys.min(), ys.max(), 5), rng.uniform(20.0, 160.0, 5)], axis=1)
    first = env.sample_flow(pts).cpu().numpy()
    probe = env.fi._probe()
    assert probe.holds(pts, False) and not probe.holds(pts[None].repeat(B, 0), True)
    assert np.array_equal(env.sample_flow(pts.copy()).cpu().numpy(), first)  # the skipped upload changes nothing
    other = pts + np.array([300.0, 50.0, 10.0])
    env.fi.set_probe_points(other)
    assert not probe.holds(pts, False)
    elsewhere = env.fi.sample_flow(None)
    assert not np.array_equal(elsewhere, first)
    assert np.array_equal(env.sample_flow(pts).cpu().numpy(), first)
    env.close()


def test_refusals_name_their_cause(layouts):
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Turb3_Row1_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    yaw = np.zeros((2, 3), np.float32)
    pts = np.array([[2000.0, 0.0, 90.0]])
    w = WfStep(np.stack([x, x + 10.0]), np.stack([y, y]), env_batch=2)  # two layouts
    w.set_wind(8.0, 270.0)
    w.set_probe_points(pts)
    with pytest.raises(ValueError, match="several layouts"):
        w.sample_flow(yaw)
    w.close()
    w = WfStep(x, y, env_batch=2, model=dict(turbine_defs=[{}, {"tsr": 7.0}], turbine_type_of=[0, 1, 0]))  # two definitions
    w.set_wind(8.0, 270.0)
    w.set_probe_points(pts)
    with pytest.raises(ValueError, match="several turbine definitions"):
        w.sample_flow(yaw)
    w.close()
    w = WfStep(x, y, env_batch=2)
    with pytest.raises(ValueError, match="no wind"):
        w.set_probe_points(pts)
        w.sample_flow(yaw)
    w.close()
    w = WfStep(x, y, env_batch=2)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="no points"):
        w.sample_flow(yaw)
    with pytest.raises(ValueError, match="z > 0"):
        w.set_probe_points(np.array([[0.0, 0.0, -1.0]]))
    with pytest.raises(ValueError, match="fused env"):
        w.set_probe_points(pts)
        w.sample_flow(None)
    assert w.sample_flow(yaw, farms=[1]).shape == (1, 1, 3)  # (the handle still serves after refusals)
    w.close()


def test_horizontal_plane_is_sample_flow_on_a_grid(layouts):
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    B, N = 3, len(x)
    rng = np.random.default_rng(5)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(np.array([8.0, 9.0, 10.0]), np.array([270.0, 255.0, 180.0]))
    mast = np.array([[x.max() + 400.0, 0.0, 90.0]])
    w.set_probe_points(mast)
    before = w.sample_flow(yaw)
    p = w.horizontal_plane(1, resolution=(7, 5), yaw=yaw[1])
    assert p["x"].shape == (7,) and p["y"].shape == (5,) and all(p[k].shape == (5, 7) and p[k].dtype == np.float32 for k in "uvw")
    assert p["x"][0] == x.min() - 2 * 126.0 and p["x"][-1] > x.max() + 9 * 126.0  # 255 deg: the wind blows towards +x (and a little +y)
    X, Y = np.meshgrid(p["x"], p["y"])
    assert np.array_equal(w.sample_flow(yaw), before)  # the plane left the caller's points alone
    w.set_probe_points(np.stack([X.ravel(), Y.ravel(), np.full(X.size, 90.0)], axis=1))
    direct = w.sample_flow(yaw, farms=[1])[0].reshape(5, 7, 3)
    for i, k in enumerate("uvw"):
        assert np.array_equal(p[k], direct[..., i]), k
    p2 = w.horizontal_plane(2, height=50.0, x_bounds=(0.0, 100.0), y_bounds=(-50.0, 50.0), resolution=(3, 2), yaw=yaw)
    assert p2["u"].shape == (2, 3) and list(p2["x"]) == [0.0, 50.0, 100.0] and list(p2["y"]) == [-50.0, 50.0]
    w.close()


def test_interface_sample_flow_at_points(layouts):
    from wfcrl_env_amd.backend import WfStep
    from wfcrl_env_amd.interface import HipFlorisInterface

    l = layouts["Turb3_Row1_"]
    x, y = np.asarray(l["xcoords"], float), np.asarray(l["ycoords"], float)
    fi = HipFlorisInterface(3, list(x), list(y))
    fi.init(wind_speed=8.0, wind_direction=270.0)
    yaw = np.array([20.0, -10.0, 0.0])
    fi.update_command(yaw)
    px, py, pz = np.array([300.0, 800.0, 1500.0, -200.0]), np.array([0.0, 20.0, -30.0, 0.0]), np.array([90.0, 60.0, 120.0, 90.0])
    u = fi.sample_flow_at_points(px, py, pz)
    w = WfStep(x, y, env_batch=1)
    w.set_wind(fi.wind_speed, fi.wind_dir)
    w.set_probe_points(np.stack([px, py, pz], axis=1))
    ref = w.sample_flow(yaw.astype(np.float32)[None])[0, :, 0]
    w.close()
    assert u.shape == (4,) and u.dtype == np.float64 and np.array_equal(u, ref.astype(np.float64))
    assert u[0] < 0.8 * fi.wind_speed and u[3] == np.float32(fi.wind_speed)  # behind turbine 0; upstream of the farm at hub height
