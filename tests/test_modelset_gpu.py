"""GPU: wake-model parameter sets per farm (include/wfmodelset.h: wf_set_model_sets; csrc/wf_resolve_ms.hip,
csrc/wf_resolve4_ms.hip, csrc/modelset/).

The checker is the unchanged CPU oracle, called once per set with that set's farms (`ModelParams(**set)`); tolerances are
the float64 contract of tests/test_resolve_gpu.py (parity.TOL_F64).  The device float64 kernel is compared with itself only
where BITS are asserted: the model as a set against plain mode 2, and a permutation of the farms against itself.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("ambient_ti", "shear", "veer", "alpha", "beta", "ka", "kb", "ad", "bd", "dm", "ch_initial", "ch_constant", "ch_ai",
          "ch_downstream", "defl_alpha", "defl_beta", "defl_ka", "defl_kb")
# four sets, every field taking another value in every set but the veer, which is off in two of them (both code paths)
SETS = {
    "ambient_ti": [0.04, 0.06, 0.09, 0.12], "shear": [0.08, 0.12, 0.16, 0.2], "veer": [0.0, 4.0, 0.0, -2.5],
    "alpha": [0.5, 0.58, 0.64, 0.7], "beta": [0.06, 0.077, 0.085, 0.095], "ka": [0.27, 0.38, 0.44, 0.49],
    "kb": [0.003, 0.004, 0.0046, 0.0052], "ad": [0.0, -1.0, 0.5, 2.0], "bd": [0.0, 0.002, -0.001, 0.001],
    "dm": [1.0, 0.9, 1.1, 1.05], "ch_initial": [0.08, 0.1, 0.12, 0.14], "ch_constant": [0.42, 0.5, 0.56, 0.62],
    "ch_ai": [0.72, 0.8, 0.86, 0.9], "ch_downstream": [-0.36, -0.32, -0.29, -0.26], "defl_alpha": [0.52, 0.6, 0.66, 0.72],
    "defl_beta": [0.065, 0.08, 0.088, 0.1], "defl_ka": [0.29, 0.36, 0.42, 0.47], "defl_kb": [0.0032, 0.0042, 0.0048, 0.0055],
}


def _set(k, sets=SETS):
    return {f: float(sets[f][k]) for f in FIELDS}


def _oracle_by_set(x, y, ws, wd, yaw, sets, set_of, extra=None):
    """The oracle once per set with that set's farms -> the batch's outputs; ws / wd of length 1 are shared."""
    from oracle import c_oracle
    from oracle.floris_gch_numpy import ModelParams

    yaw = np.asarray(yaw, dtype=np.float64)
    out = None
    for k in range(len(sets["ambient_ti"])):
        idx = np.flatnonzero(np.asarray(set_of) == k)
        if idx.size == 0:
            continue
        w = (ws, wd) if len(ws) == 1 else (ws[idx], wd[idx])
        r = c_oracle.farm_step_batch(x, y, w[0], w[1], yaw[idx], ModelParams(**_set(k, sets), **(extra or {})), margin=True)
        if out is None:
            out = {key: np.zeros((yaw.shape[0],) + np.shape(v)[1:]) for key, v in r.items()}
        for key, v in r.items():
            out[key][idx] = v
    return out


def _wind(rng, B, mode):
    if mode == "shared":
        return np.array([8.0]), np.array([270.0])
    return np.clip(8 * rng.weibull(8, B), 3, 28), rng.normal(270, 20, B) % 360


# (12 farms: the four-wave kernel on a short list, with its helper waves; Ablaincourt x 2048: past the switch to the one-wave
# kernel, which serves 7-turbine farms beyond one residency — csrc/wf_resolve.hip: wfk_launch_resolve)
CASES = [("Ablaincourt_", 12, 4), ("Turb16_Row5_", 12, 4), ("HornsRev1_", 12, 4), ("Ablaincourt_", 2048, 1)]


@pytest.mark.parametrize("name,B,waves", CASES)
@pytest.mark.parametrize("mode", ["shared", "per_env"])
def test_mixed_sets_are_the_oracle_per_set(layouts, name, B, waves, mode):
    import parity
    from wfcrl_env_amd.backend import WfStep

    l = layouts[name]
    N = l["num_turbines"]
    rng = np.random.default_rng(zlib.crc32(f"modelset/{name}/{B}/{mode}".encode()))
    set_of = rng.permutation(np.arange(B) % 4).astype(np.int32)  # every set is used, mixed over the farms
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    ws, wd = _wind(rng, B, mode)
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B, model_sets=SETS, model_set_of=set_of)
    assert w.risk_resolve() == 2
    w.set_wind(ws, wd)
    out = w.step(yaw)
    assert w.resolve_stats()["n_resolved"] == B and not w.risk_flags().any()
    assert w.model_sets_kernel() == waves
    ref = _oracle_by_set(l["xcoords"], l["ycoords"], ws, wd, yaw, SETS, set_of)
    parity.check_strict(out, ref, parity.TOL_F64)
    # ... and the sets matter: under the handle's one model the powers are somewhere else
    from oracle import c_oracle

    plain = c_oracle.farm_step_batch(l["xcoords"], l["ycoords"], ws, wd, yaw.astype(np.float64))
    assert np.abs(plain["power"] - ref["power"]).max() > 1e4
    got_sets, got_of = w.model_sets()
    assert np.array_equal(got_of, set_of) and all(np.array_equal(got_sets[f], np.asarray(SETS[f])) for f in FIELDS)
    w.close()


@pytest.mark.parametrize("B,waves", [(64, 4), (1500, 1)])
def test_the_model_as_a_set_is_plain_mode_two(layouts, B, waves):
    """A set equal to the model gives the bytes of the handle's own constants, hence the bits of mode 2 (both kernels)."""
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    N = l["num_turbines"]
    rng = np.random.default_rng(B)
    yaw = rng.uniform(-35, 35, (B, N)).astype(np.float32)
    ws, wd = _wind(rng, B, "per_env")
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B, model=dict(ambient_ti=0.07, veer=2.0, ka=0.35))
    w.set_risk_resolve(2)
    w.set_wind(ws, wd)
    plain = {k: np.array(v) for k, v in w.step(yaw).items()}
    one = w.model_set_from_model()
    assert (one["ambient_ti"], one["veer"], one["ka"], one["defl_ka"]) == (0.07, 2.0, 0.35, 0.35)
    w.set_model_sets([one], np.zeros(B, np.int32))
    got = w.step(yaw)
    assert w.model_sets_kernel() == waves
    for k in plain:
        assert np.array_equal(plain[k], np.asarray(got[k])), k
    w.close()


@pytest.mark.parametrize("name,B,waves", [("Turb16_Row5_", 2500, 4), ("Ablaincourt_", 5000, 1)])
def test_permuting_the_farms_permutes_the_outputs(layouts, name, B, waves):
    """A farm's result depends on its own set only — not on the farm a persistent block solved before it.  More farms than
    resident blocks (four-wave kernel: at most 4 per CU; one-wave kernel: 16 per CU), neighbouring farms on different sets."""
    from wfcrl_env_amd.backend import WfStep

    l = layouts[name]
    N = l["num_turbines"]
    rng = np.random.default_rng(B)
    set_of = (np.arange(B) % 4).astype(np.int32)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    ws, wd = _wind(rng, B, "per_env")
    perm = rng.permutation(B)
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B, model_sets=SETS, model_set_of=set_of)
    w.set_wind(ws, wd)
    first = {k: np.array(v) for k, v in w.step(yaw).items()}
    assert w.model_sets_kernel() == waves
    w.set_model_sets(SETS, set_of[perm])
    w.set_wind(ws[perm], wd[perm])
    second = w.step(yaw[perm])
    for k in first:
        assert np.array_equal(first[k][perm], np.asarray(second[k])), k
    assert np.abs(first["power"][0::4].mean() - first["power"][3::4].mean()) > 1e3  # (the sets differ in what they give)
    w.close()


def test_life_cycle(layouts):
    import parity
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    N, B = l["num_turbines"], 24
    rng = np.random.default_rng(11)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    ws, wd = _wind(rng, B, "per_env")
    set_of = (np.arange(B) % 4).astype(np.int32)
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B)
    w.set_risk_resolve(1)
    w.set_wind(ws, wd)
    plain = {k: np.array(v) for k, v in w.step(yaw).items()}
    w.set_model_sets(SETS, set_of)
    assert w.risk_resolve() == 2
    with pytest.raises(ValueError, match="mode 0 cannot be served"):
        w.set_risk_resolve(0)
    parity.check_strict(w.step(yaw), _oracle_by_set(l["xcoords"], l["ycoords"], ws, wd, yaw, SETS, set_of), parity.TOL_F64)
    # wf_set_model afterwards is honoured in the fields outside a set (here the air density and the recovery switch)
    w.set_model(dict(air_density=1.1, enable_yaw_added_recovery=False))
    ref = _oracle_by_set(l["xcoords"], l["ycoords"], ws, wd, yaw, SETS, set_of,
                         extra=dict(air_density=1.1, enable_yaw_added_recovery=False))
    parity.check_strict(w.step(yaw), ref, parity.TOL_F64)
    w.set_model({})
    # clearing restores the earlier mode and the earlier bits
    w.clear_model_sets()
    assert w.risk_resolve() == 1 and w.model_sets()[1].size == 0 and w.model_sets_kernel() == 0
    again = w.step(yaw)
    for k in plain:
        assert np.array_equal(plain[k], np.asarray(again[k])), k
    # another batch invalidates the assignment: the next step says so
    w.set_model_sets(SETS, set_of)
    w.set_batch(B // 2)
    w.set_wind(ws[:B // 2], wd[:B // 2])
    with pytest.raises(ValueError, match="set the parameter sets again"):
        w.step(yaw[:B // 2])
    w.set_model_sets(SETS, set_of[:B // 2])
    parity.check_strict(w.step(yaw[:B // 2]), _oracle_by_set(l["xcoords"], l["ycoords"], ws[:B // 2], wd[:B // 2], yaw[:B // 2], SETS,
                                                             set_of[:B // 2]), parity.TOL_F64)
    w.close()


def test_sets_with_turbine_definitions(layouts):
    import parity
    from oracle.floris_gch_numpy import ModelParams
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Ablaincourt_"]
    N, B = l["num_turbines"], 16
    rng = np.random.default_rng(21)
    base = ModelParams()
    derated = dict(table_ws=list(base.table_ws), table_ct=[0.9 * c for c in base.table_ct], table_cp=[0.8 * c for c in base.table_cp],
                   tsr=7.0, pP=2.0, gen_eff=0.95, ref_density=1.2)
    type_of = [0, 1, 1, 0, 1, 0, 1]
    two = {f: SETS[f][1:3] for f in FIELDS}
    set_of = rng.integers(0, 2, B).astype(np.int32)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    ws, wd = _wind(rng, B, "per_env")
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B, model=dict(turbine_defs=[{}, derated], turbine_type_of=type_of),
               model_sets=two, model_set_of=set_of)
    assert w.turbine_types() == 2
    w.set_wind(ws, wd)
    out = w.step(yaw)
    odefs = [{}, {("TSR" if k == "tsr" else k): v for k, v in derated.items()}]
    ref = _oracle_by_set(l["xcoords"], l["ycoords"], ws, wd, yaw, two, set_of, extra=dict(turbine_defs=odefs, turbine_type_of=type_of))
    parity.check_strict(out, ref, parity.TOL_F64)
    w.close()


def test_sets_with_two_layouts(layouts):
    import parity
    from wfcrl_env_amd.backend import WfStep

    rng = np.random.default_rng(31)
    N, B = 9, 20
    X, Y = rng.uniform(0, 2500, (2, N)), rng.uniform(0, 1500, (2, N))
    layout_of = rng.integers(0, 2, B).astype(np.int32)
    two = {f: SETS[f][2:4] for f in FIELDS}
    set_of = rng.integers(0, 2, B).astype(np.int32)
    yaw = rng.uniform(-30, 30, (B, N)).astype(np.float32)
    ws, wd = np.clip(8 * rng.weibull(8, B), 4, 20), rng.uniform(0, 360, B)
    w = WfStep(X, Y, env_batch=B, layout_of=layout_of, model_sets=two, model_set_of=set_of)
    w.set_wind(ws, wd)
    out = {k: np.asarray(v) for k, v in w.step(yaw).items()}
    for lay in range(2):
        idx = np.flatnonzero(layout_of == lay)
        ref = _oracle_by_set(X[lay], Y[lay], ws[idx], wd[idx], yaw[idx], two, set_of[idx])
        parity.check_strict({k: v[idx] for k, v in out.items()}, ref, parity.TOL_F64)
    w.close()


def test_refusals_by_name(layouts):
    from wfcrl_env_amd.backend import WfStep

    l = layouts["Turb3_Row1_"]
    N, B = l["num_turbines"], 4
    w = WfStep(l["xcoords"], l["ycoords"], env_batch=B)
    w.set_wind(8.0, 270.0)
    with pytest.raises(ValueError, match="outside 0..n_sets-1"):
        w.set_model_sets([{}, {"ka": 0.3}], [0, 1, 2, 0])
    with pytest.raises(ValueError, match="not finite"):
        w.set_model_sets([{"shear": float("nan")}], [0] * B)
    with pytest.raises(ValueError, match="ambient_ti must be > 0"):
        w.set_model_sets([{"ambient_ti": 0.0}], [0] * B)
    with pytest.raises(ValueError, match=r"unknown model-set field\(s\): \['air_density'\]"):
        w.set_model_sets([{"air_density": 1.1}], [0] * B)
    with pytest.raises(ValueError, match="1..env_batch"):
        w.set_model_sets([{}] * (B + 1), [0] * B)
    assert w.model_sets()[1].size == 0  # (a refused call leaves the handle as it was)
    w.set_model_sets([{}, {"ambient_ti": 0.1}], [0, 1, 0, 1])
    w.env_config(yaw_lo=-40, yaw_hi=40, yaw_step=5, actuator_rate=0.3, dt=60, budget=0.1, load_coef=0.1, discrete=False, power_mw=True)
    w.env_reset()
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wf_set_model_sets"):
        w.lookahead_returns(np.zeros((B, 2, 2, N), np.float32))
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wf_set_model_sets"):
        w.optimize_yaw(None)
    w.set_probe_points(np.array([[100.0, 0.0, 90.0]]))
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wf_set_model_sets"):
        w.sample_flow(np.zeros((B, N), np.float32))
    w.close()


def _host_env_with(params, name, **kw):
    """The reference-semantics env of tests/test_vec_env_gpu.py on the oracle, under another ModelParams."""
    from helpers import OracleStep
    from oracle import c_oracle
    from wfcrl_env_amd.environments.registration import get_case, get_default_control
    from wfcrl_env_amd.interface import HipFlorisInterface
    from wfcrl_env_amd.simple_env import WindFarmEnv

    class Step(OracleStep):
        def step(self, yaw, out=None):
            self.calls += 1
            yaw = np.asarray(yaw, np.float32).reshape(self.env_batch, self.num_turbines).astype(np.float64)
            r = c_oracle.farm_step_batch(self.x, self.y, self.ws, self.wd, yaw, params, nthreads=1)
            return {k: v.astype(np.float32) for k, v in r.items()}

    class Interface(HipFlorisInterface):
        def _make_backend(self, xcoords, ycoords, device_id, model):
            return Step(xcoords, ycoords)

    return WindFarmEnv(interface=Interface, farm_case=get_case(name, "Floris").clone(), controls=get_default_control(["yaw"]), **kw)


def test_env_with_explicit_sets_matches_reference_envs_per_set(layouts):
    import torch
    from oracle.floris_gch_numpy import ModelParams
    from wfcrl_env_amd import environments as envs

    name, B, T = "Turb6_Row2_", 6, 12
    N = layouts[name]["num_turbines"]
    three = {f: SETS[f][:3] for f in FIELDS}
    set_of = np.array([0, 1, 2, 2, 0, 1], np.int32)
    venv = envs.make(name + "Floris", env_batch=B, max_num_steps=T, load_coef=0.25,
                     model_randomization=dict(sets=three, set_of=set_of))
    assert np.array_equal(venv.model_set_of, set_of) and np.array_equal(venv.model_sets["ka"], three["ka"])
    obs = venv.reset(seed=77)
    fw = obs["freewind_measurements"].cpu().numpy()
    params = [ModelParams(**_set(k, three)) for k in range(3)]  # (built once per set)
    refs = []
    for b in range(B):
        e = _host_env_with(params[set_of[b]], name, max_num_steps=T, load_coef=0.25)
        o = e.reset(options={"wind_speed": fw[b, 0], "wind_direction": fw[b, 1]})
        assert np.abs(obs["wind_speed"][b].cpu().numpy() - o["wind_speed"]).max() < 2e-5 * 28
        refs.append(e)
    arng = np.random.default_rng(5)
    for step in range(5):
        a = arng.uniform(-7, 7, (B, N)).astype(np.float32)
        obs, rew, term, trunc, info = venv.step({"yaw": torch.from_numpy(a).cuda()})
        for b in range(B):
            o, r, t, tr, i = refs[b].step({"yaw": a[b].copy()})
            assert np.array_equal(obs["yaw"][b].cpu().numpy(), o["yaw"]), (step, b)  # float32 MDP arithmetic: exact
            assert abs(float(rew[b]) - r[0]) <= 3e-5 * abs(r[0]), (step, b, float(rew[b]), r[0])  # (test_vec_env_gpu.py's tolerance)
            assert np.allclose(info["power"][b].cpu().numpy(), i["power"], rtol=2e-4, atol=1e-6)
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wf_set_model_sets"):
        venv.optimal_yaw()
    with pytest.raises(ValueError, match="WF_E_UNSUPPORTED.*wf_set_model_sets"):
        venv.lookahead_returns(np.zeros((B, 2, 2, N), np.float32))
    venv.close()


def test_env_ranges_are_seeded_and_leave_the_wind_stream_alone(layouts):
    from wfcrl_env_amd import environments as envs

    name, B = "Turb6_Row2_", 8
    mr = dict(ranges={"ambient_ti": (0.04, 0.12), "ka": (0.27, 0.49)}, n_sets=4, resample="reset")
    a = envs.make(name + "Floris", env_batch=B, max_num_steps=20, return_torch=False, model_randomization=mr)
    b = envs.make(name + "Floris", env_batch=B, max_num_steps=20, return_torch=False, model_randomization=dict(mr))
    plain = envs.make(name + "Floris", env_batch=B, max_num_steps=20, return_torch=False)
    oa, ob, op = a.reset(seed=123), b.reset(seed=123), plain.reset(seed=123)
    for f in FIELDS:
        assert np.array_equal(a.model_sets[f], b.model_sets[f]), f
    assert np.array_equal(a.model_set_of, b.model_set_of) and a.model_sets["ka"].shape == (4,)
    assert ((a.model_sets["ambient_ti"] >= 0.04) & (a.model_sets["ambient_ti"] <= 0.12)).all() and len(set(a.model_sets["ka"])) == 4
    assert (a.model_sets["beta"] == 0.077).all()  # an unranged field is the model's
    assert plain.model_sets is None and plain.fi.risk_resolve() == 1 and a.fi.risk_resolve() == 2
    assert np.array_equal(oa["freewind_measurements"], op["freewind_measurements"])  # the wind stream of an env without sets
    assert np.array_equal(oa["wind_speed"], ob["wind_speed"])
    a.reset(seed=124)
    assert not np.array_equal(a.model_sets["ka"], b.model_sets["ka"])  # resample="reset": another seed, other sets
    # get_state / set_state: a fresh env resumes with the same bits
    rng = np.random.default_rng(0)
    acts = rng.uniform(-5, 5, (6, B, 6)).astype(np.float32)
    for x in acts[:3]:
        a.step(x)
    snap = a.get_state()
    first = [a.step(x) for x in acts[3:]]
    other = envs.make(name + "Floris", env_batch=B, max_num_steps=20, return_torch=False, model_randomization=dict(mr))
    other.reset(seed=99)
    other.set_state(snap)
    assert np.array_equal(other.model_set_of, a.model_set_of) and np.array_equal(other.model_sets["ka"], a.model_sets["ka"])
    for x, (o1, r1, _, t1, i1) in zip(acts[3:], first):
        o2, r2, _, t2, i2 = other.step(x)
        assert np.array_equal(o1["yaw"], o2["yaw"]) and np.array_equal(r1, r2) and np.array_equal(i1["power"], i2["power"])
    for e in (a, b, plain, other):
        e.close()
