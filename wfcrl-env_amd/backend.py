"""`WfStep` — thin object wrapper over the C ABI handle (one handle = one device + stream).

Accepts NumPy arrays (host path: staged through pinned buffers inside the library) or torch CUDA
tensors (device path: pointers handed over as-is, call is asynchronous on the handle's stream).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import EnvParams, KernelChoice, KernelInfo, ModelParams, WindDist, WindProcess, check


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


PROCESS = ("ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp")  # the keys of a wind process dict (include/wfwindgen.h)


def _wind_process(process, who=None) -> WindProcess:
    """A wind process dict as the library takes it (missing keys: 0).  `who`: the public method that needs one and names itself
    in the refusal of None (generate_wind's process is not optional: no name)."""
    if process is None and who:
        raise ValueError(f"{who} needs a wind process: dict(ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp)")
    unknown = set(process) - set(PROCESS)
    if unknown:
        raise ValueError(f"unknown wind process parameter(s): {sorted(unknown)}")
    return WindProcess(**{k: float(process.get(k, 0.0)) for k in PROCESS})


def _is_series(wind) -> bool:
    """wind="series": the series-ahead mode of lookahead, plan and credit (include/wfseries.h)."""
    return isinstance(wind, str) and wind == "series"


def default_model() -> dict:
    """Reference defaults (case.yaml + nrel_5MW) as a plain dict incl. the power/thrust table."""
    p = ModelParams()
    check(_lib.load().wf_default_model(C.byref(p)))
    d = {n: getattr(p, n) for n in _lib._MODEL_DOUBLES}
    d.update({n: bool(getattr(p, n)) for n in _lib._MODEL_SWITCHES})
    n = p.n_table
    d["table_ws"] = [p.table_ws[i] for i in range(n)]
    d["table_ct"] = [p.table_ct[i] for i in range(n)]
    d["table_cp"] = [p.table_cp[i] for i in range(n)]
    return d


def turbine_table(name: str = "nrel_5MW_floris3") -> dict:
    """A named power/thrust table shipped with the library (include/wfstep.h: wf_turbine_table) as the three model keys
    `table_ws`, `table_ct`, `table_cp` — e.g. WfStep(..., model=turbine_table("nrel_5MW_survey_a5"))."""
    n = C.c_int(0)
    dp = C.POINTER(C.c_double)
    ws, ct, cp = dp(), dp(), dp()
    check(_lib.load().wf_turbine_table(name.encode(), C.byref(n), C.byref(ws), C.byref(ct), C.byref(cp)))
    return {"table_ws": [ws[i] for i in range(n.value)], "table_ct": [ct[i] for i in range(n.value)],
            "table_cp": [cp[i] for i in range(n.value)]}


def wd_uncertainty_members(spec) -> tuple:
    """(delta (M,) float64 degrees, weight (M,) float64 — not normalised —, frame "fixed" | "relative"): the member set of
    a `wd_uncertainty` argument (include/wfrobust.h).  `spec` is one of two dicts:
      dict(delta=..., weight=..., frame="fixed")  the offsets and weights as they are
      dict(std=..., resolution=1.0, cutoff=0.995, frame="fixed")  a Gaussian table the way FLORIS users expect
          (UncertaintyInterface: std_wd, pmf_res, pdf_cutoff): bound = ceil(inv_cdf(cutoff) std / resolution),
          2 bound + 1 members at resolution x (-bound .. bound), weights exp(-delta^2 / (2 std^2))
    The default frame is "fixed": the nacelle stays where the nominal direction put it."""
    if not isinstance(spec, dict):
        raise ValueError("wd_uncertainty must be a dict: (delta, weight[, frame]) or (std[, resolution, cutoff, frame])")
    frame = spec.get("frame", "fixed")
    if frame not in ("fixed", "relative"):
        raise ValueError("wd_uncertainty: frame must be 'fixed' or 'relative'")
    if "std" in spec:
        if set(spec) - {"std", "resolution", "cutoff", "frame"}:
            raise ValueError("wd_uncertainty: give either (delta, weight) or (std, resolution, cutoff)")
        from statistics import NormalDist

        std, res, cutoff = float(spec["std"]), float(spec.get("resolution", 1.0)), float(spec.get("cutoff", 0.995))
        if not (std > 0.0 and res > 0.0 and 0.5 < cutoff < 1.0) or not np.isfinite(std + res):
            raise ValueError("wd_uncertainty: std and resolution must be > 0 and cutoff inside (0.5, 1)")
        bound = int(np.ceil(NormalDist().inv_cdf(cutoff) * std / res))
        delta = res * np.arange(-bound, bound + 1, dtype=np.float64)
        weight = np.exp(-(delta * delta) / (2.0 * std * std))
    else:
        if set(spec) - {"delta", "weight", "frame"} or "delta" not in spec or "weight" not in spec:
            raise ValueError("wd_uncertainty: give either (delta, weight) or (std, resolution, cutoff)")
        delta = np.ascontiguousarray(np.atleast_1d(spec["delta"]), dtype=np.float64)
        weight = np.ascontiguousarray(np.atleast_1d(spec["weight"]), dtype=np.float64)
        if delta.ndim != 1 or weight.shape != delta.shape:
            raise ValueError("wd_uncertainty: delta and weight must be 1-D and of one length")
    return delta, weight, frame


def normalize_model_sets(sets, base: dict) -> tuple:
    """({field: float64 array [S]} over the eighteen fields of include/wfmodelset.h, S) from a list of dicts or a dict of
    arrays; a field that is not given takes `base[field]` (the handle's model).  Unknown keys are refused by name; needs no
    device."""
    fields = _lib._MODEL_SET_FIELDS
    if isinstance(sets, dict):
        unknown = sorted(set(sets) - set(fields))
        if unknown:
            raise ValueError(f"unknown model-set field(s): {unknown} (a set may change: {list(fields)})")
        cols = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in sets.items()}
        sizes = {v.shape for v in cols.values()}
        if len(sizes) != 1 or len(next(iter(sizes))) != 1 or next(iter(sizes))[0] < 1:
            raise ValueError("model sets as a dict of arrays: every field needs one 1-D array of the same length S >= 1")
        S = next(iter(sizes))[0]
    else:
        sets = list(sets)
        if not sets or not all(isinstance(d, dict) for d in sets):
            raise ValueError("model sets: a list of dicts or a dict of arrays")
        unknown = sorted(set().union(*sets) - set(fields))
        if unknown:
            raise ValueError(f"unknown model-set field(s): {unknown} (a set may change: {list(fields)})")
        S = len(sets)
        cols = {k: np.array([float(d.get(k, base[k])) for d in sets], dtype=np.float64) for k in set().union(*sets)}
    out = {f: np.ascontiguousarray(cols[f]) if f in cols else np.full(S, float(base[f])) for f in fields}
    for f, v in out.items():
        if not np.isfinite(v).all():
            raise ValueError(f"model sets: {f} is not finite")
    if not (out["ambient_ti"] > 0.0).all():
        raise ValueError("model sets: ambient_ti must be > 0")
    return out, S


class WfStep:
    def __init__(self, xcoords, ycoords, env_batch: int = 1, device_id: int = 0, model: dict | None = None,
                 kernel_choice: dict | None = None, layout_of=None, model_sets=None, model_set_of=None):
        if model_sets is None and model_set_of is not None:
            raise ValueError("model_set_of comes with model_sets")
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.wf_create(int(device_id), C.byref(self._h)))
        self.device_id = int(device_id)
        self.num_turbines = 0
        self.env_batch = 0
        self._windgen_obj = None  # the wf_windgen object (include/wfwindgen.h), created on first use ...
        self._windgen = None  # ... and the same object while a generated wind episode is active (generate_wind), else None
        if model is not None:
            self.set_model(model)
        ragged = (not isinstance(xcoords, np.ndarray) and len(xcoords) > 0 and hasattr(xcoords[0], "__len__")
                  and len({len(r) for r in xcoords}) > 1)
        if ragged:  # layouts of different turbine counts: the handle holds the largest, shorter rows are padded (set_layouts)
            n = max(len(r) for r in xcoords)
            big = max(range(len(xcoords)), key=lambda l: len(xcoords[l]))
            self.set_layout(np.asarray(xcoords[big], np.float64), np.asarray(ycoords[big], np.float64))
            self.set_batch(env_batch)
            self.set_layouts(xcoords, ycoords, layout_of)
            self._apply_turbine_defs()
            if kernel_choice:
                self.set_kernel_choice(**kernel_choice)
            if model_sets is not None:
                self.set_model_sets(model_sets, model_set_of)
            return
        xy = np.asarray(xcoords, dtype=np.float64), np.asarray(ycoords, dtype=np.float64)
        if xy[0].ndim == 2:  # several layouts in the batch: [n_layouts][n_turbines], layout_of[env_batch] (set_layouts)
            self.set_layout(xy[0][0], xy[1][0])
            self.set_batch(env_batch)
            self.set_layouts(xy[0], xy[1], layout_of)
        else:
            if layout_of is not None:
                raise ValueError("layout_of needs 2-D coordinates [n_layouts][num_turbines]")
            self.set_layout(*xy)
            self.set_batch(env_batch)
        self._apply_turbine_defs()
        if kernel_choice:  # keyword arguments of set_kernel_choice: which kernels may serve this handle
            self.set_kernel_choice(**kernel_choice)
        if model_sets is not None:  # wake-model parameter sets per farm (set_model_sets)
            self.set_model_sets(model_sets, model_set_of)

    # -- configuration ---------------------------------------------------------------------------
    def set_model(self, model: dict):
        """Model constants + the power_thrust_table (keys of default_model()).  Two more keys describe a farm of SEVERAL
        turbine definitions (set_turbine_types): `turbine_defs`, `turbine_type_of`."""
        base = default_model()
        model = dict(model)
        self._turbine_defs = model.pop("turbine_defs", None)
        self._turbine_type_of = model.pop("turbine_type_of", None)
        if (self._turbine_defs is None) != (self._turbine_type_of is None):
            raise ValueError("turbine_defs and turbine_type_of come together")
        for k in ("alpha", "beta", "ka", "kb"):  # one gauss set given: the deflection model follows it (as in the template)
            if k in model and "defl_" + k not in model:
                model["defl_" + k] = model[k]
        unknown = set(model) - set(base)
        if unknown:
            raise ValueError(f"unknown model parameter(s): {sorted(unknown)}")
        base.update(model)
        p = ModelParams()
        for n in _lib._MODEL_DOUBLES:
            setattr(p, n, float(base[n]))
        for n in _lib._MODEL_SWITCHES:
            setattr(p, n, int(bool(base[n])))
        tws = np.ascontiguousarray(base["table_ws"], dtype=np.float64)
        tct = np.ascontiguousarray(base["table_ct"], dtype=np.float64)
        tcp = np.ascontiguousarray(base["table_cp"], dtype=np.float64)
        if not (len(tws) == len(tct) == len(tcp)):
            raise ValueError("power_thrust_table columns must have equal length")
        p.n_table = len(tws)
        dp = C.POINTER(C.c_double)
        p.table_ws, p.table_ct, p.table_cp = tws.ctypes.data_as(dp), tct.ctypes.data_as(dp), tcp.ctypes.data_as(dp)
        check(self._lib.wf_set_model(self._h, C.byref(p)), self._h)
        self._model = base
        if self.num_turbines:
            self._apply_turbine_defs()

    def _apply_turbine_defs(self):
        if getattr(self, "_turbine_defs", None) is not None:
            self.set_turbine_types(self._turbine_defs, self._turbine_type_of)
        elif self.turbine_types():
            self.set_turbine_types(None, None)

    def set_turbine_types(self, defs, type_of):
        """Several turbine definitions per farm (include/wfstep.h: wf_set_turbine_types; farm.turbine_type of a FLORIS case is
        a list): `defs` = up to 4 dicts with any of table_ws / table_ct / table_cp / tsr / pP / gen_eff / ref_density (missing:
        the model's value), `type_of[num_turbines]` the definition of each turbine.  The definitions share the rotor.  Every
        farm is then solved by the float64 kernels on every step (risk_resolve() reports 2).  None / [] clears them."""
        if not defs:
            check(self._lib.wf_set_turbine_types(self._h, 0, None, None), self._h)
            return
        base = getattr(self, "_model", None) or default_model()
        allowed = {"table_ws", "table_ct", "table_cp", "tsr", "pP", "gen_eff", "ref_density"}
        arr = (_lib.TurbineDef * len(defs))()
        keep = []
        dp = C.POINTER(C.c_double)
        for k, d in enumerate(defs):
            bad = set(d) - allowed
            if bad:
                raise ValueError(f"turbine definition {k}: {sorted(bad)} cannot differ between the definitions of one farm "
                                 f"(allowed: {sorted(allowed)})")
            cols = [np.ascontiguousarray(d.get(c, base[c]), dtype=np.float64) for c in ("table_ws", "table_ct", "table_cp")]
            if not (len(cols[0]) == len(cols[1]) == len(cols[2])):
                raise ValueError("power_thrust_table columns must have equal length")
            keep.append(cols)
            arr[k].n_table = len(cols[0])
            arr[k].table_ws, arr[k].table_ct, arr[k].table_cp = (c.ctypes.data_as(dp) for c in cols)
            for n in ("tsr", "pP", "gen_eff", "ref_density"):
                setattr(arr[k], n, float(d.get(n, base[n])))
        t = np.ascontiguousarray(type_of, dtype=np.int32)
        if t.shape != (self.num_turbines,):
            raise ValueError("turbine_type_of: one definition index per turbine of the layout")
        check(self._lib.wf_set_turbine_types(self._h, len(defs), arr, t.ctypes.data_as(C.POINTER(C.c_int))), self._h)

    def turbine_types(self) -> int:
        """Number of turbine definitions in force (0: the model's single one)."""
        n = C.c_int(0)
        check(self._lib.wf_get_turbine_types(self._h, C.byref(n)), self._h)
        return int(n.value)

    # -- wake-model parameter sets per farm (include/wfmodelset.h) ------------------------------------------------
    def model_set_from_model(self) -> dict:
        """The handle's model as a parameter set (wf_model_set_from_model): the starting point of a perturbation."""
        s = _lib.ModelSet()
        check(self._lib.wf_model_set_from_model(self._h, C.byref(s)), self._h)
        return {n: float(getattr(s, n)) for n in _lib._MODEL_SET_FIELDS}

    def set_model_sets(self, sets, set_of=None):
        """Wake-model parameter sets per farm (include/wfmodelset.h: wf_set_model_sets).  `sets`: a list of dicts of any of the
        eighteen fields of `_lib._MODEL_SET_FIELDS`, or a dict of arrays of one length S; a missing field is the handle's
        model.  `set_of[env_batch]`: the set of each farm (None: S == env_batch, farm b takes set b).  While sets are held
        EVERY farm is solved by the float64 kernels on every step (risk_resolve() reports 2): that is the cost.  None / []
        clears them (clear_model_sets)."""
        if sets is None or len(sets) == 0:
            return self.clear_model_sets()
        arr, S = normalize_model_sets(sets, self.model_set_from_model())
        so = None
        if set_of is not None:
            so = np.ascontiguousarray(set_of, dtype=np.int32)
            if so.shape != (self.env_batch,):
                raise ValueError("set_of must have one entry per env")
        c = (_lib.ModelSet * S)()
        for k in range(S):
            for n in _lib._MODEL_SET_FIELDS:
                setattr(c[k], n, float(arr[n][k]))
        check(self._lib.wf_set_model_sets(self._h, S, c, so.ctypes.data_as(C.POINTER(C.c_int)) if so is not None else None), self._h)

    def clear_model_sets(self):
        """Back to the handle's one model; the re-solve mode set before is in force again."""
        check(self._lib.wf_set_model_sets(self._h, 0, None, None), self._h)

    def model_sets(self):
        """(dict of float64 arrays of length S, set_of int32 [env_batch]) in force; ({field: empty}, empty) without sets."""
        n = C.c_int(0)
        check(self._lib.wf_get_model_sets(self._h, C.byref(n), None, None), self._h)
        S = int(n.value)
        if S == 0:
            return {f: np.zeros(0) for f in _lib._MODEL_SET_FIELDS}, np.zeros(0, np.int32)
        c = (_lib.ModelSet * S)()
        so = np.zeros(self.env_batch, np.int32)
        check(self._lib.wf_get_model_sets(self._h, C.byref(n), c, so.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        return {f: np.array([getattr(c[k], f) for k in range(S)], dtype=np.float64) for f in _lib._MODEL_SET_FIELDS}, so

    def model_sets_kernel(self) -> int:
        """Waves per farm of the float64 kernel behind the last step with sets: 4 (four-wave kernel), 1 (one-wave kernel), 0."""
        w = C.c_int(0)
        check(self._lib.wf_model_sets_last_kernel(self._h, C.byref(w)), self._h)
        return int(w.value)

    def set_layout(self, xcoords, ycoords):
        x = np.ascontiguousarray(xcoords, dtype=np.float64)
        y = np.ascontiguousarray(ycoords, dtype=np.float64)
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError("xcoords and ycoords layout coordinates must have the same length")
        check(self._lib.wf_set_layout(self._h, x.size, x.ctypes.data, y.ctypes.data), self._h)
        self.num_turbines = int(x.size)
        self._layout_xy = (x.copy(), y.copy())

    def set_layouts(self, xcoords, ycoords, layout_of=None, counts=None):
        """Several layouts in one batch (include/wfstep.h: wf_set_layouts): xcoords / ycoords [n_layouts][n_turbines],
        layout_of [env_batch] the layout of each farm (None: n_layouts == env_batch, farm b has layout b).  After
        set_batch; the wind has to be set again.
        Layouts of DIFFERENT turbine counts (wf_set_layouts_counts): `counts[l]` turbines of row l are real, or pass
        ragged lists of coordinates — rows are padded to the handle's turbine count; the outputs of the padding are 0."""
        if counts is None and not isinstance(xcoords, np.ndarray) and len({len(r) for r in xcoords}) > 1:
            counts = [len(r) for r in xcoords]  # ragged lists
            n = self.num_turbines
            if max(counts) > n or any(len(a) != len(b) for a, b in zip(xcoords, ycoords)):
                raise ValueError("every layout needs as many x as y coordinates, at most the handle's turbine count")
            xcoords = [list(r) + [0.0] * (n - len(r)) for r in xcoords]
            ycoords = [list(r) + [0.0] * (n - len(r)) for r in ycoords]
        x = np.ascontiguousarray(xcoords, dtype=np.float64)
        y = np.ascontiguousarray(ycoords, dtype=np.float64)
        if x.ndim != 2 or x.shape != y.shape or x.shape[1] != self.num_turbines:
            raise ValueError("xcoords and ycoords must both be [n_layouts][num_turbines]")
        cn = None
        if counts is not None:
            cn = np.ascontiguousarray(counts, dtype=np.int32)
            if cn.shape != (x.shape[0],):
                raise ValueError("counts must have one entry per layout")
        lo = None
        if layout_of is not None:
            lo = np.ascontiguousarray(layout_of, dtype=np.int32)
            if lo.shape != (self.env_batch,):
                raise ValueError("layout_of must have one entry per env")
        check(self._lib.wf_set_layouts_counts(self._h, x.shape[0], x.ctypes.data, y.ctypes.data, cn.ctypes.data if cn is not None else None,
                                              lo.ctypes.data if lo is not None else None), self._h)
        self.turbine_counts = None if cn is None else cn.copy()  # per layout; None: every layout has num_turbines

    def set_batch(self, env_batch: int):
        check(self._lib.wf_set_batch(self._h, int(env_batch)), self._h)
        self.env_batch = int(env_batch)
        self._windgen = None  # (a new batch has no wind: a generated episode ends)

    def set_stream(self, hip_stream: int | None, external: bool = True):
        """Adopt an external HIP stream (int handle; 0/None = the null stream) or, with external=False,
        return to the handle's own stream."""
        check(self._lib.wf_set_stream(self._h, C.c_void_p(hip_stream or 0), int(external)), self._h)
        self._stream_key = (int(hip_stream or 0), bool(external))

    def _follow_torch_stream(self):
        """Device tensors are produced/consumed on torch's current stream: run there too, so that no
        cross-stream synchronisation is needed around our kernels."""
        import torch

        s = torch.cuda.current_stream(self.device_id).cuda_stream
        if getattr(self, "_stream_key", None) != (int(s), True):
            self.set_stream(s, True)

    def set_wind(self, wind_speed, wind_direction):
        """Scalar (shared by the batch) or one value per env; NumPy/float or torch float64 CUDA tensors.  A speed per
        env with ONE direction (size-1 `wind_direction`) keeps the shared geometry and the pair-table path."""
        if _is_torch(wind_speed):
            ws, wd = wind_speed.contiguous().reshape(-1), wind_direction.contiguous().reshape(-1)
            assert ws.dtype == wd.dtype and str(ws.dtype) == "torch.float64" and ws.is_cuda and wd.is_cuda
            self._follow_torch_stream()
            self._windgen = None
            check(self._lib.wf_set_wind_counts(self._h, ws.data_ptr(), ws.numel(), wd.data_ptr(), wd.numel(), 1), self._h)
            return
        ws = np.ascontiguousarray(np.atleast_1d(wind_speed), dtype=np.float64)
        wd = np.ascontiguousarray(np.atleast_1d(wind_direction), dtype=np.float64)
        if ws.shape != wd.shape and wd.size != 1:
            raise ValueError("wind_speed and wind_direction must have the same shape (or one direction for all)")
        self._windgen = None  # (a wind set another way ends a generated episode)
        check(self._lib.wf_set_wind_counts(self._h, ws.ctypes.data, ws.size, wd.ctypes.data, wd.size, 0), self._h)

    def sample_wind(self, seed: int, dist: dict | None = None, direction_step: float | None = None):
        """On-device per-farm reset sampling (reference distributions by default, mdp.py:237-258).  `direction_step`
        (degrees, must divide 360; build-defined): directions rounded to that grid, farms grouped by direction, every
        step on the pair-table path (include/wfstep.h: wf_wind_sample_binned)."""
        d = None
        if dist is not None:
            base = dict(ws_scale=8.0, ws_shape=8.0, ws_lo=3.0, ws_hi=28.0, wd_mean=270.0, wd_std=20.0, wd_lo=0.0, wd_hi=360.0)
            base.update(dist)
            d = C.byref(WindDist(**base))
        s = C.c_ulonglong(int(seed) & (2**64 - 1))
        self._windgen = None
        if direction_step:
            check(self._lib.wf_wind_sample_binned(self._h, s, d, float(direction_step)), self._h)
        else:
            check(self._lib.wf_wind_sample(self._h, s, d), self._h)

    def set_wind_series(self, series, start=None, seed: int = 0):
        """series: (T, 2) [speed, direction]; start: (B,) ints or None (random per farm from `seed`)."""
        ts = np.ascontiguousarray(series, dtype=np.float64)
        if ts.ndim != 2 or ts.shape[1] < 2:
            raise ValueError("wind series must have shape (T, 2): speed, direction")
        ws, wd = np.ascontiguousarray(ts[:, 0]), np.ascontiguousarray(ts[:, 1])
        st = None if start is None else np.ascontiguousarray(start, dtype=np.int32)
        if st is not None and st.shape != (self.env_batch,):
            raise ValueError("start must have one entry per farm")
        self._windgen = None
        check(self._lib.wf_wind_series(self._h, ts.shape[0], ws.ctypes.data, wd.ctypes.data,
                                       None if st is None else st.ctypes.data, C.c_ulonglong(int(seed) & (2**64 - 1))), self._h)

    def wind_series_step(self):
        if self._windgen is not None:
            self._windgen.call("step")
            return
        check(self._lib.wf_wind_series_step(self._h), self._h)

    # -- synthetic wind episodes: a stochastic wind series per farm (include/wfwindgen.h) ---------------
    def generate_wind(self, T: int, seed: int, process: dict, dist: dict | None = None, ws0=None, wd0=None, kernel: str | None = None):
        """Generates a wind series of `T` ticks for every farm on the device (include/wfwindgen.h: DEFINITION) and starts
        playing it: the handle holds tick 0, and wind_series_step, wind_preview, series_state, series_seek and wind="series"
        of lookahead_returns, plan_actions, counterfactual_rewards, controller_returns and return_gradient work as on a
        series episode — every farm on a realisation of its own.  set_wind, sample_wind and set_wind_series end the episode.
          process   dict(ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp): reverts in [0, 1]; sigmas and ramp >= 0 (missing: 0)
          dist      tick 0's distribution (keys of sample_wind's; None: its default), whose ws_lo / ws_hi clip every speed
          ws0, wd0  (B,) float64: tick 0 given instead of drawn (both or neither)
          kernel    None: the library's choice; "serial" (a thread per farm) or "tiled" — the same bits, for measurements"""
        if kernel not in (None, "serial", "tiled"):
            raise ValueError('kernel must be None, "serial" or "tiled"')
        p = _wind_process(process)
        d = None
        if dist is not None:
            base = dict(ws_scale=8.0, ws_shape=8.0, ws_lo=3.0, ws_hi=28.0, wd_mean=270.0, wd_std=20.0, wd_lo=0.0, wd_hi=360.0)
            base.update(dist)
            d = C.byref(WindDist(**base))
        a0 = [None if a is None else np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (ws0, wd0)]
        for a in a0:
            if a is not None and a.shape != (self.env_batch,):
                raise ValueError("ws0 and wd0 must have one entry per farm")
        if self._windgen_obj is None:
            self._windgen_obj = _WindGen(self)
        self._windgen = None
        self._windgen_obj.call("set_kernel", {None: -1, "serial": 0, "tiled": 1}[kernel])
        self._windgen_obj.call("generate", int(T), C.c_ulonglong(int(seed) & (2**64 - 1)), d, C.byref(p),
                               *[None if a is None else a.ctypes.data for a in a0])
        self._windgen = self._windgen_obj

    def _generated(self) -> "_WindGen":
        if self._windgen is None:
            raise ValueError("no generated wind episode is active: generate_wind comes first")
        return self._windgen

    def generated_wind(self, farms=None, first: int = 0, n: int | None = None) -> np.ndarray:
        """(n_farms, n, 2) float64 [speed, direction]: ticks first .. first + n - 1 (None: to the last) of the generated series of
        the listed farms (None: all), read back from the device whatever the cursor is."""
        g = self._generated()
        fa = None if farms is None else np.ascontiguousarray(farms, dtype=np.int32).reshape(-1)
        nf = self.env_batch if fa is None else int(fa.size)
        first = int(first)
        n = g.state()["T"] - first if n is None else int(n)
        out = np.empty((nf, max(n, 0), 2), np.float64)
        g.call("read", first, n, nf, None if fa is None else fa.ctypes.data, out.ctypes.data)
        return out

    def generated_wind_state(self) -> dict:
        """What regenerates the active episode: {"T", "t", "prev_pending", "seed", "dist", "process"}."""
        return self._generated().state()

    def windgen_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the generator's kernel as the runtime reports them."""
        if self._windgen_obj is None:
            self._windgen_obj = _WindGen(self)
        return self._windgen_obj.kernel_info()

    # -- time-series episodes beyond reset / step (include/wfseries.h) ---------------------------------
    def wind_preview(self, H: int, first: int = 1, farms=None, as_torch: bool = False, out=None):
        """The window (first, H) of the wind series' coming rows (include/wfseries.h; a handle in series mode): entry h is
        the wind of tick min(t + first + h, T - 1).  first=1 starts at the wind of the coming env step (the env ticks before
        it steps), first=0 at the wind the handle holds.  Returns ((n, H, 2) float64 [speed, direction], available):
        `available` = clamp(T - t - first, 0, H) entries are real, the rest hold the last tick's wind.  as_torch (or a torch
        `out`): a CUDA tensor written by one kernel launch on torch's current stream, nothing read back; else NumPy.
          farms   farm indices (any order), or None: every farm of the batch"""
        H, first = int(H), int(first)
        fa = None if farms is None else np.ascontiguousarray(farms, dtype=np.int32).reshape(-1)
        n = self.env_batch if fa is None else int(fa.size)
        on_device = bool(as_torch) or _is_torch(out)
        if on_device:
            import torch

            self._follow_torch_stream()
            if out is None:
                out = torch.empty((n, max(H, 0), 2), dtype=torch.float64, device=f"cuda:{self.device_id}")
            assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (n, H, 2), "out"
            ptr = out.data_ptr()
        else:
            if out is None:
                out = np.empty((n, max(H, 0), 2), np.float64)
            assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (n, H, 2), "out"
            ptr = out.ctypes.data
        avail = C.c_int(0)
        if self._windgen is not None:
            self._windgen.call("window", first, H, n, None if fa is None else fa.ctypes.data, ptr, C.byref(avail), int(on_device))
            return out, int(avail.value)
        check(self._lib.wf_series_window(self._h, first, H, n, None if fa is None else fa.ctypes.data, ptr, C.byref(avail),
                                         int(on_device)), self._h)
        return out, int(avail.value)

    def series_state(self) -> dict:
        """The series cursor (include/wfseries.h: wf_series_get): {"T", "t" — ticks made since set_wind_series —, "start" (B,)
        int32, "prev_pending" — the speed of tick t - 1 waits for the next env step's reward}."""
        if self._windgen is not None:  # every farm plays its own series from row 0
            st = self._windgen.state()
            return {"T": st["T"], "t": st["t"], "start": np.zeros(self.env_batch, np.int32), "prev_pending": st["prev_pending"]}
        T, t, pending = C.c_int(), C.c_int(), C.c_int()
        start = np.empty(self.env_batch, np.int32)
        check(self._lib.wf_series_get(self._h, C.byref(T), C.byref(t), start.ctypes.data, C.byref(pending)), self._h)
        return {"T": int(T.value), "t": int(t.value), "start": start, "prev_pending": bool(pending.value)}

    def series_seek(self, t: int, prev_pending: bool = False):
        """Puts the handle in the state `t` ticks after set_wind_series would have left (include/wfseries.h: wf_series_seek);
        the series and the start rows stay.  On a generated episode: include/wfwindgen.h: wf_windgen_seek."""
        if self._windgen is not None:
            self._windgen.call("seek", int(t), int(bool(prev_pending)))
            return
        check(self._lib.wf_series_seek(self._h, int(t), int(bool(prev_pending))), self._h)

    def series_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the series kernel as the runtime reports them."""
        v = (C.c_int * 3)()
        check(self._lib.wf_series_kernel_info(self._h, v), self._h)
        return {"window": dict(zip(("vgprs", "lds_bytes", "scratch_bytes"), v))}

    def get_wind(self, as_torch: bool = False):
        """Current (ws, wd) of every farm: two float64 arrays of length B."""
        B = self.env_batch
        if as_torch:
            import torch

            self._follow_torch_stream()
            ws = torch.empty(B, dtype=torch.float64, device=f"cuda:{self.device_id}")
            wd = torch.empty_like(ws)
            check(self._lib.wf_get_wind(self._h, ws.data_ptr(), wd.data_ptr(), 1), self._h)
            return ws, wd
        ws, wd = np.empty(B), np.empty(B)
        check(self._lib.wf_get_wind(self._h, ws.ctypes.data, wd.ctypes.data, 0), self._h)
        return ws, wd

    # -- the step ----------------------------------------------------------------------------------
    def step(self, yaw, out: dict | None = None):
        """yaw: (B, N) absolute degrees.  Returns dict(power, wind_speed, wind_direction, load)."""
        B, N = self.env_batch, self.num_turbines
        if _is_torch(yaw):
            import torch

            assert yaw.is_cuda and yaw.dtype == torch.float32 and yaw.numel() == B * N
            yaw = yaw.contiguous()
            self._follow_torch_stream()
            if out is None:
                out = {
                    "power": torch.empty((B, N), device=yaw.device, dtype=torch.float32),
                    "wind_speed": torch.empty((B, N), device=yaw.device, dtype=torch.float32),
                    "wind_direction": torch.empty((B, N), device=yaw.device, dtype=torch.float32),
                    "load": torch.empty((B, N, 4), device=yaw.device, dtype=torch.float32),
                }
            check(self._lib.wf_step(self._h, yaw.data_ptr(), out["power"].data_ptr(), out["wind_speed"].data_ptr(),
                                    out["wind_direction"].data_ptr(), out["load"].data_ptr(), 1), self._h)
            return out
        yaw = np.ascontiguousarray(yaw, dtype=np.float32).reshape(B, N)
        if out is None:
            out = {
                "power": np.empty((B, N), np.float32),
                "wind_speed": np.empty((B, N), np.float32),
                "wind_direction": np.empty((B, N), np.float32),
                "load": np.empty((B, N, 4), np.float32),
            }
        check(self._lib.wf_step(self._h, yaw.ctypes.data, out["power"].ctypes.data, out["wind_speed"].ctypes.data,
                                out["wind_direction"].ctypes.data, out["load"].ctypes.data, 0), self._h)
        return out

    # -- flow sampling at arbitrary points (include/wfprobe.h) ---------------------------------------
    def _probe(self, plane: bool = False) -> "_Probe":
        """The handle's probe object for the caller's points, or the separate one horizontal_plane uses (so that a plane
        leaves set_probe_points' points alone); created on first use, destroyed in close() before the handle."""
        name = "_probe_plane" if plane else "_probe_points"
        pr = getattr(self, name, None)
        if pr is None:
            pr = _Probe(self)
            setattr(self, name, pr)
        return pr

    def set_probe_points(self, points, per_farm: bool = False):
        """The points `sample_flow` samples: (P, 3) [x, y, z] in the layout's coordinates, z the height above ground (> 0) —
        one set for every farm — or, with per_farm=True, (B, P, 3): a set per farm.  NumPy (validated: finite, z > 0; the
        call synchronises) or a torch float64 CUDA tensor (copied as it is, asynchronously)."""
        self._probe().set_points(points, per_farm)

    def sample_flow(self, yaw=None, farms=None, out=None):
        """The flow (u, v, w) [m/s] at the probe points: (n_farms, P, 3) float32, u along the wind, v lateral, w vertical.
          yaw    (B, N) absolute degrees — torch CUDA float32 tensor or NumPy — or None: the fused env's current yaw state
          farms  farm indices to solve and sample (any order, repeats allowed), or None: every farm of the batch
          out    a tensor / array to write into (a torch `out` selects the device path when yaw is None)
        The listed farms are solved in float64 at `yaw` under the handle's current wind, then sampled.  A probe value is
        what a rotor-grid point of one additional, wake-less turbine placed there would see in THIS project's sequential
        solve (include/wfprobe.h); it is not pinned to FLORIS' own full-flow solver (PARITY UNPINNED, as everything beyond
        the one known-answer vector)."""
        return self._probe().sample(yaw, farms, out)

    def probe_timing(self, plane: bool = False) -> dict:
        """HIP-event milliseconds of the two kernels of the last sample_flow (plane=True: of the last horizontal_plane):
        {"state_ms": the float64 farm solve, "sample_ms": the sampler}; synchronises."""
        return self._probe(plane).timing()

    def probe_kernel_info(self) -> dict:
        """Registers, static LDS bytes and private-segment bytes of the two probe kernels as the runtime reports them
        (hipFuncGetAttributes; tools/probe_timing.py records them next to the timings)."""
        return self._probe().kernel_info()

    def horizontal_plane(self, farm: int, height: float = None, x_bounds=None, y_bounds=None, resolution=(200, 100), yaw=None):
        """A horizontal cut through the flow of ONE farm of the batch (FLORIS: calculate_horizontal_plane): dict(x, y, u, v,
        w) with x (nx,), y (ny,) in the layout's coordinates and u / v / w (ny, nx) float32.  Python on top of sample_flow
        (same definition of a point value, same PARITY UNPINNED note).  Defaults: hub height; the layout's bounding box
        plus 2 rotor diameters on every side, stretched to 10 D on the side(s) the farm's wind blows towards.
        yaw: (N,) for this farm, (B, N), or None = the fused env's yaw state.  Leaves set_probe_points' points alone."""
        B, N = self.env_batch, self.num_turbines
        farm = int(farm)
        if not 0 <= farm < B:
            raise ValueError("farm index out of range")
        model = getattr(self, "_model", None) or default_model()
        D = float(model["rotor_diameter"])
        z = float(model["hub_height"] if height is None else height)
        lx, ly = self._layout_xy
        if x_bounds is None or y_bounds is None:
            wd = float(self.get_wind()[1][farm]) % 360.0
            dev = np.radians((wd - 270.0) % 360.0)
            ex, ey = np.cos(dev), -np.sin(dev)  # downstream direction in the layout's frame
            if x_bounds is None:
                x_bounds = (lx.min() - D * (2.0 + 8.0 * max(0.0, -ex)), lx.max() + D * (2.0 + 8.0 * max(0.0, ex)))
            if y_bounds is None:
                y_bounds = (ly.min() - D * (2.0 + 8.0 * max(0.0, -ey)), ly.max() + D * (2.0 + 8.0 * max(0.0, ey)))
        nx, ny = int(resolution[0]), int(resolution[1])
        x = np.linspace(float(x_bounds[0]), float(x_bounds[1]), nx)
        y = np.linspace(float(y_bounds[0]), float(y_bounds[1]), ny)
        X, Y = np.meshgrid(x, y)
        pr = self._probe(plane=True)
        pr.set_points(np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], axis=1), False)
        if yaw is not None:
            if _is_torch(yaw):
                yaw = yaw.detach().cpu().numpy()
            yaw = np.asarray(yaw, dtype=np.float32)
            if yaw.size == N:
                full = np.zeros((B, N), np.float32)
                full[farm] = yaw.reshape(N)
                yaw = full
        uvw = pr.sample(yaw, [farm], None)[0].reshape(ny, nx, 3)
        return {"x": x, "y": y, "u": uvw[..., 0].copy(), "v": uvw[..., 1].copy(), "w": uvw[..., 2].copy()}

    # -- batched yaw optimisation on the device (include/wfyawopt.h) -----------------------------------
    def _yawopt(self) -> "_YawOpt":
        """The handle's optimiser object; created on first use, destroyed in close() before the handle."""
        yo = getattr(self, "_yawopt_obj", None)
        if yo is None:
            yo = self._yawopt_obj = _YawOpt(self)
        return yo

    def optimize_yaw(self, yaw0=None, farms=None, bounds=(-25.0, 25.0), passes=(5, 4), strict=False, max_eval_farms=65536,
                     out=None, wd_uncertainty=None):
        """The best static yaw for the handle's current wind, by the project's own coordinate search (include/wfyawopt.h;
        in the spirit of "serial refine", not pinned to FLORIS' optimiser): turbines are visited upstream to downstream,
        pass 0 tries `passes[0]` angles across `bounds` per turbine, each later pass `passes[p]` angles inside the bracket
        the previous one left; the incumbent is always a candidate and only a strictly greater farm power replaces it.
          yaw0    (n_farms, N) start (row i belongs to farms[i]) — torch CUDA float32 tensor or NumPy — or None: zeros
          farms   farm indices to optimise (any order), or None: every farm of the batch
          strict  every candidate is evaluated in float64 (validation); otherwise the handle's own resolve mode
          max_eval_farms  farms the optimiser's evaluator handle may hold: longer lists run in chunks
          out     dict of tensors / arrays to write into (a torch `out` selects the device path when yaw0 is None)
        Returns dict(yaw (n_farms, N) degrees, power (n_farms,) W, power_initial (n_farms,) W at yaw0), float32.  With torch
        tensors the call only enqueues work on torch's current stream (include/wfyawopt.h lists when it has to wait);
        with NumPy it returns the results.  The handle itself — wind, env state, calibration — is not touched.
          wd_uncertainty  None: the wind direction is taken as exact.  A dict (`wd_uncertainty_members`): the ROBUST search
                  of include/wfrobust.h — the same search with "farm power" replaced by the expected power over the
                  direction offsets; power / power_initial are then expected powers, and max_eval_farms has to hold
                  (max(passes) + 1) x members rows per farm."""
        if wd_uncertainty is not None:
            return self._robust().optimize(yaw0, farms, bounds, passes, strict, max_eval_farms, out, wd_uncertainty)
        return self._yawopt().run(yaw0, farms, bounds, passes, strict, max_eval_farms, out)

    def yawopt_timing(self, detail=None) -> dict:
        """detail=True / False: the following optimize_yaw calls record (do not record) an event around every launch, so
        that step and glue time can be told apart — returns None.  detail=None: HIP-event milliseconds of the last
        optimize_yaw {"total_ms", "step_ms", "glue_ms"} (the last two 0 without detail); synchronises."""
        return self._yawopt().timing(detail)

    # -- wind-direction uncertainty: expected power and the robust yaw search (include/wfrobust.h) -----
    def _robust(self) -> "_Robust":
        """The handle's robust object; created on first use, destroyed in close() before the handle."""
        ro = getattr(self, "_robust_obj", None)
        if ro is None:
            ro = self._robust_obj = _Robust(self)
        return ro

    def uncertain_power(self, yaw=None, farms=None, wd_uncertainty=None, strict=False, max_eval_farms=65536, out=None):
        """Expected power under wind-direction uncertainty at a given yaw, for the handle's current wind: every farm is
        stepped once per member at (ws, wd + delta[m]) and the powers are averaged with the normalised weights
        (include/wfrobust.h; the project's own definition, PARITY UNPINNED beyond the oracle).
          yaw     (n_farms, N) degrees (row i belongs to farms[i]) — torch CUDA float32 tensor or NumPy — or None: zeros
          farms   farm indices (any order), or None: every farm of the batch
          wd_uncertainty  the member set, a dict `wd_uncertainty_members` understands; frame "fixed" (default): the nacelle
                  stays where the nominal direction put it, member m is stepped at yaw + delta[m]; "relative": at yaw
          strict  every member is solved in float64 (validation); otherwise the handle's own resolve mode
          max_eval_farms  rows (farm x member) the evaluator handle may hold: longer lists run in chunks
          out     dict of torch CUDA tensors expected_power (n,) float64, turbine_expected_power (n, N) float64,
                  member_power (n, M) float32 to write into (selects the device path when yaw is None)
        Returns dict(expected_power (n,) W, turbine_expected_power (n, N), member_power (n, M) float32, delta (M,),
        weight (M,) normalised).  Deterministic: fixed summation order, no atomics.  The handle is not touched."""
        if wd_uncertainty is None:
            raise ValueError("uncertain_power needs wd_uncertainty: dict(delta, weight[, frame]) or dict(std[, resolution, cutoff, frame])")
        return self._robust().evaluate(yaw, farms, strict, max_eval_farms, out, wd_uncertainty)

    def robust_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last robust optimize_yaw or uncertain_power {"total_ms", "step_ms", "glue_ms"}."""
        return self._robust().timing(detail)

    def robust_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the robust kernels as the runtime reports them."""
        return self._robust().kernel_info()

    # -- yaw sensitivities: power Jacobian and vector-Jacobian product (include/wfgrad.h) --------------
    def _grad(self) -> "_Grad":
        """The handle's gradient object; created on first use, destroyed in close() before the handle."""
        go = getattr(self, "_grad_obj", None)
        if go is None:
            go = self._grad_obj = _Grad(self)
        return go

    def yaw_gradient(self, yaw=None, cotangent=None, farms=None, step=1.0, bounds=(-45.0, 45.0), strict=False,
                     max_eval_farms=65536, jacobian=False, out=None):
        """How the power changes when a turbine turns, for the handle's current wind: the DIFFERENCE QUOTIENT of the step's
        per-turbine power at a finite step (include/wfgrad.h; the project's own definition, PARITY UNPINNED beyond the
        oracle) — not an analytic derivative of the kernels.  Turbine i is moved to y+ = float32(min(y + step, hi)) and
        y- = float32(max(y - step, lo)); d = y+ - y- is the divisor (one-sided at a bound, 0 sensitivity where d <= 0).
          yaw        (n_farms, N) degrees (row i belongs to farms[i]) — torch CUDA float32 tensor or NumPy — or None: zeros
          cotangent  (n_farms, N) float32 weights c of the per-turbine powers, or None: ones (the farm power)
          farms      farm indices (any order), or None: every farm of the batch
          strict     every row is solved in float64 (validation); otherwise the handle's own resolve mode
          max_eval_farms  rows the evaluator handle may hold, 2 N + 1 per farm: longer lists run in chunks
          jacobian   also return J (n_farms, N, N) float64, J[i, j] = d P_j / d yaw_i [W/deg]
          out        dict of tensors / arrays power (n, N) float32, gradient (n, N) float64[, jacobian (n, N, N) float64] to
                     write into (a torch `out` selects the device path when yaw is None)
        Returns dict(power — the forward value —, gradient G[i] = sum_j c_j J[i, j], summed over j in caller order in
        float64[, jacobian]).  Deterministic: fixed summation order, no atomics.  With torch tensors the call only enqueues
        work on torch's current stream; with NumPy it returns the results.  The handle is not touched."""
        return self._grad().run(yaw, cotangent, farms, step, bounds, strict, max_eval_farms, jacobian, out)

    def grad_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last yaw_gradient {"total_ms", "step_ms", "glue_ms"}."""
        return self._grad().timing(detail)

    def grad_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the gradient kernels as the runtime reports them."""
        return self._grad().kernel_info()

    # -- per-agent counterfactual rewards: difference rewards, COMA rows (include/wfcredit.h) ----------
    def _credit(self) -> "_Credit":
        """The handle's credit object; created on first use, destroyed in close() before the handle."""
        co = getattr(self, "_credit_obj", None)
        if co is None:
            co = self._credit_obj = _Credit(self)
        return co

    def counterfactual_rewards(self, base=None, alt=None, base_kind="yaw", alt_kind="yaw", farms=None, strict=False,
                               max_eval_farms=None, want=("reward", "difference"), out=None, wind=None):
        """What the farm's reward would have been had ONE turbine done something else, for the handle's current wind
        (include/wfcredit.h; the project's own definition, PARITY UNPINNED beyond the oracle): R = 1 + N K farm solves per
        farm in one batched step — row 0 the base, row 1 + i K + k the base with turbine i's entry replaced by alternative
        (i, k) — and each row's reward  mean_j(P_j [MW] 1e3 / ws^3) - load_coef mean|loads|  in float64.
          base       (n_farms, N) float32 (row i belongs to farms[i]) — torch CUDA tensor or NumPy — or None: the fused env's
                     current yaw state
          alt        (n_farms, N, K) float32, K alternatives per turbine (1 <= K <= 8; (n_farms, N) is K = 1), or None: one
                     alternative, the hold action (alt_kind "action") or zero yaw ("yaw")
          base_kind, alt_kind  "yaw": absolute degrees, used as given; "action": the env's encoding under env_config, turned
                     into a yaw by the fused step's own transition (budget gate, increment, clip) on the env state, which is
                     only read
          farms      farm indices (any order), or None: every farm of the batch
          strict     every row is solved in float64; otherwise the handle's own resolve mode.  A difference of two float32
                     rows is bounded only by twice the step's tolerance: use strict=True on large farms or where |D| is
                     small (include/wfcredit.h: WHEN TO USE strict)
          max_eval_farms  rows the evaluator handle may hold, 1 + N K per farm: longer lists run in chunks (None: 65 536)
          want       of "reward" (n, R) float64, "farm_power" (n, R) float64 [W], "difference" (n, N, K) float64 =
                     reward[:, 0] - reward[:, 1 + i K + k]
          out        dict of tensors / arrays of those names to write into (a torch `out` selects the device path when base
                     and alt are None)
          wind       None: the handle's current wind; "series" (a handle in series mode): the wind of the coming env step —
                     the series' next row, read on the device (include/wfseries.h) —, the reward normalised by the current
                     speed, as that step will
        Where an alternative's float32 yaw has the bits of the base entry, difference is exactly 0.0 and the row's reward
        and farm_power are copies of row 0's.  The reward is normalised by the speed the next env_step would normalise by
        (env_set_prev_wind is read, not consumed).  Deterministic: fixed summation order, no atomics.  With torch tensors
        the call only enqueues work on torch's current stream.  The handle is not touched."""
        return self._credit().run(base, alt, base_kind, alt_kind, farms, strict, max_eval_farms, want, out, wind)

    def credit_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last counterfactual_rewards {"total_ms", "step_ms", "glue_ms"}."""
        return self._credit().timing(detail)

    def credit_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the credit kernels as the runtime reports them."""
        return self._credit().kernel_info()

    # -- multi-step look-ahead returns of action sequences (include/wflookahead.h) ---------------------
    def _lookahead(self) -> "_Lookahead":
        """The handle's lookahead object; created on first use, destroyed in close() before the handle."""
        lo = getattr(self, "_lookahead_obj", None)
        if lo is None:
            lo = self._lookahead_obj = _Lookahead(self)
        return lo

    def lookahead_returns(self, actions, gamma=1.0, wind=None, farms=None, strict=False, max_eval_farms=65536,
                          want=("returns", "best"), out=None):
        """The discounted return the fused env would pay over the next H steps for each of K candidate action sequences,
        from the env state the handle holds, which is read and never changed (include/wflookahead.h; the project's own
        definition, PARITY UNPINNED beyond the oracle): the step's own transition (budget gate, increment, clip, accumulator,
        move counter) walks every sequence, the K H yaws of a farm are rows of one batched step, each row's reward is
        mean_j(P_j [MW] 1e3 / wr^3) - load_coef mean|loads| in float64 with wr the free-stream speed before that step, and
        ret = sum_h gamma^h r_h added in ascending h.
          actions    (n_farms, K, H, N) float32 in the env's encoding under env_config (block i belongs to farms[i]) — torch
                     CUDA tensor or NumPy; 1 <= H <= 64, K H <= 4096
          gamma      discount in [0, 1]
          wind       (n_farms, H, 2) float64 (speed, direction) the wind step h is solved under; None: the handle's
                     current wind held over the horizon (also in series mode); "series" (a handle in series mode): the
                     series' coming rows, read on the device — step h under the wind of tick t + 1 + h, the last row held
                     past the end, step 0 normalised by the current speed (include/wfseries.h)
          farms      farm indices (any order), or None: every farm of the batch
          strict     every row is solved in float64; otherwise the handle's own resolve mode.  Returns closer than the sum
                     of their rows' tolerances are not ordered reliably in the default mode
          max_eval_farms  rows the evaluator handle may hold, K H per farm: longer lists run in chunks
          want       of "returns" (n, K) float64, "rewards" (n, K, H) float64, "farm_power" (n, K, H) float64 [W],
                     "final_yaw" (n, K, N) float32 — the yaw after step H - 1 —, "best" (n,) int32 — the sequence of the
                     largest return, the lowest index among equal maxima
          out        dict of tensors / arrays of those names to write into
        Step 0 is normalised by the speed the next env_step would normalise by (env_set_prev_wind is read, not consumed).
        Deterministic: fixed summation order, no atomics.  With torch tensors the call only enqueues work on torch's current
        stream.  HipFlorisInterface has no such method: its MDP state lives in the host-side mdp.py, not in the handle."""
        return self._lookahead().run(actions, gamma, wind, farms, strict, max_eval_farms, want, out)

    def lookahead_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last lookahead_returns {"total_ms", "step_ms", "glue_ms"}."""
        return self._lookahead().timing(detail)

    def lookahead_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the lookahead kernels as the runtime reports them."""
        return self._lookahead().kernel_info()

    # -- closed-loop rollouts of MLP policies (include/wfpolicy.h) ---------------------------------------
    def _policy(self) -> "_Policy":
        """The handle's policy object; created on first use, destroyed in close() before the handle."""
        po = getattr(self, "_policy_obj", None)
        if po is None:
            po = self._policy_obj = _Policy(self)
        return po

    def policy_returns(self, params, spec, horizon, gamma=1.0, wind=None, farms=None, strict=False, max_eval_farms=65536,
                       want=("returns", "best"), out=None):
        """What each of K parameter vectors of one small MLP policy earns over the next `horizon` steps of the fused env, in
        closed loop, from the env state the handle holds, which is read and never changed (include/wfpolicy.h; the project's
        own definition, PARITY UNPINNED beyond the oracle).  The network observes what the env would show it — yaw, the
        per-turbine local wind speed and direction of the last solve, the free wind —, so a run is ONE batched step per env
        step, K rows per farm, with one glue kernel between two steps (reward, observation, network, transition) and no host
        read.  Round 0 solves the current yaw under the current wind for observation 0; rewards and returns are those of
        lookahead_returns: feeding "actions"[:, k] to it returns this call's rewards, returns and final_yaw bit for bit.
          params     (K, P) float32, 1 <= K <= 64 — torch CUDA tensor or NumPy; the same K policies for every farm; a vector
                     as torch.nn.utils.parameters_to_vector lays out an nn.Sequential of nn.Linear
          spec       policy.mlp_spec(...) (policy.policy_from_torch returns both)
          horizon    H, 1 <= H <= 256
          gamma      discount in [0, 1]
          wind       (n_farms, H, 2) float64 (speed, direction) the wind step h is solved under; None: the handle's current
                     wind held over the horizon
          farms      farm indices (any order), or None: every farm of the batch
          strict     every row is solved in float64; otherwise the handle's own resolve mode
          max_eval_farms  rows the evaluator handle may hold, K per farm: longer lists run in chunks
          want       of "returns" (n, K) float64, "rewards" (n, K, H) float64, "farm_power" (n, K, H) float64 [W], "actions"
                     (n, K, H, N) float32 — RAW, what env_step or lookahead_returns would be given —, "observations"
                     (n, K, H, 3 N + 2) float32 — un-normalised, the central lay-out for both kinds —, "final_yaw" (n, K, N)
                     float32, "gated" (n, K) int32 — (step, turbine) pairs with a closed budget gate —, "best" (n,) int32 —
                     the lowest index among equal maxima
          out        dict of tensors / arrays of those names to write into
        The network's arithmetic is float64 in a fixed order (input i ascending, product and sum rounded separately): with
        relu and softsign a NumPy loop reproduces the actions bit for bit, with tanh to one float32 ulp.  Step 0 is normalised
        by the speed the next env_step would normalise by (env_set_prev_wind is read, not consumed).  Deterministic: no
        floating-point atomics.  With torch tensors (params, wind or out) the call only enqueues work on torch's current
        stream and returns torch CUDA tensors."""
        return self._policy().run(params, spec, horizon, gamma, wind, farms, strict, max_eval_farms, want, out)

    def policy_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last policy_returns {"total_ms", "step_ms", "glue_ms"}."""
        return self._policy().timing(detail)

    def policy_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the policy kernels as the runtime reports them."""
        return self._policy().kernel_info()

    # -- policy rollouts over a wind ensemble (include/wfpolscen.h) ---------------------------------------
    def _polscen(self) -> "_PolScen":
        """The handle's policy-scenario object; created on first use, destroyed in close() before the handle."""
        po = getattr(self, "_polscen_obj", None)
        if po is None:
            po = self._polscen_obj = _PolScen(self)
        return po

    def policy_scenarios(self, params, spec, horizon, members, process, seed=0, gamma=1.0, tail=None, risk_weight=0.0, anchor=None,
                         bounds=(3.0, 28.0), farms=None, strict=False, max_eval_farms=65536,
                         want=("expected_returns", "cvar", "score", "best"), out=None) -> dict:
        """What each of K parameter vectors of one small MLP policy earns over the next `horizon` steps of the fused env in
        closed loop under each of `members` wind futures drawn from the wind process, from the wind and the env state the
        handle holds, which are read and never changed (include/wfpolscen.h; the project's own definition, PARITY UNPINNED
        beyond the oracle: tests/polscen_ref.py composes tests/scenario_ref.py and tests/policy_ref.py).  The network, the
        observation and the transition are policy_returns'; the member paths, their seed keying and the statistics are
        scenario_returns': `wind_paths` has the bits scenario_returns gives for the same (seed, members, horizon, process,
        bounds, anchor), and member m's outputs have the bits of policy_returns(wind=wind_paths[:, m]) while no prev-wind
        speed is pending (strict: always; default mode: where both evaluators' batches take the same step kernel).  Step 0 is normalised by the farm's current speed: a pending speed is neither used nor consumed.

          params, spec   as policy_returns takes them: (K, P) float32, 1 <= K <= 64, and policy.mlp_spec(...)
          horizon        H in 1..64;  members M in 1..64
          process        dict(ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp), missing keys 0
          tail           q in 1..M (None: M, the tail mean is the mean in another summation order)
          risk_weight    lam in [0, 1]: score = (1 - lam) mean + lam cvar
          anchor         (n_farms, 2) float64 the paths revert to, or None = every farm's current wind
          bounds         (ws_lo, ws_hi) the stored speeds are clipped to
          farms, strict, max_eval_farms   as policy_returns; the evaluator holds K M rows per farm
          want           of "expected_returns", "cvar", "score" (n, K), "member_returns" (n, K, M), "rewards", "farm_power"
                         (n, K, M, H), "wind_paths" (n, M, H, 2), "actions" (n, K, M, H, N), "observations"
                         (n, K, M, H, 3 N + 2), "final_yaw" (n, K, M, N), "gated" (n, K, M), "first_action" (n, K, N), "best" (n,)

        One batched step per env step, K M rows per farm, nothing read back in between.  Torch CUDA tensors in (params,
        anchor or `out`) give torch tensors out."""
        return self._polscen().run(params, spec, horizon, members, process, seed, gamma, tail, risk_weight, anchor, bounds, farms,
                                   strict, max_eval_farms, want, out)

    def policy_scenarios_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last policy_scenarios {"total_ms", "step_ms", "glue_ms"}."""
        return self._polscen().timing(detail)

    def policy_scenarios_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the kernels a policy_scenarios run launches."""
        return self._polscen().kernel_info()

    # -- policy search: CEM over MLP weights (include/wfpolsearch.h) --------------------------------------
    def _polsearch(self) -> "_PolSearch":
        """The handle's policy-search object, created on its policy and polscen objects on first use; destroyed in close()
        before them."""
        po = getattr(self, "_polsearch_obj", None)
        if po is None:
            po = self._polsearch_obj = _PolSearch(self)
        return po

    def search_policy(self, mean, spec, horizon, sigma=0.5, candidates=32, elites=8, iterations=4, sigma_min=0.0, seed=0, gamma=1.0,
                      wind=None, members=None, process=None, scenario_seed=0, tail=None, risk_weight=0.0, anchor=None,
                      bounds=(3.0, 28.0), farms=None, strict=False, max_eval_farms=65536,
                      want=("best_params", "best_fitness", "init_fitness", "mean", "sigma"), out=None) -> dict:
        """A cross-entropy search over the weights of one small MLP policy, in one call and on the device: per iteration K
        candidates — the incumbent, the mean, K - 2 Philox draws mean + sigma z per weight —, their fitness = the mean over the
        listed farms of policy_returns' return (or, with `members`, of policy_scenarios' score), the `elites` best refit mean
        and width per weight (include/wfpolsearch.h; the project's own definition, PARITY UNPINNED beyond the oracle:
        tests/search_ref.py).  The env state and the wind are read and never changed.  The rollouts run on the policy (or
        policy-scenario) object of this handle: policy_returns(candidates[i]) afterwards returns farm_scores[i] bit for bit.

          mean        (P,) float32 the start vector (policy.policy_from_torch gives one) — torch CUDA tensor or NumPy
          spec        policy.mlp_spec(...)
          horizon     H, the scorer's
          sigma       (P,) float32 widths >= 0, or a scalar for all weights
          candidates  K in 3..64;  elites E in 1..K;  iterations I in 1..16
          sigma_min   added to every refitted width (>= 0): the only schedule
          seed        of the draws: a draw depends on (seed, k, p, i) only
          gamma, wind, farms, strict, max_eval_farms   as policy_returns takes them
          members     None: policy_returns scores; M: policy_scenarios scores over M members with `process`, `scenario_seed`
                      (the same in every iteration), `tail`, `risk_weight`, `anchor`, `bounds`
          want        of "best_params" (P,) float32, "best_fitness", "init_fitness" () float64, "mean", "sigma" (P,) float32 —
                      the next call's warm start —, "fitness" (I, K) float64, "winner" (I,) int32, "candidates" (I, K, P)
                      float32, "sigma_history" (I, P) float32, "farm_scores" (I, n, K) float64
          out         dict of tensors / arrays of those names to write into
        Deterministic: fixed summation orders, no atomics; fitness[i][0] has the bits of max fitness[i - 1].  With torch
        tensors the call only enqueues work on torch's current stream and returns torch CUDA tensors."""
        return self._polsearch().run(mean, spec, horizon, sigma, candidates, elites, iterations, sigma_min, seed, gamma, wind, members,
                                     process, scenario_seed, tail, risk_weight, anchor, bounds, farms, strict, max_eval_farms, want, out)

    def search_policy_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last search_policy {"total_ms", "step_ms", "glue_ms"}: step_ms is the scorer's runs,
        glue_ms this extension's own kernels."""
        return self._polsearch().timing(detail)

    def search_policy_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the policy-search kernels as the runtime reports them."""
        return self._polsearch().kernel_info()

    # -- scenario look-ahead: returns of action sequences over a wind ensemble (include/wfscenario.h) ------
    def _scenario(self) -> "_Scenario":
        """The handle's scenario object; created on first use, destroyed in close() before the handle."""
        so = getattr(self, "_scenario_obj", None)
        if so is None:
            so = self._scenario_obj = _Scenario(self)
        return so

    def scenario_returns(self, actions, members, process, seed=0, gamma=1.0, tail=None, risk_weight=0.0, anchor=None,
                         bounds=(3.0, 28.0), farms=None, strict=False, max_eval_farms=65536,
                         want=("expected_returns", "cvar", "score", "best"), out=None):
        """The returns of K candidate action sequences over an ensemble of `members` wind futures drawn on the device from a
        wind process, from the wind and the env state the handle holds, which are read and never changed
        (include/wfscenario.h; the project's own definition, PARITY UNPINNED beyond the oracle).  Every farm draws M paths
        of H ticks that start at its current wind and revert to the anchor (Philox streams 16 to 18, keyed by the farm's index
        in the batch: the K sequences share the paths — common random numbers); step h of every sequence is solved under
        every member's wind of tick h + 1, the K M H rows of a farm in one batched step; a member's return is
        lookahead_returns' discounted sum, step 0 normalised by the current speed, step h by the member's speed of step
        h - 1; then per sequence the mean over the members, the tail mean (CVaR) of the `tail` lowest member returns and
        score = (1 - risk_weight) mean + risk_weight cvar, in float64 in fixed orders.
          actions    (n_farms, K, H, N) float32 in the env's encoding (block i belongs to farms[i]) — torch CUDA tensor or
                     NumPy; 1 <= H <= 64, K M H <= 4096
          members    M in 1..64
          process    dict(ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp) as generate_wind's (missing: 0)
          seed       64-bit seed of the draws
          gamma      discount in [0, 1]
          tail       q in 1..M (None: M, the tail mean is the mean in another summation order)
          risk_weight  lam in [0, 1]
          anchor     (n_farms, 2) float64 (speed > 0, direction) the paths revert to; None: every farm's current wind
          bounds     (ws_lo, ws_hi) the stored speeds are clipped to, 0 < ws_lo < ws_hi
          farms, strict, max_eval_farms   as lookahead_returns'; a farm takes K M H rows
          want       of "expected_returns", "cvar", "score" (n, K) float64, "member_returns" (n, K, M) float64, "rewards"
                     (n, K, M, H) float64, "wind_paths" (n, M, H, 2) float64 — (speed, direction) of tick h + 1 —,
                     "final_yaw" (n, K, N) float32, "best" (n,) int32 — the sequence of the largest score, the lowest index
                     among equal maxima
          out        dict of tensors / arrays of those names to write into
        Works under any wind the handle holds — set, sampled, a file series or a generated episode: only the current wind
        is read.  Deterministic: fixed summation orders, no atomics; any chunking and any farm list give the same bits in
        strict mode.  With torch tensors the call only enqueues work on torch's current stream."""
        return self._scenario().run(actions, members, process, seed, gamma, tail, risk_weight, anchor, bounds, farms, strict,
                                    max_eval_farms, want, out)

    def scenario_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last scenario_returns {"total_ms", "step_ms", "glue_ms"}."""
        return self._scenario().timing(detail)

    def scenario_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the scenario kernels as the runtime reports them."""
        return self._scenario().kernel_info()

    # -- the gradient of look-ahead returns w.r.t. the action sequences (include/wfretgrad.h) ------------
    def _retgrad(self) -> "_RetGrad":
        """The handle's retgrad object; created on first use, destroyed in close() before the handle."""
        ro = getattr(self, "_retgrad_obj", None)
        if ro is None:
            ro = self._retgrad_obj = _RetGrad(self)
        return ro

    def return_gradient(self, actions, gamma=1.0, wind=None, terminal=None, delta=1.0, farms=None, strict=False,
                        max_eval_farms=65536, want=("returns", "action_gradient"), out=None):
        """The derivative of lookahead_returns' H-step return with respect to the action sequences that produce it, from the
        env state the handle holds, which is read and never changed — call it before env_step (include/wfretgrad.h; the
        project's own definition, PARITY UNPINNED beyond the oracle).  The step's own transition walks every sequence and
        records where the gate and the two clips returned their input unchanged (the 0/1 transition Jacobian); per step the
        base yaw and a +- delta row per turbine are rows of one batched step — K H (2 N + 1) per farm —, q = (r+ - r-) / d is
        the reward's difference quotient (include/wfgrad.h's perturbation, one-sided at a yaw bound), and a backward sweep
        over the horizon, lam = gamma^h q + lam, in float64, carries it to every action.  Later gates' dependence on the
        accumulated actuation is piecewise constant: its derivative is taken as 0.  Continuous encoding only.
          actions    (n_farms, K, H, N) float32 (block i belongs to farms[i]) — torch CUDA tensor or NumPy; 1 <= H <= 64,
                     K H (2 N + 1) <= max_eval_farms
          gamma      discount in [0, 1]
          wind       as lookahead_returns: (n_farms, H, 2) float64, None (the current wind held) or "series"
          terminal   (n_farms, K, N) float64 or None (zeros): the derivative of a terminal value w.r.t. the final yaw
          delta      the perturbation in degrees
          farms, strict, max_eval_farms   as lookahead_returns; a quotient carries (bound+ + bound-) / d of the step's
                     tolerance, so strict=True is the mode for validation
          want       of "returns", "rewards", "farm_power", "final_yaw", "best" (lookahead_returns' base outputs),
                     "action_gradient" (n, K, H, N) float64 [reward / deg], "reward_gradient" (n, K, H, N) float64 — the
                     undiscounted q —, "state_gradient" (n, K, N) float64 — w.r.t. the yaw the env holds now —,
                     "yaw" (n, K, H, N) float32 — the trajectory —, "pass_mask" (n, K, H, N) uint8: bit 0 the action
                     passes, bit 1 the state passes
          out        dict of tensors / arrays of those names to write into
        Deterministic: fixed summation order, no atomics.  With torch tensors the call only enqueues work on torch's current
        stream."""
        return self._retgrad().run(actions, gamma, wind, terminal, delta, farms, strict, max_eval_farms, want, out)

    def return_gradient_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last return_gradient {"total_ms", "step_ms", "glue_ms"}."""
        return self._retgrad().timing(detail)

    def return_gradient_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the retgrad kernels as the runtime reports them."""
        return self._retgrad().kernel_info()

    # -- receding-horizon planner: CEM over action sequences (include/wfplan.h) ------------------------
    def _plan(self) -> "_Plan":
        """The handle's plan object; created on first use, destroyed in close() before the handle."""
        po = getattr(self, "_plan_obj", None)
        if po is None:
            po = self._plan_obj = _Plan(self)
        return po

    def plan_actions(self, horizon, candidates=64, elites=8, sigma=None, seed=0, gamma=1.0, wind=None, mean=None, farms=None,
                     strict=False, max_eval_farms=65536, want=("first_action", "plan_return"), out=None):
        """A receding-horizon plan for every farm, from the env state the handle holds, which is read and never changed
        (include/wfplan.h; the project's own definition, PARITY UNPINNED beyond the oracle): the cross-entropy method over
        (horizon, N) raw actions, continuous control only.  Each of len(sigma) iterations scores `candidates` sequences as
        lookahead_returns scores them — candidate 0 the best sequence so far (at first the hold: the plan is never worse
        than doing nothing), candidate 1 the mean, the others the mean plus sigma[i] times a unit-variance deviate of a
        counter-based generator, clipped to +-yaw_step — and moves the mean to the average of the `elites` best.  One glue
        kernel stands between two evaluator steps; nothing is read back in between.
          horizon    H, 1 <= H <= 64
          candidates K >= 3, K H <= 4096;  elites  1 <= E <= K
          sigma      one width per iteration, degrees, non-negative; None: (1, 1/2, 1/4) yaw_step
          seed       of the draws; a farm's draws depend on (seed, its index in the batch, iteration, element) alone
          gamma      discount in [0, 1]
          wind       (n_farms, H, 2) float64 (speed, direction) the wind step h is solved under; None: the handle's
                     current wind held over the horizon; "series": the series' coming rows, as lookahead_returns reads them
          mean       (n_farms, H, N) float32 the warm start, or None: zeros (receding horizon: the previous call's "mean"
                     shifted by one step)
          farms      farm indices (any order), or None: every farm of the batch
          strict     every row is solved in float64; otherwise the handle's own resolve mode
          max_eval_farms  rows the evaluator handle may hold, K H per farm: longer lists run in chunks
          want       of "plan" (n, H, N) float32 — the best sequence seen —, "plan_return" (n,) float64, "hold_return" (n,)
                     float64 — the return of doing nothing —, "first_action" (n, N) float32 — plan[:, 0], what to execute —,
                     "final_yaw" (n, N) float32 — the yaw after walking the plan —, "mean" (n, H, N) float32
          out        dict of tensors / arrays of those names to write into
        Deterministic: fixed summation order, no atomics.  With torch tensors (wind, mean or out) the call only enqueues
        work on torch's current stream and returns torch CUDA tensors."""
        return self._plan().run(horizon, candidates, elites, sigma, seed, gamma, wind, mean, farms, strict, max_eval_farms, want, out)

    def plan_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last plan_actions {"total_ms", "step_ms", "glue_ms"}."""
        return self._plan().timing(detail)

    def plan_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the plan kernel as the runtime reports them."""
        return self._plan().kernel_info()

    # -- wake-model calibration: parameter sets scored against and fitted to measured powers (include/wfcalib.h) ----
    def _calib(self) -> "_Calib":
        """The handle's calib object; created on first use, destroyed in close() before the handle."""
        co = getattr(self, "_calib_obj", None)
        if co is None:
            co = self._calib_obj = _Calib(self)
        return co

    def rated_power(self) -> float:
        """The largest power of the handle's table, watts: 1/2 rho_ref A Cp eta ws^3 — the default `scale` of a calibration."""
        m = getattr(self, "_model", None) or default_model()
        ws, cp = np.asarray(m["table_ws"], np.float64), np.asarray(m["table_cp"], np.float64)
        area = np.pi * (0.5 * float(m["rotor_diameter"])) ** 2
        return float(np.max(0.5 * float(m["ref_density"]) * area * cp * float(m["gen_eff"]) * ws ** 3))

    def model_loss(self, sets, ws, wd, yaw, power, weight=None, scale=None, out=None, want=("loss", "best"), max_eval_farms=65536):
        """The losses of candidate wake-model parameter sets against measured turbine powers (include/wfcalib.h:
        wf_calib_score; the project's own definition, PARITY UNPINNED beyond the oracle).  G problems of C conditions:
          sets    the candidates, as set_model_sets takes them: a list of S dicts or a dict of arrays [S], shared by all
                  problems — or a list of G such lists / a dict of arrays [G][S], a batch per problem
          ws, wd  (G, C) float64 the wind of each condition;  yaw (G, C, N) float32;  power (G, C, N) float64, watts
          weight  (G, C, N) float64 >= 0, or None: ones; 0 masks a turbine that was off-line or pads a problem: the power
                  under it may be anything, NaN included.  A NaN power under a positive weight is refused in NumPy arrays; in
                  torch tensors (not read on the host) it makes every loss of its problem +inf, and `best` is then 0
          scale   watts, > 0; None: rated_power()
          want    of "loss" (G, S) float64 — sum_c sum_t w ((P_dev - P) / scale)^2, float64 in a fixed order —, "best" (G,)
                  int32 — the lowest loss, the lowest index among equals —, "row_power" (G, S, C, N) float32
          max_eval_farms  rows the evaluator handle may hold, S C per problem: more problems run in chunks
        The leading G axis is optional: without it (ws of shape (C,)) the outputs have none either.  The handle supplies the
        model's other fields, its layout and its turbine; it needs no wind and is not changed.  Deterministic: two runs and
        any chunking give the same bits.  With torch tensors (the observations or out) the call only enqueues work on
        torch's current stream and returns torch CUDA tensors."""
        return self._calib().score(sets, ws, wd, yaw, power, weight, scale, out, want, max_eval_farms)

    def calibrate_model(self, ws, wd, yaw, power, bounds, init=None, candidates=64, elites=8, sigma=(0.25, 0.12, 0.06, 0.03),
                        seed=0, weight=None, scale=None, max_eval_farms=65536):
        """Fits wake-model fields to measured turbine powers on the device (include/wfcalib.h: wf_calib_fit; the project's
        own definition, PARITY UNPINNED beyond the oracle): the cross-entropy method of plan_actions over the eighteen
        fields of a parameter set, scored by model_loss.  One glue kernel stands between two evaluator steps; the
        candidates' constants are written on the device and nothing is read back in between.
          ws .. power, weight, scale   the observations, as model_loss takes them
          bounds      {field: (lo, hi)}: the fields to fit; every other field is FIXED at init
          init        the starting set(s): a dict, or a list of G dicts / dict of arrays [G]; missing fields and None: the
                      handle's model.  Inside the bounds
          candidates  S >= 3;  elites  1 <= E <= S
          sigma       one width per iteration (at most 16), a fraction of hi - lo, non-negative
          seed        of the draws; a problem's draws depend on (seed, its index, iteration, candidate, field) alone
        Returns a dict: "best_set" and "mean" as {field: array (G,)} — what set_model_sets accepts —, "best_loss",
        "init_loss" (G,), "history" (G, I) the winner's loss per iteration, "fit_power" (G, C, N) float32 the best set's
        powers, "n_invalid" (G,) int32 candidates that left the model's domain (their loss is +inf).  best_loss <= init_loss:
        candidate 0 is the best set so far, at first init.  Without a leading G axis the outputs have none either."""
        return self._calib().fit(ws, wd, yaw, power, bounds, init, candidates, elites, sigma, seed, weight, scale, max_eval_farms)

    def calib_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last model_loss / calibrate_model {"total_ms", "step_ms", "glue_ms"}."""
        return self._calib().timing(detail)

    def calib_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the calib kernel as the runtime reports them."""
        return self._calib().kernel_info()

    # -- scenario planner: CEM over action sequences scored over a wind ensemble (include/wfscenplan.h) ----
    def _scenplan(self) -> "_ScenPlan":
        """The handle's scenplan object; created on first use, destroyed in close() before the handle."""
        so = getattr(self, "_scenplan_obj", None)
        if so is None:
            so = self._scenplan_obj = _ScenPlan(self)
        return so

    def plan_scenarios(self, horizon, candidates=64, elites=8, members=8, process=None, sigma=None, seed=0, scenario_seed=0,
                       gamma=1.0, tail=None, risk_weight=0.0, anchor=None, bounds=(3.0, 28.0), mean=None, farms=None,
                       strict=False, max_eval_farms=65536,
                       want=("plan", "plan_score", "plan_expected", "plan_cvar", "plan_member_returns", "hold_score",
                             "first_action", "final_yaw", "mean", "wind_paths"), out=None):
        """A receding-horizon plan under wind uncertainty for every farm, from the wind and the env state the handle holds,
        which are read and never changed (include/wfscenplan.h; the project's own definition, PARITY UNPINNED beyond the
        oracle): plan_actions' cross-entropy method over (horizon, N) raw actions, every candidate scored as
        scenario_returns scores a sequence — over `members` wind futures drawn once per farm from the process, by
        score = (1 - risk_weight) mean + risk_weight cvar of its member returns.  The futures are the same for every
        candidate and every iteration (common random numbers), so the best sequence carried forward scores the same bits
        again and the plan's score never decreases.  One glue kernel stands between two evaluator steps.
          horizon    H, 1 <= H <= 64
          candidates K >= 3;  elites 1 <= E <= K;  members M in 1..64;  K M H <= 4096
          process    dict(ws_revert, ws_sigma, wd_revert, wd_sigma, wd_ramp) as generate_wind's (missing: 0)
          sigma      one width per iteration (at most 16), degrees, non-negative; None: (1, 1/2, 1/4) yaw_step
          seed       of the candidates' draws;  scenario_seed  of the member paths (scenario_returns' `seed`)
          gamma      discount in [0, 1]
          tail       q in 1..M (None: M);  risk_weight  lam in [0, 1]
          anchor     (n_farms, 2) float64 (speed > 0, direction) the paths revert to; None: every farm's current wind
          bounds     (ws_lo, ws_hi) the stored speeds are clipped to, 0 < ws_lo < ws_hi
          mean       (n_farms, H, N) float32 the warm start, or None: zeros
          farms, strict, max_eval_farms   as plan_actions'; a farm takes K M H rows
          want       of "plan" (n, H, N) float32, "plan_score", "plan_expected", "plan_cvar" (n,) float64 — the winner's in the
                     last iteration —, "plan_member_returns" (n, M) float64, "hold_score" (n,) float64 — the score of doing
                     nothing —, "first_action" (n, N) float32, "final_yaw" (n, N) float32, "mean" (n, H, N) float32,
                     "wind_paths" (n, M, H, 2) float64
          out        dict of tensors / arrays of those names to write into
        Returns a dict of the outputs.  Deterministic: fixed summation orders, no atomics.  With torch tensors (anchor, mean
        or out) the call only enqueues work on torch's current stream and returns torch CUDA tensors."""
        return self._scenplan().run(horizon, candidates, elites, members, process, sigma, seed, scenario_seed, gamma, tail,
                                    risk_weight, anchor, bounds, mean, farms, strict, max_eval_farms, want, out)

    def plan_scenarios_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last plan_scenarios {"total_ms", "step_ms", "glue_ms"}."""
        return self._scenplan().timing(detail)

    def plan_scenarios_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the scenplan kernels as the runtime reports them."""
        return self._scenplan().kernel_info()

    # -- wind-rose expected power and the yaw look-up table (include/wfrose.h) -------------------------
    def _rose(self) -> "_Rose":
        """The handle's rose object; created on first use, destroyed in close() before the handle."""
        ro = getattr(self, "_rose_obj", None)
        if ro is None:
            ro = self._rose_obj = _Rose(self)
        return ro

    def set_yaw_table(self, table, wd_axis, ws_axis, interp="linear", slot=0):
        """Store a yaw look-up table in `slot` (0..3): table (Dt, St, N) degrees — NumPy, or a torch CUDA float32 tensor
        with float64 CUDA axes, copied as it is — over wd_axis (Dt,) degrees, strictly ascending inside [0, 360), circular,
        and ws_axis (St,) m/s, strictly ascending, clamped at both ends.  interp "linear" (bilinear) or "nearest"; the
        look-up is the project's own definition (include/wfrose.h).  `expected_power` cases ("table", slot) and the
        look-up-table controller (`lut_policy`, VecWindFarmEnv.lut_action) read it."""
        self._rose().set_table(table, wd_axis, ws_axis, interp, slot)

    def expected_power(self, wd, ws, freq, cases=("zero",), cut_in=0.001, cut_out=None, strict=False, max_eval_farms=65536,
                       out=None):
        """Expected power over a wind rose: directions wd (D,), speeds ws (S,), frequencies freq (D, S) >= 0 (any scale).
          cases   each "zero", an (N,) yaw array held under every condition, or ("table", slot) — a table of set_yaw_table
                  looked up at every condition
          cut_in / cut_out   a condition with ws < cut_in or ws > cut_out counts as zero power (None: no cut-out)
          strict  every condition is solved in float64 (validation); otherwise the handle's own resolve mode
          max_eval_farms  rows (direction x case x speed) the rose's evaluator handle may hold: longer roses run in chunks
          out     dict of torch CUDA tensors weighted_power (C,) float64, weighted_turbine_power (C, N) float64,
                  condition_power (C, D, S) float32 to write into: the call then only enqueues work on torch's current
                  stream (include/wfrose.h lists when it has to wait) and the results are torch tensors
        Returns dict(expected_power (C,) W = sum(freq P) / sum(freq), aep_gwh (C,) = sum(freq P) x 8760 h / 1e9,
        turbine_expected_power (C, N), condition_power (C, D, S) float32, freq_sum).  The project's own interpolation and
        reduction (deterministic: fixed summation order, no atomics), not FLORIS' AEP routine; PARITY UNPINNED beyond the
        oracle.  The handle itself — wind, env state, calibration — is not touched."""
        return self._rose().evaluate(wd, ws, freq, cases, cut_in, cut_out, strict, max_eval_farms, out)

    def build_yaw_table(self, wd_axis, ws_axis, bounds=(-25.0, 25.0), passes=(5, 4), strict=False, wd_uncertainty=None):
        """Fill a yaw table with `optimize_yaw`: a private helper handle with this handle's layout and model and one farm
        per (direction, speed) node, a wind per farm, optimised in one call.  Returns dict(table (Dt, St, N) float32 —
        what set_yaw_table takes —, power (Dt, St) and power_initial (Dt, St): the optimiser's farm power at the optimum
        and at zero yaw).  wd_uncertainty: as in optimize_yaw — every node is then optimised for the expected power
        over the direction offsets, and the two powers are expected powers."""
        wd_axis = np.ascontiguousarray(np.atleast_1d(wd_axis), dtype=np.float64)
        ws_axis = np.ascontiguousarray(np.atleast_1d(ws_axis), dtype=np.float64)
        if wd_axis.ndim != 1 or ws_axis.ndim != 1 or wd_axis.size < 1 or ws_axis.size < 1:
            raise ValueError("wd_axis and ws_axis must be 1-D with at least one node each")
        if self.turbine_types():
            raise ValueError("WF_E_UNSUPPORTED: a yaw table is built for one turbine definition (and the layout of set_layout)")
        if self.model_sets()[1].size:
            raise ValueError("WF_E_UNSUPPORTED: a yaw table is built for one wake model: this handle holds parameter sets per farm")
        Dt, St = wd_axis.size, ws_axis.size
        x, y = self._layout_xy
        helper = WfStep(x, y, env_batch=Dt * St, device_id=self.device_id, model=getattr(self, "_model", None))
        try:
            helper.set_risk_resolve(self.risk_resolve())
            helper.set_wind(np.tile(ws_axis, Dt), np.repeat(wd_axis, St))
            r = helper.optimize_yaw(None, bounds=bounds, passes=passes, strict=strict, wd_uncertainty=wd_uncertainty)
        finally:
            helper.close()
        return {"table": r["yaw"].reshape(Dt, St, self.num_turbines), "power": r["power"].reshape(Dt, St),
                "power_initial": r["power_initial"].reshape(Dt, St)}

    def lut_policy(self, slot=0, want=("target_yaw", "action"), as_torch=False) -> dict:
        """The look-up-table controller for every farm: the table of `slot` at the farm's CURRENT wind (read on the device),
        clipped to the env's yaw bounds -> target_yaw (B, N); and the `action` (B, N) env_step takes to track it from the
        env's current yaw state under env_config (continuous: the difference clipped to +-yaw_step; discrete: 0 / 1 / 2).
        Reads the env state, never writes it (include/wfrose.h: wf_rose_policy)."""
        return self._rose().policy(slot, want, as_torch)

    def rose_timing(self) -> dict:
        """HIP-event milliseconds of the last expected_power {"total_ms", "step_ms", "glue_ms"}: the evaluator's wind + step
        calls, and the lay-out and reducing kernels; synchronises."""
        return self._rose().timing()

    def rose_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the rose kernels as the runtime reports them."""
        return self._rose().kernel_info()

    # -- closed-loop rollouts of yaw-table controllers (include/wfrollout.h) ---------------------------
    def _rollout(self) -> "_Rollout":
        """The handle's rollout object, created on its rose object on first use; destroyed in close() before it."""
        ro = getattr(self, "_rollout_obj", None)
        if ro is None:
            ro = self._rollout_obj = _Rollout(self)
        return ro

    @staticmethod
    def controller_grid(alphas, deadbands, leads, slot=0):
        """The full grid of look-up-table controllers over filter gains, deadbands [deg] and previews [steps] on table
        `slot`: (controllers, params) — the dict controller_returns takes and, index for index, the list of
        dict(slot, alpha, deadband, lead) each controller stands for (alpha slowest, lead fastest)."""
        params = [{"slot": int(slot), "alpha": float(a), "deadband": float(d), "lead": int(l)}
                  for a in np.atleast_1d(alphas) for d in np.atleast_1d(deadbands) for l in np.atleast_1d(leads)]
        controllers = {"slot": np.array([p["slot"] for p in params], np.int32), "alpha": np.array([p["alpha"] for p in params], np.float64),
                       "deadband": np.array([p["deadband"] for p in params], np.float32), "lead": np.array([p["lead"] for p in params], np.int32)}
        return controllers, params

    def controller_returns(self, controllers, horizon, gamma=1.0, wind=None, filter0=None, farms=None, strict=False,
                           max_eval_farms=65536, want=("returns", "best"), out=None):
        """What each of K look-up-table controllers earns over the next `horizon` steps of the fused env, in closed loop,
        from the env state the handle holds, which is read and never changed (include/wfrollout.h; the project's own
        definition, PARITY UNPINNED beyond the oracle).  At step h controller k observes the wind (obs[min(h + lead, H)],
        obs[0] the current wind, obs[j] the wind of step j - 1), filters it in float64 (fs += alpha (o_s - fs),
        fd += alpha wrap(o_d - fd); alpha 1 copies), looks the table of `slot` up at the filtered wind (set_yaw_table's
        tables, the look-up of lut_policy), clips the target to the env's yaw bounds, holds inside `deadband` degrees and
        else issues lut_policy's action; the action goes through the step's own budget gate, increment and clip.  The K H
        yaws of a farm are rows of one batched step; rewards and returns are those of lookahead_returns.
          controllers  dict of "slot" (default 0), "alpha" in (0, 1] (default 1), "deadband" >= 0 [deg] (default 0), "lead"
                       0..16 steps (default 0): scalars or sequences, broadcast to a common length K <= 64 — the same K
                       controllers for every farm.  alpha 1, deadband 0, lead 0 is what lut_policy's action does every step
          horizon      H, 1 <= H <= 1024, K H <= 4096
          gamma        discount in [0, 1]
          wind         (n_farms, H, 2) float64 (speed, direction) the wind step h is solved under; None: the handle's
                       current wind held; "series" (a handle in series mode): the series' coming rows, read on the device
          filter0      (n_farms, K, 2) float64 the filter states to start from — a previous call's "filter_final" —; None:
                       the farm's current wind
          farms        farm indices (any order), or None: every farm of the batch
          strict       every row is solved in float64; otherwise the handle's own resolve mode
          max_eval_farms  rows the evaluator handle may hold, K H per farm: longer lists run in chunks
          want         of "returns" (n, K) float64, "rewards" (n, K, H) float64, "farm_power" (n, K, H) float64 [W],
                       "actions" (n, K, H, N) float32 — the RAW actions: what env_step or lookahead_returns would be given —,
                       "final_yaw" (n, K, N) float32, "gated" (n, K) int32 — (step, turbine) pairs with a closed budget gate —,
                       "filter_final" (n, K, 2) float64, "best" (n,) int32 — the lowest index among equal maxima
          out          dict of tensors / arrays of those names to write into
        actions, final_yaw, gated and filter_final do not depend on the solver: the same bits in every mode.  Deterministic:
        fixed summation order, no floating-point atomics.  With torch tensors (wind, filter0 or out) the call only enqueues
        work on torch's current stream and returns torch CUDA tensors."""
        return self._rollout().run(controllers, horizon, gamma, wind, filter0, farms, strict, max_eval_farms, want, out)

    def rollout_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last controller_returns {"total_ms", "step_ms", "glue_ms"}."""
        return self._rollout().timing(detail)

    def rollout_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the rollout kernels as the runtime reports them."""
        return self._rollout().kernel_info()

    # -- scenario rollouts: yaw-table controllers in closed loop over a wind ensemble (include/wfrollscen.h) --
    def _rollscen(self) -> "_RollScen":
        """The handle's scenario-rollout object, created on its rose object on first use; destroyed in close() before it."""
        ro = getattr(self, "_rollscen_obj", None)
        if ro is None:
            ro = self._rollscen_obj = _RollScen(self)
        return ro

    def controller_scenarios(self, controllers, horizon, members, process, seed=0, gamma=1.0, tail=None, risk_weight=0.0,
                             anchor=None, bounds=(3.0, 28.0), filter0=None, farms=None, strict=False, max_eval_farms=65536,
                             want=("expected_returns", "cvar", "score", "best"), out=None):
        """What each of K look-up-table controllers earns over the next `horizon` steps of the fused env, in closed loop,
        under each of `members` wind futures drawn on the device from a wind process, from the wind and the env state the
        handle holds, which are read and never changed (include/wfrollscen.h; the project's own definition, PARITY UNPINNED
        beyond the oracle): controller_returns' controller under scenario_returns' paths, rows, rewards and statistics.
        Every farm draws M paths of H ticks that start at its current wind (scenario_returns' paths, bit for bit); under
        member m controller k observes obs[min(h + lead, H)] — obs[0] the current wind, obs[j] member m's tick j —, filters
        it, looks its table up, holds inside its deadband and goes through the step's own budget gate, increment and clip;
        the K M H yaws of a farm are rows of one batched step, row (k, m, h) solved under member m's tick h + 1; then per
        controller the mean over the members, the tail mean (CVaR) of the `tail` lowest member returns and
        score = (1 - risk_weight) mean + risk_weight cvar.  A controller with lead >= 1 previews ITS OWN member's future: a
        perfect forecast inside each scenario.
          controllers  as controller_returns takes them (controller_grid builds a tuning grid), K <= 64
          horizon      H in 1..64;  members  M in 1..64;  K M H <= 4096
          process, seed, gamma, tail, risk_weight, anchor, bounds   as scenario_returns'
          filter0      (n_farms, K, 2) float64 the filter states to start from, the same under every member; None: the
                       farm's current wind
          farms, strict, max_eval_farms   as scenario_returns'; a farm takes K M H rows
          want         of "expected_returns", "cvar", "score" (n, K) float64, "member_returns" (n, K, M) float64, "rewards"
                       (n, K, M, H) float64, "wind_paths" (n, M, H, 2) float64, "actions" (n, K, M, H, N) float32 — the RAW
                       actions —, "final_yaw" (n, K, M, N) float32, "gated" (n, K, M) int32, "first_action" (n, K, N)
                       float32 — member 0's action of step 0, the same under every member iff lead == 0 —, "best" (n,) int32 —
                       the controller of the largest score, the lowest index among equal maxima
          out          dict of tensors / arrays of those names to write into
        wind_paths, actions, final_yaw, gated and first_action do not depend on the solver: the same bits in every mode.
        Deterministic: fixed summation orders, no floating-point atomics; any chunking and any farm list give the same bits
        in strict mode.  With torch tensors (anchor, filter0 or out) the call only enqueues work on torch's current stream
        and returns torch CUDA tensors."""
        return self._rollscen().run(controllers, horizon, members, process, seed, gamma, tail, risk_weight, anchor, bounds,
                                    filter0, farms, strict, max_eval_farms, want, out)

    def controller_scenarios_timing(self, detail=None) -> dict:
        """As yawopt_timing, for the last controller_scenarios {"total_ms", "step_ms", "glue_ms"}."""
        return self._rollscen().timing(detail)

    def controller_scenarios_kernel_info(self) -> dict:
        """vgprs / static LDS bytes / private-segment bytes of the scenario-rollout kernels as the runtime reports them:
        "layout" (its brackets in LDS), "layout_spill" (its brackets in global memory), "reduce"."""
        return self._rollscen().kernel_info()

    # -- fused env step ---------------------------------------------------------------
    def env_config(self, yaw_lo=-40.0, yaw_hi=40.0, yaw_step=5.0, actuator_rate=0.3, dt=60.0, budget=0.1,
                   load_coef=0.1, discrete=False, power_mw=False):
        """power_mw: the `power` output of env_step in MW (include/wfstep.h: wf_env_set_power_unit) instead of W."""
        p = EnvParams(yaw_lo, yaw_hi, yaw_step, actuator_rate, dt, budget, load_coef, int(bool(discrete)))
        check(self._lib.wf_env_config(self._h, C.byref(p)), self._h)
        check(self._lib.wf_env_set_power_unit(self._h, int(bool(power_mw))), self._h)
        self._env_yaw_step = float(np.float32(yaw_step))  # (plan_actions' default widths are fractions of it)

    def env_reset(self):
        check(self._lib.wf_env_reset(self._h), self._h)

    def env_set_prev_wind(self, wind_speed):
        """Free-stream speed (B,) of the state before the coming env step, when it differs from the current wind
        (include/wfstep.h: wf_env_set_prev_wind); used once."""
        ws = np.ascontiguousarray(np.broadcast_to(np.asarray(wind_speed, np.float64), (self.env_batch,)))
        check(self._lib.wf_env_set_prev_wind(self._h, ws.ctypes.data, 0), self._h)

    def env_get_state(self, as_torch: bool = False) -> dict:
        """Copy of the device-resident env state: yaw (B, N), acc (B, N), moves (B,) — host NumPy arrays, or torch CUDA
        tensors (device-to-device, asynchronous on torch's current stream) with as_torch=True."""
        B, N = self.env_batch, self.num_turbines
        if as_torch:
            import torch

            self._follow_torch_stream()
            dev = f"cuda:{self.device_id}"
            st = {"yaw": torch.empty((B, N), dtype=torch.float32, device=dev), "acc": torch.empty((B, N), dtype=torch.float32, device=dev),
                  "moves": torch.empty(B, dtype=torch.int32, device=dev)}
            check(self._lib.wf_env_state(self._h, st["yaw"].data_ptr(), st["acc"].data_ptr(), st["moves"].data_ptr(), 0, 1), self._h)
            return st
        st = {"yaw": np.empty((B, N), np.float32), "acc": np.empty((B, N), np.float32), "moves": np.empty(B, np.int32)}
        check(self._lib.wf_env_state(self._h, st["yaw"].ctypes.data, st["acc"].ctypes.data, st["moves"].ctypes.data, 0, 0), self._h)
        return st

    def env_set_state(self, state: dict):
        B, N = self.env_batch, self.num_turbines
        yaw = np.ascontiguousarray(state["yaw"], np.float32).reshape(B, N)
        acc = np.ascontiguousarray(state["acc"], np.float32).reshape(B, N)
        moves = np.ascontiguousarray(state["moves"], np.int32).reshape(B)
        check(self._lib.wf_env_state(self._h, yaw.ctypes.data, acc.ctypes.data, moves.ctypes.data, 1, 0), self._h)

    def env_step(self, action=None, want=("reward", "yaw", "power", "wind_speed", "wind_direction", "load"), out=None):
        """One fused env step.  `action` (B, N) torch CUDA float32 tensor or NumPy array, or None for a solve
        at the current yaw (reset warm-up).  `want` selects which outputs are produced at all."""
        B, N = self.env_batch, self.num_turbines
        shapes = {"reward": (B,), "yaw": (B, N), "power": (B, N), "wind_speed": (B, N), "wind_direction": (B, N),
                  "load": (B, N, 4)}
        order = ("reward", "yaw", "power", "wind_speed", "wind_direction", "load")
        use_torch = _is_torch(action) or (action is None and out is not None and any(_is_torch(v) for v in out.values()))
        if use_torch:
            import torch

            dev = action.device if action is not None else next(iter(out.values())).device
            self._follow_torch_stream()
            if action is not None:
                assert action.is_cuda and action.dtype == torch.float32 and action.numel() == B * N
                action = action.contiguous()
            out = dict(out or {})
            for k in want:
                if k not in out:
                    out[k] = torch.empty(shapes[k], device=dev, dtype=torch.float32)
            ptrs = [out[k].data_ptr() if k in want else None for k in order]
            check(self._lib.wf_env_step(self._h, action.data_ptr() if action is not None else None, *ptrs, 1), self._h)
            return {k: out[k] for k in want}
        if action is not None:
            action = np.ascontiguousarray(action, dtype=np.float32).reshape(B, N)
        out = dict(out or {})
        for k in want:
            if k not in out:
                out[k] = np.empty(shapes[k], np.float32)
        ptrs = [out[k].ctypes.data if k in want else None for k in order]
        check(self._lib.wf_env_step(self._h, action.ctypes.data if action is not None else None, *ptrs, 0), self._h)
        return {k: out[k] for k in want}

    def sync(self):
        check(self._lib.wf_sync(self._h), self._h)

    def set_risk_guard(self, rel_band: float):
        """Relative half-width of the guard band around the overlap threshold (include/wfstep.h, WF_RISK_OVERLAP)."""
        check(self._lib.wf_set_risk_guard(self._h, float(rel_band)), self._h)

    def set_risk_resolve(self, mode: int | bool = 1):
        """Float64 re-solve of the farms the float32 kernels flag (include/wfstep.h: wf_set_risk_resolve): 1 / True the
        flagged farms (the DEFAULT of a new handle: every farm then meets the parity tolerances and its flag is 0), 2 every
        farm, 0 / False off (float32 only: flagged farms within the per-flag bounds of include/wfstep.h)."""
        check(self._lib.wf_set_risk_resolve(self._h, int(mode)), self._h)

    def risk_resolve(self) -> int:
        """The handle's re-solve mode (wf_get_risk_resolve): 0 off, 1 flagged farms, 2 every farm."""
        m = C.c_int(0)
        check(self._lib.wf_get_risk_resolve(self._h, C.byref(m)), self._h)
        return int(m.value)

    def resolve_stats(self) -> dict:
        """{"n_resolved": farms the last step solved in float64, "raw_flags": int32 (B,) flags before they were cleared}.
        Only meaningful after a step with the re-solve on: with it off (set_risk_resolve(0)) nothing is recorded and
        this raises instead of returning stale flags — read risk_flags() there."""
        if not self.risk_resolve():
            raise RuntimeError("resolve_stats() needs the float64 re-solve on (set_risk_resolve(1), the default); with it off "
                               "the flags of the last step are risk_flags()")
        n = C.c_int(0)
        raw = np.empty(self.env_batch, np.int32)
        check(self._lib.wf_get_resolve_stats(self._h, C.byref(n), raw.ctypes.data, 0), self._h)
        return {"n_resolved": int(n.value), "raw_flags": raw}

    def risk_flags(self, as_torch: bool = False):
        """WF_RISK_* bits of every farm for the last step: int32 (B,).  0 = every float64 decision of the reference
        was reproduced with a margin; see include/wfstep.h."""
        B = self.env_batch
        if as_torch:
            import torch

            self._follow_torch_stream()
            f = torch.empty(B, dtype=torch.int32, device=f"cuda:{self.device_id}")
            check(self._lib.wf_get_risk_flags(self._h, f.data_ptr(), 1), self._h)
            return f
        f = np.empty(B, np.int32)
        check(self._lib.wf_get_risk_flags(self._h, f.ctypes.data, 0), self._h)
        return f

    def timing_begin(self):
        check(self._lib.wf_timing_begin(self._h), self._h)

    def timing_end(self) -> float:
        ms = C.c_float()
        check(self._lib.wf_timing_end(self._h, C.byref(ms)), self._h)
        return float(ms.value)

    def set_kernel_choice(self, slot=None, one_block=None, pair_table=None, fly_one_block=None, far_skip=None, calibrate=None, mixed=None,
                          own_stage=None):
        """Which kernels may serve THIS handle (include/wfstep.h: wf_set_kernel_choice); None = automatic.
          slot=(G, S) or "16x5"      wf_step_kernel<G,S>
          one_block=False            never wf_step_ll_kernel;  one_block=(G, S) / "4x2" / "8": always, with that shape
          pair_table=False           everything on the fly
          fly_one_block=False        a wind per farm stays on wf_step_kernel
          far_skip=False             wf_step_ll_kernel evaluates every (source, target) pair (no far-source / far-pair skip)
          calibrate=False            the rounds model's guess stands: no timing of the kernel families before the first step
          mixed=False                always ONE launch per step (no whole-rounds + remainder split of the batch)
          own_stage=False / "always" wf_step_ll_kernel's own-source stage (set_own_stage): never / every block speculates
        Drops the current wind: set it again before the next step."""
        def gs(v, default_s=1):
            if isinstance(v, bool):
                raise ValueError("a kernel shape is (G, S), 'GxS' or G — not a bool (one_block=False disables the one-block "
                                 "kernel, None leaves the choice to the rounds model)")
            if isinstance(v, str):
                parts = v.lower().split("x")
                return int(parts[0]), (int(parts[1]) if len(parts) > 1 else default_s)
            if isinstance(v, int):
                return v, default_s
            return int(v[0]), int(v[1])

        c = KernelChoice(0, 0, -1, 0, 0, -1, -1, -1, -1, -1)
        if slot:
            c.slot_G, c.slot_S = gs(slot)
        if one_block is not None:
            if one_block is False or (not isinstance(one_block, bool) and one_block == 0):
                c.one_block = 0
            else:
                c.one_block = 1
                c.ll_G, c.ll_S = gs(one_block)
        if pair_table is not None:
            c.pair_table = int(bool(pair_table)) if pair_table is False else -1
        if fly_one_block is not None:
            c.fly_one_block = 0 if fly_one_block is False else -1
        if far_skip is not None:
            c.far_skip = 0 if far_skip is False or far_skip == 0 else -1
        if calibrate is not None:
            c.calibrate = 0 if calibrate is False or calibrate == 0 else -1
        if mixed is not None:
            c.mixed = 0 if mixed is False or mixed == 0 else -1
        check(self._lib.wf_set_kernel_choice(self._h, C.byref(c)), self._h)
        if own_stage is not None:
            self.set_own_stage(own_stage)

    def set_own_stage(self, mode):
        """The one-block kernel's own-source stage (include/wfstep.h: wf_set_own_stage): None / True where the kernel's
        pre-test allows, False never, "always" every block speculates (the fallback inside the kernel then does the work where
        the check fails: for tests).  Results are bit for bit the same in every setting.  Drops the current wind."""
        m = {None: -1, True: 1, False: 0, "always": 2}.get(mode, mode)
        check(self._lib.wf_set_own_stage(self._h, int(m)), self._h)

    def own_stage(self) -> dict:
        """{"mode": as set, "spec_blocks": (direction group, target block) pairs of the current wind that may run as a stage,
        "blocks": all of them} — the counts are 0 before the first step after the wind was set; reading them synchronises."""
        m, n, t = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.wf_get_own_stage(self._h, C.byref(m), C.byref(n), C.byref(t)), self._h)
        return {"mode": int(m.value), "spec_blocks": int(n.value), "blocks": int(t.value)}

    def kernel_choice(self) -> dict:
        c = KernelChoice()
        check(self._lib.wf_get_kernel_choice(self._h, C.byref(c)), self._h)
        return {n: getattr(c, n) for n, _ in KernelChoice._fields_}

    def calibration(self) -> dict:
        """What the per-handle kernel calibration found (include/wfstep.h: wf_get_calibration): {"shape": "2x2" / "16x5-slot
        kernel" ... or None when it has not run, "family_ms": {family: ms per launch} of the families it timed; "on_the_fly":
        which kernel the timing on the on-the-fly path (a wind per farm) kept, None before it ran}."""
        code = C.c_int(-1)
        ms = (C.c_float * 6)()
        check(self._lib.wf_get_calibration(self._h, C.byref(code), ms), self._h)
        names = ("slot", "8x1", "4x2", "4x1", "2x2", "16x1")
        shape = None if code.value < 0 else ("slot" if code.value == 0 else f"{code.value >> 4}x{code.value & 15}")
        fly, fms = C.c_int(0), (C.c_float * 2)()
        check(self._lib.wf_get_fly_calibration(self._h, C.byref(fly), fms), self._h)
        mixn, mixms = C.c_int(0), C.c_float(0.0)
        check(self._lib.wf_get_mixed_launch(self._h, C.byref(mixn), C.byref(mixms)), self._h)
        return {"shape": shape, "family_ms": {n: float(m) for n, m in zip(names, ms) if m > 0.0},
                "on_the_fly": (None, "one_block", "slot")[fly.value], "on_the_fly_ms": {n: float(m) for n, m in zip(("one_block", "slot"), fms) if m > 0.0},
                "mixed_main_farms": int(mixn.value), "mixed_ms": float(mixms.value)}

    def calibrate(self):
        """Time the kernel families NOW for the current layout / batch / wind (include/wfstep.h: wf_calibrate; synchronises) —
        otherwise the first step of a configuration does it (or takes the process-wide cached result)."""
        check(self._lib.wf_calibrate(self._h), self._h)

    _FAMILY_CODES = {"slot": 0, "8x1": (8 << 4) | 1, "4x2": (4 << 4) | 2, "4x1": (4 << 4) | 1, "2x2": (2 << 4) | 2, "16x1": (16 << 4) | 1}

    def set_calibration(self, shape=None, on_the_fly=None):
        """Take a saved calibration as is — `shape` and `on_the_fly` as calibration() returned them (None: leave that one
        to the timing); nothing is timed for this configuration afterwards (wf_set_calibration)."""
        code = -1 if shape is None else self._FAMILY_CODES[shape]
        fly = {None: 0, "one_block": 1, "slot": 2}[on_the_fly]
        check(self._lib.wf_set_calibration(self._h, code, fly), self._h)

    def kernel_info(self) -> dict:
        k = KernelInfo()
        check(self._lib.wf_get_kernel_info(self._h, C.byref(k)), self._h)
        return {n: getattr(k, n) for n, _ in KernelInfo._fields_}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            # an extension object goes before its handle (include/wfprobe.h, wfyawopt.h, wfrose.h, wfrobust.h, wfgrad.h,
            # wfcredit.h, wflookahead.h, wfpolicy.h, wfplan.h, wfretgrad.h, wfrollout.h, wfrollscen.h, wfcalib.h — the rollout and the scenario-rollout
            # object, created on the rose object, before it; the policy-search object before the policy and polscen objects)
            for name in ("_probe_points", "_probe_plane", "_yawopt_obj", "_rollout_obj", "_rollscen_obj", "_rose_obj", "_robust_obj", "_grad_obj", "_credit_obj",
                         "_lookahead_obj", "_polsearch_obj", "_policy_obj", "_polscen_obj", "_scenario_obj", "_plan_obj", "_scenplan_obj", "_retgrad_obj", "_calib_obj", "_windgen_obj"):
                ext = getattr(self, name, None)
                if ext is not None:
                    ext.close()
                    setattr(self, name, None)
            self._windgen = None
            self._lib.wf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Ext:
    """An extension object of a WfStep handle — the `wf_<NAME>` of include/wf<NAME>.h — and what the wrappers share:
    create / close, timing, kernel_info, evaluator, and the conversion of farm lists, (n, N) float32 rows and output dicts
    into the pointers the C ABI takes.  `_r` is the raw object, `KERNELS` names kernel_info's entries in the library's order."""

    NAME = ""
    KERNELS = ()

    def __init__(self, owner: WfStep):
        self._w, self._lib = owner, owner._lib
        self._r = C.c_void_p()
        check(self._fn("create")(owner._h, C.byref(self._r)), owner._h)

    def _fn(self, name):
        return getattr(self._lib, f"wf_{self.NAME}_{name}")

    def _call(self, name, *args):
        """wf_<NAME>_<name>(object, *args); a failure raises with the text of wf_<NAME>_last_error."""
        _lib.check_ext(self._fn(name)(self._r, *args), self._r, f"wf_{self.NAME}_last_error")

    def _series_mode(self, ahead):
        """The series-ahead mode of a row extension (include/wfseries.h), and whose series it reads: the generator's while a
        generated episode is active (include/wfwindgen.h), else the handle's own."""
        self._call("set_series", int(bool(ahead)))
        gen = self._w._windgen if ahead else None
        self._call("set_wind_source", None if gen is None else gen._r)

    def timing(self, detail=None):
        if detail is not None:
            self._call("set_timing", int(bool(detail)))
            return None
        t = [C.c_float(), C.c_float(), C.c_float()]
        self._call("last_timing", *[C.byref(v) for v in t])
        return {"total_ms": float(t[0].value), "step_ms": float(t[1].value), "glue_ms": float(t[2].value)}

    def kernel_info(self) -> dict:
        v = (C.c_int * (3 * len(self.KERNELS)))()
        self._call("kernel_info", v)
        keys = ("vgprs", "lds_bytes", "scratch_bytes")
        return {n: dict(zip(keys, v[3 * i:3 * i + 3])) for i, n in enumerate(self.KERNELS)}

    def evaluator(self):
        """The evaluator's raw handle (None before the first run; of a robust object: the search's): tools/yawopt_timing.py,
        robust_timing.py and grad_timing.py time a plain wf_step loop on it."""
        return self._fn("evaluator")(self._r)

    def close(self):
        if self._r is not None:
            self._fn("destroy")(self._r)
            self._r = None

    def _farms(self, farms):
        """(the int32 array kept alive, the number of farms served, the list's pointer or None) of a `farms` argument."""
        fa = None if farms is None else np.ascontiguousarray(farms, dtype=np.int32).reshape(-1)
        return fa, (self._w.env_batch if fa is None else int(fa.size)), (None if fa is None else fa.ctypes.data)

    def _rows(self, a, n, on_device, name, per="listed"):
        """(the array kept alive, its pointer) of an (n, N) float32 input, or (None, None)."""
        N = self._w.num_turbines
        if a is None:
            return None, None
        if on_device:
            import torch

            assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (n, N), name
            a = a.contiguous()
            return a, a.data_ptr()
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != (n, N):
            raise ValueError(f"{name} must be (n_farms, num_turbines): a row per {per} farm")
        return a, a.ctypes.data

    @staticmethod
    def _members_tail_bounds(members, tail, bounds):
        """(M, the tail q — all M members when `tail` is None —, ws_lo, ws_hi) of a wind ensemble's arguments."""
        M = int(members)
        q = M if tail is None else int(tail)
        ws_lo, ws_hi = (float(v) for v in bounds)
        return M, q, ws_lo, ws_hi

    @staticmethod
    def _f64(a, shape, name, what, on_device, like):
        """(the array kept alive, its pointer) of a float64 input of `shape`, or (None, None): a torch CUDA tensor (made on
        the device of `like` from anything else) on the device path, a NumPy array else.  `what` ends the refusal of a shape."""
        if a is None:
            return None, None
        if on_device:
            import torch

            if not _is_torch(a):
                a = torch.as_tensor(np.asarray(a, np.float64), device=like.device)
            assert a.is_cuda and a.dtype == torch.float64, name
            a = a.contiguous()
        else:
            a = np.ascontiguousarray(a, dtype=np.float64)
        if tuple(a.shape) != shape:
            raise ValueError(f"{name} must be {what}")
        return a, (a.data_ptr() if on_device else a.ctypes.data)

    def _anchor(self, anchor, n, on_device, like):
        """... of the (n, 2) anchor of a wind ensemble."""
        return self._f64(anchor, (n, 2), "anchor", "(n_farms, 2): the (speed, direction) every listed farm's paths revert to", on_device, like)

    @staticmethod
    def _outputs(out, spec, on_device, like=None):
        """The outputs `spec` = {name: (shape, NumPy dtype)} names, and their pointers in spec's order: `out` checked against
        it, or allocated when None — torch CUDA tensors (on the device of `like`) on the device path, NumPy arrays else."""
        if on_device:
            import torch

            kinds = {k: getattr(torch, np.dtype(d).name) for k, (_, d) in spec.items()}
            if out is None:
                out = {k: torch.empty(s, device=like.device, dtype=kinds[k]) for k, (s, _) in spec.items()}
            for k, (s, _) in spec.items():
                assert out[k].is_cuda and out[k].dtype == kinds[k] and out[k].is_contiguous() and tuple(out[k].shape) == s, k
            return out, [out[k].data_ptr() for k in spec]
        if out is None:
            out = {k: np.empty(s, d) for k, (s, d) in spec.items()}
        for k, (s, d) in spec.items():
            assert out[k].dtype == d and out[k].flags.c_contiguous and out[k].shape == s, k
        return out, [out[k].ctypes.data for k in spec]


class _WindGen(_Ext):
    """The `wf_windgen` object of a WfStep handle (include/wfwindgen.h)."""

    NAME = "windgen"
    KERNELS = ("generate", "generate_tiled")

    def call(self, name, *args):
        self._call(name, *args)

    def state(self) -> dict:
        T, t, pending, seed = C.c_int(), C.c_int(), C.c_int(), C.c_ulonglong()
        d, p = WindDist(), WindProcess()
        self._call("get", C.byref(T), C.byref(t), C.byref(pending), C.byref(seed), C.byref(d), C.byref(p))
        return {"T": int(T.value), "t": int(t.value), "prev_pending": bool(pending.value), "seed": int(seed.value),
                "dist": {n: float(getattr(d, n)) for n, _ in WindDist._fields_},
                "process": {n: float(getattr(p, n)) for n, _ in WindProcess._fields_}}


class _Probe(_Ext):
    """One `wf_probe` object of a WfStep handle (include/wfprobe.h): its points and the two calls on them."""

    NAME = "probe"
    KERNELS = ("state", "sample")

    def __init__(self, owner: WfStep):
        super().__init__(owner)
        self.n_points = 0
        self._host_points = None  # the NumPy points this probe holds (a copy), or None: none yet, or a device tensor's

    def holds(self, points, per_farm: bool) -> bool:
        """True when `points` is a NumPy array equal to the one this probe was last given: setting it again would change nothing."""
        last = self._host_points
        return (last is not None and not _is_torch(points) and last.ndim == (3 if per_farm else 2)
                and last.shape == np.shape(points) and np.array_equal(last, points))

    def set_points(self, points, per_farm: bool):
        B = self._w.env_batch
        on_device = _is_torch(points)
        self._host_points = None
        if on_device:
            pts = points.contiguous()
            assert pts.is_cuda and str(pts.dtype) == "torch.float64"
        else:
            pts = np.ascontiguousarray(points, dtype=np.float64)
        shape = tuple(pts.shape)
        if len(shape) != (3 if per_farm else 2) or shape[-1] != 3 or (per_farm and shape[0] != B):
            raise ValueError("probe points must be (P, 3), or (env_batch, P, 3) with per_farm=True")
        if on_device:
            self._w._follow_torch_stream()
        ptr = pts.data_ptr() if on_device else pts.ctypes.data
        self._call("set_points", shape[-2], ptr, B if per_farm else 1, int(on_device))
        self.n_points = int(shape[-2])
        self._host_points = None if on_device else pts.copy()

    def sample(self, yaw, farms, out):
        w = self._w
        B, N, P = w.env_batch, w.num_turbines, self.n_points
        fa, n_farms, fptr = self._farms(farms)
        shape = (n_farms, P, 3)
        if _is_torch(yaw) or _is_torch(out):
            import torch

            w._follow_torch_stream()
            yptr = None
            if yaw is not None:
                assert yaw.is_cuda and yaw.dtype == torch.float32 and yaw.numel() == B * N
                yaw = yaw.contiguous()
                yptr = yaw.data_ptr()
            if out is None:
                out = torch.empty(shape, device=yaw.device, dtype=torch.float32)
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and (P == 0 or tuple(out.shape) == shape)
            self._call("sample", yptr, n_farms, fptr, out.data_ptr(), 1)
            return out
        yptr = None
        if yaw is not None:
            yaw = np.ascontiguousarray(yaw, dtype=np.float32).reshape(B, N)
            yptr = yaw.ctypes.data
        if out is None:
            out = np.empty(shape, np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and (P == 0 or out.shape == shape)
        self._call("sample", yptr, n_farms, fptr, out.ctypes.data, 0)
        return out

    def timing(self) -> dict:
        a, b = C.c_float(), C.c_float()
        self._call("last_timing", C.byref(a), C.byref(b))
        return {"state_ms": float(a.value), "sample_ms": float(b.value)}


def _passes(passes):
    return (C.c_int * max(len(passes), 1))(*[int(k) for k in passes])


class _YawOpt(_Ext):
    """The `wf_yawopt` object of a WfStep handle (include/wfyawopt.h)."""

    NAME = "yawopt"

    def run(self, yaw0, farms, bounds, passes, strict, max_eval_farms, out):
        w = self._w
        N = w.num_turbines
        self._call("config", float(bounds[0]), float(bounds[1]), len(passes), _passes(passes), int(bool(strict)), int(max_eval_farms))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(yaw0) or (out is not None and _is_torch(out["yaw"]))
        if on_device:
            w._follow_torch_stream()
        yaw0, yptr = self._rows(yaw0, n, on_device, "yaw0", per="optimised")
        out, ptrs = self._outputs(out, {"yaw": ((n, N), np.float32), "power": ((n,), np.float32), "power_initial": ((n,), np.float32)},
                                  on_device, yaw0)
        self._call("run", yptr, n, fptr, *ptrs, int(on_device))
        return out


class _Rose(_Ext):
    """The `wf_rose` object of a WfStep handle (include/wfrose.h)."""

    NAME = "rose"
    KERNELS = ("layout", "rowsum", "accumulate", "policy")
    INTERP = {"linear": 0, "nearest": 1}

    def set_table(self, table, wd_axis, ws_axis, interp, slot):
        if interp not in self.INTERP:
            raise ValueError("interp must be 'linear' or 'nearest'")
        N = self._w.num_turbines
        if _is_torch(table):
            tb, twd, tws = table.contiguous(), wd_axis.contiguous().reshape(-1), ws_axis.contiguous().reshape(-1)
            assert tb.is_cuda and str(tb.dtype) == "torch.float32" and twd.is_cuda and tws.is_cuda
            assert str(twd.dtype) == "torch.float64" and str(tws.dtype) == "torch.float64"
            Dt, St = int(twd.numel()), int(tws.numel())
            ptrs, on_device = (twd.data_ptr(), tws.data_ptr(), tb.data_ptr()), 1
            self._w._follow_torch_stream()
        else:
            tb = np.ascontiguousarray(table, dtype=np.float32)
            twd = np.ascontiguousarray(np.atleast_1d(wd_axis), dtype=np.float64).reshape(-1)
            tws = np.ascontiguousarray(np.atleast_1d(ws_axis), dtype=np.float64).reshape(-1)
            Dt, St = int(twd.size), int(tws.size)
            ptrs, on_device = (twd.ctypes.data, tws.ctypes.data, tb.ctypes.data), 0
        if tuple(tb.shape) != (Dt, St, N):
            raise ValueError("a yaw table must be (len(wd_axis), len(ws_axis), num_turbines)")
        self._call("set_table", int(slot), Dt, ptrs[0], St, ptrs[1], ptrs[2], self.INTERP[interp], on_device)

    def _cases(self, cases):
        N = self._w.num_turbines
        kind, arg, fixed = [], [], []
        for c in cases:
            if isinstance(c, str):
                if c != "zero":
                    raise ValueError('a case is "zero", an (N,) yaw array or ("table", slot)')
                kind.append(0); arg.append(0)
            elif isinstance(c, tuple) and len(c) == 2 and c[0] == "table":
                kind.append(2); arg.append(int(c[1]))
            else:
                row = np.asarray(c.detach().cpu() if _is_torch(c) else c, dtype=np.float32).reshape(-1)
                if row.shape != (N,):
                    raise ValueError('a case is "zero", an (N,) yaw array or ("table", slot)')
                kind.append(1); arg.append(len(fixed)); fixed.append(row)
        if not kind:
            raise ValueError("expected_power needs at least one case")
        fx = np.ascontiguousarray(np.stack(fixed)) if fixed else None
        return np.asarray(kind, np.int32), np.asarray(arg, np.int32), fx

    def evaluate(self, wd, ws, freq, cases, cut_in, cut_out, strict, max_eval_farms, out):
        w = self._w
        N = w.num_turbines
        wd = np.ascontiguousarray(np.atleast_1d(wd), dtype=np.float64)
        ws = np.ascontiguousarray(np.atleast_1d(ws), dtype=np.float64)
        freq = np.ascontiguousarray(freq, dtype=np.float64)
        if wd.ndim != 1 or ws.ndim != 1 or freq.shape != (wd.size, ws.size):
            raise ValueError("freq must be (len(wd), len(ws))")
        D, S = wd.size, ws.size
        kind, arg, fixed = self._cases(cases)
        Cn = kind.size
        self._call("set_rose", D, wd.ctypes.data, S, ws.ctypes.data, freq.ctypes.data, float(cut_in), 0.0 if cut_out is None else float(cut_out))
        self._call("config", int(bool(strict)), int(max_eval_farms))
        fsum = float(np.sum(freq))
        on_device = out is not None
        fptr = None if fixed is None else fixed.ctypes.data
        if on_device:
            import torch

            w._follow_torch_stream()
        out, ptrs = self._outputs(out, {"weighted_power": ((Cn,), np.float64), "weighted_turbine_power": ((Cn, N), np.float64),
                                        "condition_power": ((Cn, D, S), np.float32)}, on_device)
        if on_device and fixed is not None:
            fixed = torch.as_tensor(fixed, device=out["condition_power"].device)
            fptr = fixed.data_ptr()
        self._call("evaluate", Cn, kind.ctypes.data, arg.ctypes.data, fptr, *ptrs, int(on_device))
        wp, wtp = out["weighted_power"], out["weighted_turbine_power"]
        return {"expected_power": wp / fsum, "aep_gwh": wp * (8760.0 / 1.0e9), "turbine_expected_power": wtp / fsum,
                "condition_power": out["condition_power"], "freq_sum": fsum, "weighted_power": wp, "weighted_turbine_power": wtp}

    def policy(self, slot, want, as_torch):
        w = self._w
        B, N = w.env_batch, w.num_turbines
        keys = [k for k in ("target_yaw", "action") if k in want]
        if not keys:
            raise ValueError("want must name target_yaw and / or action")
        if as_torch:
            import torch

            w._follow_torch_stream()
            out = {k: torch.empty((B, N), dtype=torch.float32, device=f"cuda:{w.device_id}") for k in keys}
            ptr = {k: v.data_ptr() for k, v in out.items()}
        else:
            out = {k: np.empty((B, N), np.float32) for k in keys}
            ptr = {k: v.ctypes.data for k, v in out.items()}
        self._call("policy", int(slot), ptr.get("target_yaw"), ptr.get("action"), int(bool(as_torch)))
        return out


class _Robust(_Ext):
    """The `wf_robust` object of a WfStep handle (include/wfrobust.h)."""

    NAME = "robust"
    KERNELS = ("order", "layout", "rowsum", "advance", "expect")
    FRAME = {"relative": 0, "fixed": 1}

    def _set_members(self, spec):
        delta, weight, frame = wd_uncertainty_members(spec)
        self._call("set_members", int(delta.size), delta.ctypes.data, weight.ctypes.data, self.FRAME[frame])
        s = 0.0
        for v in weight:  # (the library's normalisation: the sum in index order)
            s = s + float(v)
        return delta, weight / s

    def _config(self, bounds, passes, strict, max_eval_farms):
        self._call("config", float(bounds[0]), float(bounds[1]), len(passes), _passes(passes), int(bool(strict)), int(max_eval_farms))

    def evaluate(self, yaw, farms, strict, max_eval_farms, out, spec):
        w = self._w
        N = w.num_turbines
        delta, wn = self._set_members(spec)
        self._config((-25.0, 25.0), (5, 4), strict, max_eval_farms)  # (bounds and passes play no part in an evaluation)
        fa, n, fptr = self._farms(farms)
        shapes = {"expected_power": ((n,), np.float64), "turbine_expected_power": ((n, N), np.float64),
                  "member_power": ((n, delta.size), np.float32)}
        on_device = _is_torch(yaw) or (out is not None and _is_torch(out["expected_power"]))
        if on_device:
            w._follow_torch_stream()
        yaw, yptr = self._rows(yaw, n, on_device, "yaw")
        out, ptrs = self._outputs(out, shapes, on_device, yaw)
        self._call("evaluate", yptr, n, fptr, *ptrs, int(on_device))
        return {**{k: out[k] for k in shapes}, "delta": delta, "weight": wn}

    def optimize(self, yaw0, farms, bounds, passes, strict, max_eval_farms, out, spec):
        w = self._w
        N = w.num_turbines
        self._set_members(spec)
        self._config(bounds, passes, strict, max_eval_farms)
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(yaw0) or (out is not None and _is_torch(out["yaw"]))
        if on_device:
            w._follow_torch_stream()
        yaw0, yptr = self._rows(yaw0, n, on_device, "yaw")
        out, ptrs = self._outputs(out, {"yaw": ((n, N), np.float32), "power": ((n,), np.float32), "power_initial": ((n,), np.float32)},
                                  on_device, yaw0)
        self._call("optimize", yptr, n, fptr, *ptrs, int(on_device))
        return out


class _Grad(_Ext):
    """The `wf_grad` object of a WfStep handle (include/wfgrad.h)."""

    NAME = "grad"
    KERNELS = ("layout", "reduce")

    def _config(self, step, bounds, strict, max_eval_farms):
        self._call("config", float(step), float(bounds[0]), float(bounds[1]), int(bool(strict)), int(max_eval_farms))

    def run(self, yaw, cotangent, farms, step, bounds, strict, max_eval_farms, jacobian, out):
        w = self._w
        N = w.num_turbines
        self._config(step, bounds, strict, max_eval_farms)
        fa, n, fptr = self._farms(farms)
        shapes = {"power": ((n, N), np.float32), "gradient": ((n, N), np.float64)}
        if jacobian:
            shapes["jacobian"] = ((n, N, N), np.float64)
        on_device = _is_torch(yaw) or _is_torch(cotangent) or (out is not None and _is_torch(out["gradient"]))
        if on_device:
            w._follow_torch_stream()
        yaw, yptr = self._rows(yaw, n, on_device, "yaw")
        cotangent, cptr = self._rows(cotangent, n, on_device, "cotangent")
        out, ptrs = self._outputs(out, shapes, on_device, yaw if yaw is not None else cotangent)
        self._call("run", yptr, cptr, n, fptr, ptrs[0], ptrs[1], ptrs[2] if jacobian else None, int(on_device))
        return {k: out[k] for k in shapes}

    def backward(self, yaw, cotangent, step, bounds, strict):
        """The vector-Jacobian product alone, device pointers in and out (autograd.differentiable_power): (B, N) float64."""
        import torch

        w = self._w
        B, N = w.env_batch, w.num_turbines
        self._config(step, bounds, strict, 0)
        w._follow_torch_stream()
        yaw, yptr = self._rows(yaw, B, True, "yaw")
        cotangent, cptr = self._rows(cotangent, B, True, "cotangent")
        grad = torch.empty((B, N), device=yaw.device, dtype=torch.float64)
        self._call("run", yptr, cptr, B, None, None, grad.data_ptr(), None, 1)
        return grad


class _Credit(_Ext):
    """The `wf_credit` object of a WfStep handle (include/wfcredit.h)."""

    NAME = "credit"
    KERNELS = ("layout", "reduce")
    KIND = {"yaw": 0, "action": 1}
    OUTPUTS = ("reward", "farm_power", "difference")

    def run(self, base, alt, base_kind, alt_kind, farms, strict, max_eval_farms, want, out, wind=None):
        w = self._w
        N = w.num_turbines
        if wind is not None and not _is_series(wind):
            raise ValueError('wind must be None (the current wind) or "series" (the series\' coming row)')
        self._series_mode(wind is not None)
        if base_kind not in self.KIND or alt_kind not in self.KIND:
            raise ValueError("base_kind and alt_kind must be 'yaw' or 'action'")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name reward, farm_power and / or difference")
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(base) or _is_torch(alt) or (out is not None and any(_is_torch(v) for v in out.values()))
        if on_device:
            w._follow_torch_stream()
        base, bptr = self._rows(base, n, on_device, "base")
        K, aptr = 1, None
        if alt is not None:
            if not on_device:
                alt = np.ascontiguousarray(alt, dtype=np.float32)
            shape = tuple(alt.shape)
            if len(shape) == 2:
                shape += (1,)
            if len(shape) != 3 or shape[:2] != (n, N):
                raise ValueError("alt must be (n_farms, num_turbines, K): K alternatives per turbine of every listed farm")
            K = int(shape[2])
            if on_device:
                import torch

                assert alt.is_cuda and alt.dtype == torch.float32, "alt"
                alt = alt.contiguous()
                aptr = alt.data_ptr()
            else:
                aptr = alt.ctypes.data
        R = 1 + N * K
        shapes = {"reward": ((n, R), np.float64), "farm_power": ((n, R), np.float64), "difference": ((n, N, K), np.float64)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        like = base if base is not None else alt
        if on_device and like is None:
            like = next(v for v in out.values() if _is_torch(v))
        out, ptrs = self._outputs(out, spec, on_device, like)
        p = dict(zip(spec, ptrs))
        self._call("run", self.KIND[base_kind], bptr, self.KIND[alt_kind], aptr, K, n, fptr, p.get("reward"), p.get("farm_power"),
                   p.get("difference"), int(on_device))
        return {k: out[k] for k in spec}


class _Lookahead(_Ext):
    """The `wf_lookahead` object of a WfStep handle (include/wflookahead.h)."""

    NAME = "lookahead"
    KERNELS = ("layout", "reduce")
    OUTPUTS = ("returns", "rewards", "farm_power", "final_yaw", "best")

    def run(self, actions, gamma, wind, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name returns, rewards, farm_power, final_yaw and / or best")
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(actions)
        if on_device:
            import torch

            w._follow_torch_stream()
            assert actions.is_cuda and actions.dtype == torch.float32, "actions"
            actions = actions.contiguous()
        else:
            actions = np.ascontiguousarray(actions, dtype=np.float32)
        shape = tuple(actions.shape)
        if len(shape) != 4 or shape[0] != n or shape[3] != N:
            raise ValueError("actions must be (n_farms, K, H, num_turbines): K sequences of H joint actions per listed farm")
        K, H = int(shape[1]), int(shape[2])
        wptr = None
        self._series_mode(_is_series(wind))
        if _is_series(wind):
            wind = None
        if wind is not None:
            if on_device:
                if not _is_torch(wind):
                    wind = torch.as_tensor(np.asarray(wind, np.float64), device=actions.device)
                assert wind.is_cuda and wind.dtype == torch.float64, "wind"
                wind = wind.contiguous()
            else:
                wind = np.ascontiguousarray(wind, dtype=np.float64)
            if tuple(wind.shape) != (n, H, 2):
                raise ValueError("wind must be (n_farms, H, 2): the (speed, direction) every step of the horizon is solved under")
            wptr = wind.data_ptr() if on_device else wind.ctypes.data
        shapes = {"returns": ((n, K), np.float64), "rewards": ((n, K, H), np.float64), "farm_power": ((n, K, H), np.float64),
                  "final_yaw": ((n, K, N), np.float32), "best": ((n,), np.int32)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec, on_device, actions)
        p = dict(zip(spec, ptrs))
        self._call("run", actions.data_ptr() if on_device else actions.ctypes.data, K, H, wptr, float(gamma), n, fptr,
                   *[p.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _Policy(_Ext):
    """The `wf_policy` object of a WfStep handle (include/wfpolicy.h)."""

    NAME = "policy"
    KERNELS = ("transpose", "begin", "advance", "reduce")
    OUTPUTS = ("returns", "rewards", "farm_power", "actions", "observations", "final_yaw", "gated", "best")

    def _set_network(self, spec):
        from . import policy as P

        if not isinstance(spec, dict) or any(k not in spec for k in ("kind", "widths", "activation", "final", "out_scale", "shift", "scale")):
            raise ValueError("spec must be what policy.mlp_spec returns")
        if spec["kind"] not in P.KINDS or spec["activation"] not in P.ACTIVATIONS or spec["final"] not in P.FINALS:
            raise ValueError("spec names an unknown kind or activation (policy.mlp_spec)")
        widths = np.ascontiguousarray(spec["widths"], dtype=np.int32)
        shift = np.ascontiguousarray(spec["shift"], dtype=np.float64)
        scale = np.ascontiguousarray(spec["scale"], dtype=np.float64)
        if shift.shape != (int(widths[0]),) or scale.shape != (int(widths[0]),):
            raise ValueError("spec: shift and scale must hold one value per input")
        self._call("set_network", P.KINDS[spec["kind"]], int(widths.size) - 1, widths.ctypes.data, P.ACTIVATIONS[spec["activation"]],
                   P.FINALS[spec["final"]], int(bool(spec.get("use_freewind", False))), float(spec["out_scale"]),
                   shift.ctypes.data, scale.ctypes.data)

    def run(self, params, spec, horizon, gamma, wind, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name returns, rewards, farm_power, actions, observations, final_yaw, gated and / or best")
        self._set_network(spec)
        H = int(horizon)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(params) or _is_torch(wind) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            import torch

            w._follow_torch_stream()
            like = next(v for v in [params, wind] + list((out or {}).values()) if _is_torch(v))
            if not _is_torch(params):
                params = torch.as_tensor(np.array(params, np.float32), device=like.device)
            assert params.is_cuda and params.dtype == torch.float32, "params"
            params = params.contiguous()
        else:
            params = np.ascontiguousarray(params, dtype=np.float32)
        if len(tuple(params.shape)) == 1:
            params = params.reshape(1, -1)
        if len(tuple(params.shape)) != 2:
            raise ValueError("params must be (K, P): a parameter vector per policy")
        K, P = int(params.shape[0]), int(params.shape[1])
        wptr = None
        if wind is not None:
            if on_device:
                if not _is_torch(wind):
                    wind = torch.as_tensor(np.array(wind, np.float64), device=like.device)
                assert wind.is_cuda and wind.dtype == torch.float64, "wind"
                wind = wind.contiguous()
            else:
                wind = np.ascontiguousarray(wind, dtype=np.float64)
            if tuple(wind.shape) != (n, H, 2):
                raise ValueError("wind must be (n_farms, H, 2): the (speed, direction) every step of the horizon is solved under")
            wptr = wind.data_ptr() if on_device else wind.ctypes.data
        shapes = {"returns": ((n, K), np.float64), "rewards": ((n, K, H), np.float64), "farm_power": ((n, K, H), np.float64),
                  "actions": ((n, K, H, N), np.float32), "observations": ((n, K, H, 3 * N + 2), np.float32),
                  "final_yaw": ((n, K, N), np.float32), "gated": ((n, K), np.int32), "best": ((n,), np.int32)}
        if not (1 <= H <= 256 and 1 <= K <= 64):  # (the library names the limit; no output is sized from a refused shape)
            shapes = {k: ((0,), d) for k, (_, d) in shapes.items()}
            out = None
        spec_out = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec_out, on_device, like)
        p = dict(zip(spec_out, ptrs))
        self._call("run", params.data_ptr() if on_device else params.ctypes.data, K, P, H, wptr, float(gamma), n, fptr,
                   *[p.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec_out}


class _PolScen(_Policy):
    """The `wf_polscen` object of a WfStep handle (include/wfpolscen.h); the network is taken as the policy object takes it."""

    NAME = "polscen"
    KERNELS = ("paths", "returns", "stats", "transpose", "begin", "advance")
    OUTPUTS = ("expected_returns", "cvar", "score", "member_returns", "rewards", "farm_power", "wind_paths", "actions",
               "observations", "final_yaw", "gated", "first_action", "best")

    def run(self, params, spec, horizon, members, process, seed, gamma, tail, risk_weight, anchor, bounds, farms, strict,
            max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name " + ", ".join(self.OUTPUTS[:-1]) + " and / or " + self.OUTPUTS[-1])
        p = _wind_process(process, "policy_scenarios")
        self._set_network(spec)
        H = int(horizon)
        M, q, ws_lo, ws_hi = self._members_tail_bounds(members, tail, bounds)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(params) or _is_torch(anchor) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            import torch

            w._follow_torch_stream()
            like = next(v for v in [params, anchor] + list((out or {}).values()) if _is_torch(v))
            if not _is_torch(params):
                params = torch.as_tensor(np.array(params, np.float32), device=like.device)
            assert params.is_cuda and params.dtype == torch.float32, "params"
            params = params.contiguous()
        else:
            params = np.ascontiguousarray(params, dtype=np.float32)
        if len(tuple(params.shape)) == 1:
            params = params.reshape(1, -1)
        if len(tuple(params.shape)) != 2:
            raise ValueError("params must be (K, P): a parameter vector per policy")
        K, P = int(params.shape[0]), int(params.shape[1])
        anchor, aptr = self._anchor(anchor, n, on_device, like)
        f8, f4, i4 = np.float64, np.float32, np.int32
        shapes = {"expected_returns": ((n, K), f8), "cvar": ((n, K), f8), "score": ((n, K), f8), "member_returns": ((n, K, M), f8),
                  "rewards": ((n, K, M, H), f8), "farm_power": ((n, K, M, H), f8), "wind_paths": ((n, M, H, 2), f8),
                  "actions": ((n, K, M, H, N), f4), "observations": ((n, K, M, H, 3 * N + 2), f4), "final_yaw": ((n, K, M, N), f4),
                  "gated": ((n, K, M), i4), "first_action": ((n, K, N), f4), "best": ((n,), i4)}
        if not (1 <= K <= 64 and 1 <= M <= 64 and 1 <= H <= 64):  # (the library names the limit; no output is sized from a refused shape)
            shapes = {k: ((0,), d) for k, (_, d) in shapes.items()}
            out = None
        spec_out = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec_out, on_device, like)
        ptr = dict(zip(spec_out, ptrs))
        self._call("run", params.data_ptr() if on_device else params.ctypes.data, K, P, H, M, C.byref(p), ws_lo, ws_hi,
                   C.c_ulonglong(int(seed) & (2**64 - 1)), float(gamma), q, float(risk_weight), aptr, n, fptr,
                   *[ptr.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec_out}


class _PolSearch(_Ext):
    """The `wf_polsearch` object of a WfStep handle (include/wfpolsearch.h), created on the handle's policy and polscen objects:
    it owns no evaluator, the rollouts run on theirs."""

    NAME = "polsearch"
    KERNELS = ("tiles", "advance")
    OUTPUTS = ("best_params", "best_fitness", "init_fitness", "mean", "sigma", "fitness", "winner", "candidates", "sigma_history",
               "farm_scores")

    def __init__(self, owner: WfStep):
        self._w, self._lib = owner, owner._lib
        self._r = C.c_void_p()
        check(self._fn("create")(owner._h, owner._policy()._r, owner._polscen()._r, C.byref(self._r)), owner._h)

    def _vector(self, a, on_device, like, name):
        """(the float32 vector kept alive, its pointer): a torch CUDA tensor on the device path, a NumPy array else."""
        if on_device:
            import torch

            if not _is_torch(a):
                a = torch.as_tensor(np.array(a, np.float32), device=like.device)
            assert a.is_cuda and a.dtype == torch.float32, name
            a = a.contiguous().reshape(-1)
            return a, a.data_ptr()
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        return a, a.ctypes.data

    def run(self, mean, spec, horizon, sigma, candidates, elites, iterations, sigma_min, seed, gamma, wind, members, process,
            scenario_seed, tail, risk_weight, anchor, bounds, farms, strict, max_eval_farms, want, out):
        w = self._w
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name " + ", ".join(self.OUTPUTS[:-1]) + " and / or " + self.OUTPUTS[-1])
        H, K, E, I = int(horizon), int(candidates), int(elites), int(iterations)
        M, q, ws_lo, ws_hi = 0, 0, 0.0, 0.0
        proc = None
        # network, strict and max_eval_farms are the scorer's settings: the scorer object takes them as its own wrapper does
        scorer = w._policy()
        if members is not None:
            scorer = w._polscen()
            proc = _wind_process(process, "search_policy")
            M, q, ws_lo, ws_hi = self._members_tail_bounds(members, tail, bounds)
            if M < 1:
                raise ValueError("members must be >= 1 (None: policy_returns scores, under the wind held or a wind per step)")
            if wind is not None:
                raise ValueError("wind and members exclude each other: the members' paths are the wind")
        scorer._set_network(spec)
        scorer._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        ins = [mean, sigma, wind, anchor] + list((out or {}).values())
        on_device = any(_is_torch(v) for v in ins)
        like = next((v for v in ins if _is_torch(v)), None)
        if on_device:
            w._follow_torch_stream()
        mean, mptr = self._vector(mean, on_device, like, "mean")
        P = int(mean.shape[0])
        if not _is_torch(sigma) and np.ndim(sigma) == 0:
            sigma = np.full(P, float(sigma), np.float32)
        sigma, sptr = self._vector(sigma, on_device, like, "sigma")
        if int(sigma.shape[0]) != P:
            raise ValueError("sigma must be a scalar or (P,): a width per weight")
        wind, wptr = self._f64(wind, (n, H, 2), "wind", "(n_farms, H, 2): the (speed, direction) every step of the horizon is solved under",
                               on_device, like)
        aptr = None
        if members is not None:
            anchor, aptr = self._anchor(anchor, n, on_device, like)
        f8, f4, i4 = np.float64, np.float32, np.int32
        shapes = {"best_params": ((P,), f4), "best_fitness": ((), f8), "init_fitness": ((), f8), "mean": ((P,), f4), "sigma": ((P,), f4),
                  "fitness": ((I, K), f8), "winner": ((I,), i4), "candidates": ((I, K, P), f4), "sigma_history": ((I, P), f4),
                  "farm_scores": ((I, n, K), f8)}
        if not (3 <= K <= 64 and 1 <= I <= 16):  # (the library names the limit; no output is sized from a refused shape)
            shapes = {k: ((0,), d) for k, (_, d) in shapes.items()}
            out = None
        spec_out = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec_out, on_device, like)
        ptr = dict(zip(spec_out, ptrs))
        self._call("run", mptr, sptr, P, K, E, I, float(sigma_min), C.c_ulonglong(int(seed) & (2**64 - 1)), H, float(gamma), wptr, M,
                   None if proc is None else C.byref(proc), ws_lo, ws_hi, C.c_ulonglong(int(scenario_seed) & (2**64 - 1)), q,
                   float(risk_weight), aptr, n, fptr, *[ptr.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec_out}


class _Scenario(_Ext):
    """The `wf_scenario` object of a WfStep handle (include/wfscenario.h)."""

    NAME = "scenario"
    KERNELS = ("layout", "reduce")
    OUTPUTS = ("expected_returns", "cvar", "score", "member_returns", "rewards", "wind_paths", "final_yaw", "best")

    def run(self, actions, members, process, seed, gamma, tail, risk_weight, anchor, bounds, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name expected_returns, cvar, score, member_returns, rewards, wind_paths, final_yaw and / or best")
        p = _wind_process(process, "scenario_returns")
        M, q, ws_lo, ws_hi = self._members_tail_bounds(members, tail, bounds)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(actions)
        if on_device:
            import torch

            w._follow_torch_stream()
            assert actions.is_cuda and actions.dtype == torch.float32, "actions"
            actions = actions.contiguous()
        else:
            actions = np.ascontiguousarray(actions, dtype=np.float32)
        shape = tuple(actions.shape)
        if len(shape) != 4 or shape[0] != n or shape[3] != N:
            raise ValueError("actions must be (n_farms, K, H, num_turbines): K sequences of H joint actions per listed farm")
        K, H = int(shape[1]), int(shape[2])
        anchor, aptr = self._anchor(anchor, n, on_device, actions)
        shapes = {"expected_returns": ((n, K), np.float64), "cvar": ((n, K), np.float64), "score": ((n, K), np.float64),
                  "member_returns": ((n, K, M), np.float64), "rewards": ((n, K, M, H), np.float64),
                  "wind_paths": ((n, M, H, 2), np.float64), "final_yaw": ((n, K, N), np.float32), "best": ((n,), np.int32)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        if out is None and not (1 <= M <= 64 and 1 <= H <= 64 and K * M * H <= 4096):
            spec = {k: ((0,), d) for k, (_, d) in spec.items()}  # (the library refuses these limits by name: nothing to allocate)
        out, ptrs = self._outputs(out, spec, on_device, actions)
        ptr = dict(zip(spec, ptrs))
        self._call("run", actions.data_ptr() if on_device else actions.ctypes.data, K, H, M, C.byref(p), ws_lo, ws_hi,
                   C.c_ulonglong(int(seed) & (2**64 - 1)), float(gamma), q, float(risk_weight), aptr, n, fptr,
                   *[ptr.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _RetGrad(_Ext):
    """The `wf_retgrad` object of a WfStep handle (include/wfretgrad.h)."""

    NAME = "retgrad"
    KERNELS = ("layout", "reduce", "best")
    OUTPUTS = ("returns", "rewards", "farm_power", "final_yaw", "best", "action_gradient", "reward_gradient", "state_gradient",
               "yaw", "pass_mask")

    def run(self, actions, gamma, wind, terminal, delta, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name " + ", ".join(self.OUTPUTS[:-1]) + " and / or " + self.OUTPUTS[-1])
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(actions)
        if on_device:
            import torch

            w._follow_torch_stream()
            assert actions.is_cuda and actions.dtype == torch.float32, "actions"
            actions = actions.contiguous()
        else:
            actions = np.ascontiguousarray(actions, dtype=np.float32)
        shape = tuple(actions.shape)
        if len(shape) != 4 or shape[0] != n or shape[3] != N:
            raise ValueError("actions must be (n_farms, K, H, num_turbines): K sequences of H joint actions per listed farm")
        K, H = int(shape[1]), int(shape[2])
        self._series_mode(_is_series(wind))
        if _is_series(wind):
            wind = None

        def f64(a, shape, name, what):
            if a is None:
                return None, None
            if on_device:
                if not _is_torch(a):
                    a = torch.as_tensor(np.asarray(a, np.float64), device=actions.device)
                assert a.is_cuda and a.dtype == torch.float64, name
                a = a.contiguous()
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
            if tuple(a.shape) != shape:
                raise ValueError(f"{name} must be {what}")
            return a, (a.data_ptr() if on_device else a.ctypes.data)

        wind, wptr = f64(wind, (n, H, 2), "wind", "(n_farms, H, 2): the (speed, direction) every step of the horizon is solved under")
        terminal, tptr = f64(terminal, (n, K, N), "terminal", "(n_farms, K, num_turbines): the terminal value's derivative w.r.t. the final yaw")
        seq = ((n, K, H, N), np.float64)
        shapes = {"returns": ((n, K), np.float64), "rewards": ((n, K, H), np.float64), "farm_power": ((n, K, H), np.float64),
                  "final_yaw": ((n, K, N), np.float32), "best": ((n,), np.int32), "action_gradient": seq, "reward_gradient": seq,
                  "state_gradient": ((n, K, N), np.float64), "yaw": ((n, K, H, N), np.float32), "pass_mask": ((n, K, H, N), np.uint8)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec, on_device, actions)
        p = dict(zip(spec, ptrs))
        self._call("run", actions.data_ptr() if on_device else actions.ctypes.data, K, H, wptr, float(gamma), float(delta), tptr,
                   n, fptr, *[p.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _Rollout(_Ext):
    """The `wf_rollout` object of a WfStep handle (include/wfrollout.h), created on the handle's rose object."""

    NAME = "rollout"
    KERNELS = ("layout", "reduce")
    OUTPUTS = ("returns", "rewards", "farm_power", "actions", "final_yaw", "gated", "filter_final", "best")
    FIELDS = {"slot": (np.int32, 0), "alpha": (np.float64, 1.0), "deadband": (np.float32, 0.0), "lead": (np.int32, 0)}

    def __init__(self, owner: WfStep):
        self._w, self._lib = owner, owner._lib
        self._r = C.c_void_p()
        check(self._fn("create")(owner._h, owner._rose()._r, C.byref(self._r)), owner._h)

    def _controllers(self, controllers):
        if not isinstance(controllers, dict) or any(k not in self.FIELDS for k in controllers):
            raise ValueError("controllers must be a dict of slot, alpha, deadband and / or lead")
        cols = {}
        for k, (dtype, default) in self.FIELDS.items():
            v = controllers.get(k, default)
            v = np.asarray(v.detach().cpu() if _is_torch(v) else v)
            if k in ("slot", "lead") and not np.array_equal(v, np.round(v)):
                raise ValueError(f"controllers[{k!r}] must hold integers")
            cols[k] = np.atleast_1d(v.astype(dtype)).reshape(-1)
        K = max(c.size for c in cols.values())
        if any(c.size not in (1, K) for c in cols.values()):
            raise ValueError("the controllers' fields must broadcast to a common length K")
        return {k: np.ascontiguousarray(np.broadcast_to(c, (K,))) for k, c in cols.items()}, K

    def run(self, controllers, horizon, gamma, wind, filter0, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name returns, rewards, farm_power, actions, final_yaw, gated, filter_final and / or best")
        ctl, K = self._controllers(controllers)
        H = int(horizon)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        self._series_mode(_is_series(wind))
        if _is_series(wind):
            wind = None
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(wind) or _is_torch(filter0) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            import torch

            w._follow_torch_stream()
            like = next(v for v in [wind, filter0] + list((out or {}).values()) if _is_torch(v))

        def f64(a, shape, name, what):
            if a is None:
                return None, None
            if on_device:
                if not _is_torch(a):
                    a = torch.as_tensor(np.asarray(a, np.float64), device=like.device)
                assert a.is_cuda and a.dtype == torch.float64, name
                a = a.contiguous()
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
            if tuple(a.shape) != shape:
                raise ValueError(f"{name} must be {what}")
            return a, (a.data_ptr() if on_device else a.ctypes.data)

        wind, wptr = f64(wind, (n, H, 2), "wind", "(n_farms, H, 2): the (speed, direction) every step of the horizon is solved under")
        filter0, f0ptr = f64(filter0, (n, K, 2), "filter0", "(n_farms, K, 2): the (speed, direction) every controller's filter starts from")
        shapes = {"returns": ((n, K), np.float64), "rewards": ((n, K, H), np.float64), "farm_power": ((n, K, H), np.float64),
                  "actions": ((n, K, H, N), np.float32), "final_yaw": ((n, K, N), np.float32), "gated": ((n, K), np.int32),
                  "filter_final": ((n, K, 2), np.float64), "best": ((n,), np.int32)}
        if H < 1 or K < 1 or K * H > 4096:  # (the library names the limit; no output is sized from a refused shape)
            shapes = {k: ((0,), d) for k, (_, d) in shapes.items()}
            out = None
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec, on_device, like)
        p = dict(zip(spec, ptrs))
        self._call("run", K, ctl["slot"].ctypes.data, ctl["alpha"].ctypes.data, ctl["deadband"].ctypes.data, ctl["lead"].ctypes.data,
                   H, wptr, f0ptr, float(gamma), n, fptr, *[p.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _RollScen(_Rollout):
    """The `wf_rollscen` object of a WfStep handle (include/wfrollscen.h), created on the handle's rose object; the
    controllers are taken as the rollout object takes them."""

    NAME = "rollscen"
    KERNELS = ("layout", "layout_spill", "reduce")
    OUTPUTS = ("expected_returns", "cvar", "score", "member_returns", "rewards", "wind_paths", "actions", "final_yaw", "gated",
               "first_action", "best")

    def run(self, controllers, horizon, members, process, seed, gamma, tail, risk_weight, anchor, bounds, filter0, farms, strict,
            max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name " + ", ".join(self.OUTPUTS[:-1]) + " and / or " + self.OUTPUTS[-1])
        p = _wind_process(process, "controller_scenarios")
        ctl, K = self._controllers(controllers)
        H = int(horizon)
        M, q, ws_lo, ws_hi = self._members_tail_bounds(members, tail, bounds)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(anchor) or _is_torch(filter0) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            w._follow_torch_stream()
            like = next(v for v in [anchor, filter0] + list((out or {}).values()) if _is_torch(v))
        anchor, aptr = self._anchor(anchor, n, on_device, like)
        filter0, f0ptr = self._f64(filter0, (n, K, 2), "filter0", "(n_farms, K, 2): the (speed, direction) every controller's filter starts from",
                                   on_device, like)
        f8, f4, i4 = np.float64, np.float32, np.int32
        shapes = {"expected_returns": ((n, K), f8), "cvar": ((n, K), f8), "score": ((n, K), f8), "member_returns": ((n, K, M), f8),
                  "rewards": ((n, K, M, H), f8), "wind_paths": ((n, M, H, 2), f8), "actions": ((n, K, M, H, N), f4),
                  "final_yaw": ((n, K, M, N), f4), "gated": ((n, K, M), i4), "first_action": ((n, K, N), f4), "best": ((n,), i4)}
        if not (1 <= K <= 64 and 1 <= M <= 64 and 1 <= H <= 64 and K * M * H <= 4096):
            shapes = {k: ((0,), d) for k, (_, d) in shapes.items()}  # (the library names the limit; no output is sized from a refused shape)
            out = None
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec, on_device, like)
        ptr = dict(zip(spec, ptrs))
        self._call("run", K, ctl["slot"].ctypes.data, ctl["alpha"].ctypes.data, ctl["deadband"].ctypes.data, ctl["lead"].ctypes.data,
                   H, M, C.byref(p), ws_lo, ws_hi, C.c_ulonglong(int(seed) & (2**64 - 1)), float(gamma), q, float(risk_weight),
                   aptr, f0ptr, n, fptr, *[ptr.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _Plan(_Ext):
    """The `wf_plan` object of a WfStep handle (include/wfplan.h)."""

    NAME = "plan"
    KERNELS = ("advance",)
    OUTPUTS = ("plan", "plan_return", "hold_return", "first_action", "final_yaw", "mean")

    def run(self, horizon, candidates, elites, sigma, seed, gamma, wind, mean, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name plan, plan_return, hold_return, first_action, final_yaw and / or mean")
        H, K, E = int(horizon), int(candidates), int(elites)
        if sigma is None:
            step = getattr(w, "_env_yaw_step", 5.0)
            sigma = (step, 0.5 * step, 0.25 * step)
        sg = np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64).reshape(-1)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        self._series_mode(_is_series(wind))
        if _is_series(wind):
            wind = None
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(wind) or _is_torch(mean) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            import torch

            w._follow_torch_stream()
            like = next(v for v in [wind, mean] + list((out or {}).values()) if _is_torch(v))
        wptr = mptr = None
        if wind is not None:
            if on_device:
                if not _is_torch(wind):
                    wind = torch.as_tensor(np.asarray(wind, np.float64), device=like.device)
                assert wind.is_cuda and wind.dtype == torch.float64, "wind"
                wind = wind.contiguous()
            else:
                wind = np.ascontiguousarray(wind, dtype=np.float64)
            if tuple(wind.shape) != (n, H, 2):
                raise ValueError("wind must be (n_farms, H, 2): the (speed, direction) every step of the horizon is solved under")
            wptr = wind.data_ptr() if on_device else wind.ctypes.data
        if mean is not None:
            if on_device:
                if not _is_torch(mean):
                    mean = torch.as_tensor(np.asarray(mean, np.float32), device=like.device)
                assert mean.is_cuda and mean.dtype == torch.float32, "mean"
                mean = mean.contiguous()
            else:
                mean = np.ascontiguousarray(mean, dtype=np.float32)
            if tuple(mean.shape) != (n, H, N):
                raise ValueError("mean must be (n_farms, H, num_turbines): the warm start of every listed farm")
            mptr = mean.data_ptr() if on_device else mean.ctypes.data
        shapes = {"plan": ((n, H, N), np.float32), "plan_return": ((n,), np.float64), "hold_return": ((n,), np.float64),
                  "first_action": ((n, N), np.float32), "final_yaw": ((n, N), np.float32), "mean": ((n, H, N), np.float32)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        out, ptrs = self._outputs(out, spec, on_device, like)
        p = dict(zip(spec, ptrs))
        self._call("run", H, K, E, int(sg.size), sg.ctypes.data, int(seed) & 0xFFFFFFFFFFFFFFFF, float(gamma), wptr, mptr, n, fptr,
                   *[p.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}


class _Calib(_Ext):
    """The `wf_calib` object of a WfStep handle (include/wfcalib.h)."""

    NAME = "calib"
    KERNELS = ("advance",)
    FIT_OUTPUTS = ("best_set", "best_loss", "init_loss", "history", "mean", "fit_power", "n_invalid")

    def _sets(self, sets, n_outer):
        """(ctypes ModelSet array, S, per_problem) of a `sets` argument: [S] shared, or [n_outer][S] a batch per problem."""
        base = self._w.model_set_from_model()
        fields = _lib._MODEL_SET_FIELDS
        per = False
        if isinstance(sets, dict):
            cols = {k: np.asarray(v, dtype=np.float64) for k, v in sets.items()}
            if any(v.ndim == 2 for v in cols.values()):
                if any(v.shape != (n_outer, next(iter(cols.values())).shape[1]) for v in cols.values()):
                    raise ValueError("model sets per problem: every field needs an array (G, S)")
                per = True
                arr, n = normalize_model_sets({k: v.reshape(-1) for k, v in cols.items()}, base)
                S = n // n_outer
            else:
                arr, S = normalize_model_sets(sets, base)
        else:
            sets = list(sets)
            if sets and isinstance(sets[0], (list, tuple)):
                if len(sets) != n_outer or len({len(r) for r in sets}) != 1:
                    raise ValueError("model sets per problem: G lists of the same length S")
                per = True
                S = len(sets[0])
                arr, _ = normalize_model_sets([d for r in sets for d in r], base)
            else:
                arr, S = normalize_model_sets(sets, base)
        n = S * n_outer if per else S
        c = (_lib.ModelSet * n)()
        for k in range(n):
            for f in fields:
                setattr(c[k], f, float(arr[f][k]))
        return c, S, per

    def _observations(self, ws, wd, yaw, power, weight, out):
        """The observations as contiguous arrays with their G axis: (ws, wd, yaw, power, weight, G, C, squeeze, on_device, like)."""
        N = self._w.num_turbines
        given = [ws, wd, yaw, power, weight] + list((out or {}).values())
        on_device = any(_is_torch(v) for v in given)
        like = None
        if on_device:
            import torch

            self._w._follow_torch_stream()
            like = next(v for v in given if _is_torch(v))

            def conv(a, dt):
                if a is None:
                    return None
                if not _is_torch(a):
                    a = torch.as_tensor(np.asarray(a, dt), device=like.device)
                assert a.is_cuda
                return a.to(getattr(torch, np.dtype(dt).name)).contiguous()
        else:
            def conv(a, dt):
                return None if a is None else np.ascontiguousarray(a, dtype=dt)
        ws, wd, power, weight = conv(ws, np.float64), conv(wd, np.float64), conv(power, np.float64), conv(weight, np.float64)
        yaw = conv(yaw, np.float32)
        squeeze = ws.ndim == 1
        if squeeze:
            ws, wd, yaw, power = ws[None], wd[None], yaw[None], power[None]
            weight = None if weight is None else weight[None]
        if ws.ndim != 2:
            raise ValueError("ws must be (G, C) or (C,): the wind speed of every condition")
        G, C_ = int(ws.shape[0]), int(ws.shape[1])
        for name, a, shape in (("wd", wd, (G, C_)), ("yaw", yaw, (G, C_, N)), ("power", power, (G, C_, N)), ("weight", weight, (G, C_, N))):
            if a is not None and tuple(a.shape) != shape:
                raise ValueError(f"{name} must be {'(G, C)' if len(shape) == 2 else '(G, C, num_turbines)'}, here {shape}: got {tuple(a.shape)}")
        return ws, wd, yaw, power, weight, G, C_, squeeze, on_device, like

    @staticmethod
    def _ptr(a, on_device):
        return None if a is None else (a.data_ptr() if on_device else a.ctypes.data)

    def score(self, sets, ws, wd, yaw, power, weight, scale, out, want, max_eval_farms):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        names = ("loss", "best", "row_power")
        if not want or any(k not in names for k in want):
            raise ValueError("want must name loss, best and / or row_power")
        ws, wd, yaw, power, weight, G, C_, squeeze, on_device, like = self._observations(ws, wd, yaw, power, weight, out)
        c, S, per = self._sets(sets, G)
        scale = w.rated_power() if scale is None else float(scale)
        self._call("config", int(max_eval_farms or 0))
        shapes = {"loss": ((G, S), np.float64), "best": ((G,), np.int32), "row_power": ((G, S, C_, N), np.float32)}
        spec = {k: shapes[k] for k in names if k in want}
        if out is not None and squeeze:
            out = {k: v[None] for k, v in out.items()}
        out, ptrs = self._outputs(out, spec, on_device, like)
        p = dict(zip(spec, ptrs))
        self._call("score", G, C_, S, c, int(per), *[self._ptr(a, on_device) for a in (ws, wd, yaw, power, weight)], scale,
                   *[p.get(k) for k in names], int(on_device))
        return {k: (out[k][0] if squeeze else out[k]) for k in spec}

    def fit(self, ws, wd, yaw, power, bounds, init, candidates, elites, sigma, seed, weight, scale, max_eval_farms):
        w = self._w
        N = w.num_turbines
        fields = _lib._MODEL_SET_FIELDS
        ws, wd, yaw, power, weight, G, C_, squeeze, on_device, like = self._observations(ws, wd, yaw, power, weight, None)
        unknown = sorted(set(bounds) - set(fields))
        if unknown:
            raise ValueError(f"unknown model-set field(s) in bounds: {unknown} (a set may change: {list(fields)})")
        if init is None:
            init = [{}]
        elif isinstance(init, dict) and not any(np.ndim(v) for v in init.values()):
            init = [init]
        ic, n_init, _ = self._sets(init, 1)
        if n_init not in (1, G):
            raise ValueError("init: one starting set, or one per problem")
        lo = np.array([getattr(ic[0], f) for f in fields], np.float64)
        hi = lo.copy()
        for k in range(1, n_init):  # a field that is not fitted is fixed at init: it must then be one value for all problems
            for j, f in enumerate(fields):
                if f not in bounds and getattr(ic[k], f) != lo[j]:
                    raise ValueError(f"init: {f} is not in bounds, so it is fixed — at ONE value for all problems")
        for f, (a, b) in bounds.items():
            lo[fields.index(f)], hi[fields.index(f)] = float(a), float(b)
        sg = np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64).reshape(-1)
        S, E, I = int(candidates), int(elites), int(sg.size)
        scale = w.rated_power() if scale is None else float(scale)
        self._call("config", int(max_eval_farms or 0))
        sets_t = np.dtype([(f, np.float64) for f in fields])
        shapes = {"best_set": ((G,), sets_t), "best_loss": ((G,), np.float64), "init_loss": ((G,), np.float64),
                  "history": ((G, I), np.float64), "mean": ((G,), sets_t), "fit_power": ((G, C_, N), np.float32),
                  "n_invalid": ((G,), np.int32)}
        # (a set goes through the C boundary as eighteen float64: (G, 18) arrays here, dicts of fields for the caller)
        raw = {k: (((G, len(fields)), np.float64) if d is sets_t else (s, d)) for k, (s, d) in shapes.items()}
        res, ptrs = self._outputs(None, raw, on_device, like)
        self._call("fit", G, C_, S, E, I, sg.ctypes.data, int(seed) & 0xFFFFFFFFFFFFFFFF, lo.ctypes.data, hi.ctypes.data, ic,
                   int(n_init == G and G > 1), *[self._ptr(a, on_device) for a in (ws, wd, yaw, power, weight)], scale, *ptrs,
                   int(on_device))
        ret = {}
        for k in self.FIT_OUTPUTS:
            v = res[k][0] if squeeze else res[k]
            ret[k] = {f: v[..., j] for j, f in enumerate(fields)} if k in ("best_set", "mean") else v
        return ret


class _ScenPlan(_Ext):
    """The `wf_scenplan` object of a WfStep handle (include/wfscenplan.h)."""

    NAME = "scenplan"
    KERNELS = ("paths", "advance")
    OUTPUTS = ("plan", "plan_score", "plan_expected", "plan_cvar", "plan_member_returns", "hold_score", "first_action", "final_yaw",
               "mean", "wind_paths")

    def run(self, horizon, candidates, elites, members, process, sigma, seed, scenario_seed, gamma, tail, risk_weight, anchor,
            bounds, mean, farms, strict, max_eval_farms, want, out):
        w = self._w
        N = w.num_turbines
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in self.OUTPUTS for k in want):
            raise ValueError("want must name " + ", ".join(self.OUTPUTS[:-1]) + " and / or " + self.OUTPUTS[-1])
        proc = _wind_process(process, "plan_scenarios")
        H, K, E = int(horizon), int(candidates), int(elites)
        M, q, ws_lo, ws_hi = self._members_tail_bounds(members, tail, bounds)
        if sigma is None:
            step = getattr(w, "_env_yaw_step", 5.0)
            sigma = (step, 0.5 * step, 0.25 * step)
        sg = np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64).reshape(-1)
        self._call("config", int(bool(strict)), int(max_eval_farms or 0))
        fa, n, fptr = self._farms(farms)
        on_device = _is_torch(anchor) or _is_torch(mean) or (out is not None and any(_is_torch(v) for v in out.values()))
        like = None
        if on_device:
            import torch

            w._follow_torch_stream()
            like = next(v for v in [anchor, mean] + list((out or {}).values()) if _is_torch(v))
        anchor, aptr = self._anchor(anchor, n, on_device, like)
        mptr = None
        if mean is not None:
            if on_device:
                if not _is_torch(mean):
                    mean = torch.as_tensor(np.asarray(mean, np.float32), device=like.device)
                assert mean.is_cuda and mean.dtype == torch.float32, "mean"
                mean = mean.contiguous()
            else:
                mean = np.ascontiguousarray(mean, dtype=np.float32)
            if tuple(mean.shape) != (n, H, N):
                raise ValueError("mean must be (n_farms, H, num_turbines): the warm start of every listed farm")
            mptr = mean.data_ptr() if on_device else mean.ctypes.data
        shapes = {"plan": ((n, H, N), np.float32), "plan_score": ((n,), np.float64), "plan_expected": ((n,), np.float64),
                  "plan_cvar": ((n,), np.float64), "plan_member_returns": ((n, M), np.float64), "hold_score": ((n,), np.float64),
                  "first_action": ((n, N), np.float32), "final_yaw": ((n, N), np.float32), "mean": ((n, H, N), np.float32),
                  "wind_paths": ((n, M, H, 2), np.float64)}
        spec = {k: shapes[k] for k in self.OUTPUTS if k in want}
        if out is None and not (1 <= M <= 64 and 1 <= H <= 64 and K * M * H <= 4096):
            spec = {k: ((0,), d) for k, (_, d) in spec.items()}  # (the library refuses these limits by name: nothing to allocate)
        out, ptrs = self._outputs(out, spec, on_device, like)
        ptr = dict(zip(spec, ptrs))
        self._call("run", H, K, E, int(sg.size), sg.ctypes.data, C.c_ulonglong(int(seed) & (2**64 - 1)), float(gamma), M, C.byref(proc),
                   ws_lo, ws_hi, C.c_ulonglong(int(scenario_seed) & (2**64 - 1)), q, float(risk_weight), aptr, mptr, n, fptr,
                   *[ptr.get(k) for k in self.OUTPUTS], int(on_device))
        return {k: out[k] for k in spec}
