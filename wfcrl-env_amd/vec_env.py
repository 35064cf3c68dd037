"""`VecWindFarmEnv` — B independent wind-farm envs stepped by ONE fused kernel launch.

Batched restatement of the reference's centralised env: reset wind sampling (wfcrl/mdp.py:233-271),
actuation budget (simple_env.py:64-72), yaw transition (mdp.py:291-319), reward (simple_env.py:78-85),
truncation bookkeeping (interface.py:578-586, mdp.py:261-262).  Env state (yaw, actuation accumulators,
move counters) lives on the device; actions and observations are torch CUDA tensors (NumPy accepted).
All B envs share the horizon, so they truncate together and are reset together.

Differences from running B reference envs, by construction of a batch: `reset` draws all winds from ONE
`default_rng(seed)` (vectorised weibull then normal draws; for B = 1 this is exactly the reference's
stream), and constrained actions are not zeroed in the caller's array (the gate is applied on the device).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from ._compat import spaces
from .backend import WfStep
from .mdp import WD_MEAN, WD_STD, WEIBULL_SCALE, WEIBULL_SHAPE, WindFarmMDP
from .rewards import DoNothingReward, ReferencePercentage, StepPercentage

_OBS_KEYS = ("yaw", "freewind_measurements", "wind_speed", "wind_direction")


class VecWindFarmEnv:
    metadata = {"name": "vectorized-centralized-windfarm"}

    def __init__(self, farm_case, controls: dict = None, env_batch: int = 1, continuous_control: bool = True,
                 reward_shaper=None, start_iter: int = 0, max_num_steps: int = 500, load_coef: float = 0.1,
                 device_id: int = 0, model: dict = None, return_torch: bool = True, backend=None,
                 wind_sampling: str = "host", reuse_buffers: bool = True, wind_direction_step: float = None,
                 actuation_budget: float = 0.1, kernel_choice: dict = None, risk_resolve: bool = None,
                 layouts: dict = None, wind_process: dict = None, model_randomization: dict = None):
        controls = {"yaw": (-40, 40, 5)} if controls is None else dict(controls)
        if list(controls) != ["yaw"]:
            raise ValueError(f"Cannot control {list(controls)}. Interface HipFlorisInterface only allows for the "
                             "following: ['yaw']")
        spec = controls["yaw"]
        if not (len(spec) in (2, 3) and spec[0] < spec[1]):
            raise ValueError("Wrong bounds for actuator yaw: ensure that lower_bound < upper_bound")
        if len(spec) == 2:
            spec = tuple(spec) + (1,)
        self.controls = {"yaw": tuple(spec)}
        self.farm_case = farm_case.clone() if hasattr(farm_case, "clone") else farm_case
        self.num_envs = int(env_batch)
        self.num_turbines = self.farm_case.num_turbines
        self.continuous_control = continuous_control
        self.max_num_steps = max_num_steps
        self.start_iter = start_iter
        self.load_coef = load_coef
        self.dt = self.farm_case.dt
        self.reward_shaper = DoNothingReward() if reward_shaper is None else reward_shaper
        self.return_torch = return_torch
        self.farm_case.max_iter = start_iter + max_num_steps
        p = self.farm_case.simul_params
        self.fi = backend if backend is not None else WfStep(p["xcoords"], p["ycoords"], env_batch=self.num_envs,
                                                              device_id=device_id, model=model, kernel_choice=kernel_choice)
        # risk_resolve: every farm the float32 kernel flags is solved again in float64 behind each step (wf_set_risk_resolve)
        # — the reference computes every step in float64 (interface.py:564), and north_star's 1e-4 holds on EVERY farm only
        # with it.  ON unless told otherwise (it is the default of the handle itself, ABI 6); a caller's own `backend=` is left as
        # it was configured unless risk_resolve is given — one set up for mode 2 (every farm in float64) stays in mode 2.  Nothing measurable where no
        # farm is flagged (a shared 270 deg wind on HornsRev1); about +1 ms per step where a wind per farm flags ~1 % of the
        # batch.  risk_resolve=False is the opt-out for throughput runs that accept the per-flag bounds of
        # include/wfstep.h on flagged farms.
        if risk_resolve is not None or backend is None:
            self.fi.set_risk_resolve(0 if risk_resolve is False else 1)
        # layouts: several layouts in the batch — dict(xcoords=[K][N], ycoords=[K][N], layout_of=[env_batch] or None for
        # K == env_batch[, counts=[K]]), each with the case's number of turbines or — with `counts`, or ragged lists of
        # coordinates — fewer (backend.WfStep.set_layouts: observations, powers and loads of the missing turbines are 0,
        # the reward averages over the real ones); the case's own layout is then only the default the handle returns to
        if layouts is not None:
            self.fi.set_layouts(layouts["xcoords"], layouts["ycoords"], layouts.get("layout_of"), layouts.get("counts"))
        self.fi.env_config(yaw_lo=spec[0], yaw_hi=spec[1], yaw_step=spec[2],
                           actuator_rate=WindFarmMDP.ACTUATORS_RATE["yaw"], dt=self.dt, budget=actuation_budget,
                           load_coef=load_coef, discrete=not continuous_control, power_mw=True)
        n = self.num_turbines
        # per-env spaces, identical to the reference's (mdp.py:108-153)
        if continuous_control:
            self.single_action_space = spaces.Dict({"yaw": spaces.Box(-spec[2], spec[2], shape=(n,))})
        else:
            self.single_action_space = spaces.Dict({"yaw": spaces.MultiDiscrete([3] * n)})
        ones = np.ones(n, dtype=np.float32)
        b = WindFarmMDP.DEFAULT_BOUNDS
        self.single_observation_space = spaces.Dict(OrderedDict([
            ("yaw", spaces.Box(ones * spec[0], ones * spec[1], shape=(n,))),
            ("freewind_measurements", spaces.Box(np.array([b["wind_speed"][0], b["wind_direction"][0]], np.float32),
                                                 np.array([b["wind_speed"][1], b["wind_direction"][1]], np.float32),
                                                 shape=(2,))),
            ("wind_speed", spaces.Box(ones * b["wind_speed"][0], ones * b["wind_speed"][1], shape=(n,))),
            ("wind_direction", spaces.Box(ones * b["wind_direction"][0], ones * b["wind_direction"][1], shape=(n,))),
        ]))
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space
        if wind_sampling not in ("host", "device"):
            raise ValueError("wind_sampling must be 'host' (NumPy stream of the reference) or 'device' (Philox on the GPU)")
        self.wind_sampling = wind_sampling
        # build-defined option of device sampling: reset directions rounded to a grid of that many degrees (must divide
        # 360), so that every step stays on the pair-table path (backend.WfStep.sample_wind)
        self.wind_direction_step = wind_direction_step
        ts = self.farm_case.wind_time_series
        has_series = ts is not None and (ts.size > 0 if isinstance(ts, np.ndarray) else bool(ts))
        if has_series:
            from .interface import _load_time_series

            self._series = np.ascontiguousarray(_load_time_series(ts)[:, :2], dtype=np.float64)
        else:
            self._series = None
        # wind_process: a synthetic wind episode — a stochastic wind series per farm, generated on the device at every reset
        # (include/wfwindgen.h; backend.WfStep.generate_wind): dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=,
        # dist=None), missing parameters 0.  Every farm then sees a changing wind of its own, reproducible from the reset's
        # seed, and everything the env does on a time-series episode applies: the tick before the step, wind_preview,
        # wind="series".  None (the default): the wind holds from reset to truncation, as in the reference.
        self._wind_process = self._wind_dist = None
        if wind_process is not None:
            if has_series:
                raise ValueError("wind_process generates the episode's wind: it cannot be combined with a case's wind_time_series")
            wp = dict(wind_process)
            self._wind_dist = wp.pop("dist", None)
            unknown = set(wp) - {"ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp"}
            if unknown:
                raise ValueError(f"unknown wind_process parameter(s): {sorted(unknown)}")
            self._wind_process = {k: float(v) for k, v in wp.items()}
        self._generated = None  # what regenerates the running episode: seed, T, ws0, wd0 (get_state)
        # model_randomization: wake-model parameter sets per farm (include/wfmodelset.h; backend.WfStep.set_model_sets) —
        #   dict(ranges={field: (lo, hi), ...}, n_sets=min(B, 256), resample="reset" | "once")   n_sets sets drawn uniformly in
        #       the ranges (other fields: the model), each farm assigned a set by a draw; at construction ("once") or at
        #       every reset(seed) ("reset"), from a NumPy generator of their OWN seeded by (seed, a fixed tag): the wind
        #       stream of _sample_wind is the one it always was
        #   dict(sets=..., set_of=...)   given explicitly
        # COST: every farm is then solved by the float64 kernels on every step.  The observation is unchanged; env.model_sets /
        # env.model_set_of expose what is in force.  None (the default) changes nothing.
        self._model_rand = None
        if model_randomization is not None:
            self._model_rand = self._check_model_randomization(model_randomization, self.num_envs)
            mr = self._model_rand
            if "sets" in mr:
                self.fi.set_model_sets(mr["sets"], mr["set_of"])
            elif mr["resample"] == "once":
                self._draw_model_sets(mr.get("seed"))
        # an episode whose wind changes from step to step: a file series or a generated one
        self._playing = self._series is not None or self._wind_process is not None
        self._num_iter = 0
        self._freewind = None
        self._shaper_ref = None
        # reuse_buffers=True (the DEFAULT since round 6; torch path): the output tensors of `step` / `step_light` are two
        # preallocated sets used alternately — what step t returned stays valid until step t + 2 overwrites it: enough for
        # (obs, next_obs) pairs; ALIASING: anything that must live longer (rollout storage, loggers, a list of observations)
        # has to be copied (`.clone()`) by the caller, or the env built with reuse_buffers=False, which allocates fresh
        # tensors every step as B reference envs would (+3 % per step on the headline batch).  The logged / AEC flavours
        # (environments.make(..., log=True), Dec_*) keep what they return and therefore build their inner env without reuse.
        self.reuse_buffers = bool(reuse_buffers) and return_torch
        self._bufs = [{}, {}]
        self._flip = 0
        self._const = {}

    # -- helpers ------------------------------------------------------------------------------------
    MODEL_RANDOMIZATION_TAG = 0x6D736574  # "mset": the second word of the seed of the sets' own generator

    @staticmethod
    def _check_model_randomization(mr, B) -> dict:
        """Validated copy of a model_randomization argument (needs no device)."""
        from . import _lib

        if not isinstance(mr, dict):
            raise ValueError("model_randomization must be a dict: (ranges[, n_sets, resample, seed]) or (sets[, set_of])")
        mr = dict(mr)
        if "sets" in mr:
            unknown = set(mr) - {"sets", "set_of"}
            if unknown:
                raise ValueError(f"model_randomization: give either (sets, set_of) or (ranges, n_sets, resample): {sorted(unknown)}")
            mr.setdefault("set_of", None)
            return mr
        unknown = set(mr) - {"ranges", "n_sets", "resample", "seed"}
        if unknown or "ranges" not in mr:
            raise ValueError(f"model_randomization: unknown key(s) {sorted(unknown)}; give ranges={{field: (lo, hi)}}")
        ranges = {}
        for k, v in dict(mr["ranges"]).items():
            if k not in _lib._MODEL_SET_FIELDS:
                raise ValueError(f"model_randomization: unknown model-set field(s): ['{k}'] (a set may change: {list(_lib._MODEL_SET_FIELDS)})")
            lo, hi = float(v[0]), float(v[1])
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError(f"model_randomization: range of {k} must be finite with lo <= hi")
            ranges[k] = (lo, hi)
        n_sets = int(mr.get("n_sets", min(B, 256)))
        if not 1 <= n_sets <= B:
            raise ValueError("model_randomization: n_sets must be in 1..env_batch")
        resample = mr.get("resample", "reset")
        if resample not in ("reset", "once"):
            raise ValueError("model_randomization: resample must be 'reset' or 'once'")
        return {"ranges": ranges, "n_sets": n_sets, "resample": resample, "seed": mr.get("seed")}

    def _draw_model_sets(self, seed):
        """n_sets sets uniform in the ranges and a set per farm, from a generator of their own: (seed, tag)."""
        mr = self._model_rand
        s = int(seed) if seed is not None else int(np.random.randint(0, 2**31 - 1))
        rng = np.random.default_rng([s, self.MODEL_RANDOMIZATION_TAG])
        sets = {k: rng.uniform(lo, hi, mr["n_sets"]) for k, (lo, hi) in sorted(mr["ranges"].items())}
        set_of = rng.integers(0, mr["n_sets"], self.num_envs).astype(np.int32)
        self.fi.set_model_sets(sets, set_of)

    @property
    def model_sets(self):
        """The parameter sets in force: dict of float64 arrays of length S (None without model_randomization)."""
        return None if self._model_rand is None else self.fi.model_sets()[0]

    @property
    def model_set_of(self):
        """The set of each farm, int32 [env_batch] (None without model_randomization)."""
        return None if self._model_rand is None else self.fi.model_sets()[1]

    def _sample_wind(self, seed, options):
        rng = np.random.default_rng(seed)
        B = self.num_envs
        lo, hi = self.single_observation_space["freewind_measurements"].low, \
            self.single_observation_space["freewind_measurements"].high
        if options is not None and "wind_speed" in options:
            ws = np.broadcast_to(np.asarray(options["wind_speed"], np.float64), (B,)).copy()
        elif self.farm_case.set_wind_speed:
            ws = np.full(B, float(self.farm_case.simul_params["speed"]))
        else:
            ws = np.clip(WEIBULL_SCALE * rng.weibull(WEIBULL_SHAPE, B), lo[0], hi[0])
        if options is not None and "wind_direction" in options:
            wd = np.broadcast_to(np.asarray(options["wind_direction"], np.float64), (B,)).copy()
        elif self.farm_case.set_wind_direction:
            wd = np.full(B, float(self.farm_case.simul_params["direction"]))
        else:
            wd = np.clip(rng.normal(WD_MEAN, WD_STD, B) % 360, lo[1], hi[1])
        return ws, wd % 360

    def _refresh_freewind(self):
        if self.return_torch:
            import torch

            ws, wd = self.fi.get_wind(as_torch=True)
            self._freewind = torch.stack([ws, wd], dim=1)
        else:
            ws, wd = self.fi.get_wind()
            self._freewind = np.stack([ws, wd], axis=1)

    def _obs(self, out):
        obs = OrderedDict()
        obs["yaw"] = out["yaw"]
        obs["freewind_measurements"] = self._freewind
        obs["wind_speed"] = out["wind_speed"]
        obs["wind_direction"] = out["wind_direction"]
        return obs

    def _next_buf(self):
        if not self.reuse_buffers:
            return None
        self._flip ^= 1
        return self._bufs[self._flip]

    def _to_device(self, a):
        if not self.return_torch:
            return np.ascontiguousarray(a, dtype=np.float32)
        import torch

        if isinstance(a, torch.Tensor):
            return a.to(device=f"cuda:{self.fi.device_id}", dtype=torch.float32)
        return torch.as_tensor(np.asarray(a, dtype=np.float32), device=f"cuda:{self.fi.device_id}")

    def _shape(self, r):
        """Batched reward shaping with the semantics of reference wfcrl/rewards.py:4-46, per env.  Dispatch is by class
        name, so a shaper instance built from the `wfcrl.rewards` alias of this package is recognised as well."""
        s = self.reward_shaper
        kind = type(s).__name__
        if kind == "DoNothingReward":
            return r
        if kind == "ReferencePercentage":
            return (r - s.reference) / s.reference
        if kind == "StepPercentage":
            # per-env previous reward, seeded from the shaper's own `reference` (constructor / reset value); a previous
            # reward of exactly 0 yields 0.0 (rewards.py:36-37), and the shaper object keeps the state like the
            # reference's does
            ref = self._shaper_ref
            if ref is None:
                base = s.reference
                ref = base if np.ndim(base) > 0 else r * 0 + float(base)
            zero = ref == 0
            safe = ref + zero  # 1 where the previous reward is 0: no division by zero, result replaced below
            shaped = (r - ref) / safe
            shaped = shaped * (~zero) if hasattr(shaped, "clone") else np.where(zero, 0.0, shaped)
            self._shaper_ref = r.clone() if hasattr(r, "clone") else r.copy()
            s.reference = self._shaper_ref
            return shaped
        return s(r)

    # -- episode ------------------------------------------------------------------------------------
    def reset(self, seed=None, options=None):
        """Samples one wind per env, zeroes the env state, runs the warm-up solve(s) at yaw = 0 and returns
        the start observation (clipped to the observation space like the reference's, mdp.py:263-266)."""
        if self._model_rand is not None and self._model_rand.get("resample") == "reset":
            self._draw_model_sets(seed)
        if self._series is not None:
            # time-series mode: requested / sampled wind is ignored (interface.py:588-600); every farm starts at a
            # random row (interface.py:516-518), then each solve consumes one row
            s = seed if seed is not None else int(np.random.randint(0, 2**31 - 1))
            self.fi.set_wind_series(self._series, start=None, seed=s)
        elif self._wind_process is not None:
            # a generated episode: reset consumes start_iter + 1 ticks and every step one more, so the last step of the
            # episode plays the last tick; options give tick 0 instead of the draw
            s = seed if seed is not None else int(np.random.randint(0, 2**31 - 1))
            ws0 = wd0 = None
            if options and ("wind_speed" in options or "wind_direction" in options):
                ws0, wd0 = self._sample_wind(seed, options)
            self._generated = {"seed": int(s), "T": int(self.start_iter + self.max_num_steps + 2), "ws0": ws0, "wd0": wd0}
            self.fi.generate_wind(self._generated["T"], s, self._wind_process, dist=self._wind_dist, ws0=ws0, wd0=wd0)
        elif self.wind_sampling == "device" and not (options and ("wind_speed" in options or "wind_direction" in options)) \
                and not (self.farm_case.set_wind_speed or self.farm_case.set_wind_direction):
            s = seed if seed is not None else int(np.random.randint(0, 2**31 - 1))
            self.fi.sample_wind(s, direction_step=self.wind_direction_step)
        else:
            ws, wd = self._sample_wind(seed, options)
            if np.all(ws == ws[0]) and np.all(wd == wd[0]):
                self.fi.set_wind(ws[0], wd[0])  # one wind for the whole batch: shared-wind (pair table) path
            else:
                self.fi.set_wind(ws, wd)
        self.fi.env_reset()
        self.reward_shaper.reset()
        self._shaper_ref = None
        seed_out = None
        if self.return_torch:
            import torch

            seed_out = {"yaw": torch.empty((self.num_envs, self.num_turbines), device=f"cuda:{self.fi.device_id}")}
        self._num_iter = 0
        out = None
        for _ in range(self.start_iter + 1):
            if self._playing:
                self.fi.wind_series_step()
            out = self.fi.env_step(None, want=("yaw", "wind_speed", "wind_direction"), out=seed_out)
            self._num_iter += 1
        self._refresh_freewind()
        obs = self._obs(out)
        sp = self.single_observation_space
        for k in ("wind_speed", "wind_direction"):
            lo, hi = float(sp[k].low[0]), float(sp[k].high[0])
            obs[k] = obs[k].clamp(lo, hi) if self.return_torch else np.clip(obs[k], lo, hi)
        # the whole start state is clipped to the observation bounds (mdp.py:263-266), the free wind included; the first
        # reward is normalised by that clipped speed (simple_env.py:78-80 reads the state before the step)
        lo, hi = sp["freewind_measurements"].low, sp["freewind_measurements"].high
        fw = obs["freewind_measurements"]
        if self.return_torch:
            import torch

            clipped = torch.minimum(torch.maximum(fw, torch.as_tensor(lo, dtype=fw.dtype, device=fw.device)),
                                    torch.as_tensor(hi, dtype=fw.dtype, device=fw.device))
            changed = bool((clipped[:, 0] != fw[:, 0]).any()) if not self._playing else False
        else:
            clipped = np.clip(fw, lo, hi)
            changed = bool((clipped[:, 0] != fw[:, 0]).any()) if not self._playing else False
        obs["freewind_measurements"] = clipped
        if changed:
            self.fi.env_set_prev_wind(clipped[:, 0].cpu().numpy() if self.return_torch else clipped[:, 0])
        return obs

    def step(self, actions):
        """actions: {"yaw": (B, N)} or the (B, N) array itself.  Returns (obs, reward[B], terminated[B],
        truncated[B], info) with info["power"] in MW and info["load"] (B, N, 4) — units of the reference."""
        a = actions["yaw"] if isinstance(actions, dict) else actions
        if self._playing:
            self.fi.wind_series_step()  # ValueError("wind series exhausted") ~ the reference's StopIteration
            self._refresh_freewind()
        buf = self._next_buf()
        out = self.fi.env_step(self._to_device(a), out=buf)
        self._num_iter += 1
        truncated = self._num_iter == self.farm_case.max_iter
        reward = self._shape(out["reward"])
        if self.return_torch:
            import torch

            if buf is not None:
                buf.update(out)  # keep the tensors env_step allocated on first use
            info = {"power": out["power"], "load": out["load"]}  # (MW out of the kernel: wf_env_set_power_unit)
            if not self._const:
                dev = out["reward"].device
                self._const = {False: torch.zeros(self.num_envs, dtype=torch.bool, device=dev),
                               True: torch.ones(self.num_envs, dtype=torch.bool, device=dev)}
            trunc, term = self._const[bool(truncated)], self._const[False]
        else:
            info = {"power": out["power"], "load": out["load"]}
            trunc = np.full(self.num_envs, bool(truncated))
            term = np.zeros(self.num_envs, bool)
        return self._obs(out), reward, term, trunc, info

    def step_light(self, actions):
        """Learner-facing variant: only reward + local wind observations leave the kernel (no power/load
        arrays are written: 2N+1 instead of 7N floats per env)."""
        a = actions["yaw"] if isinstance(actions, dict) else actions
        if self._playing:
            self.fi.wind_series_step()
            self._refresh_freewind()
        buf = self._next_buf()
        out = self.fi.env_step(self._to_device(a), want=("reward", "yaw", "wind_speed", "wind_direction"), out=buf)
        if buf is not None:
            buf.update(out)
        self._num_iter += 1
        return self._obs(out), self._shape(out["reward"]), self._num_iter == self.farm_case.max_iter

    def sample_flow(self, points, farms=None):
        """The flow (u, v, w) at `points` — (P, 3) for every farm or (num_envs, P, 3) per farm; x, y in the layout's
        coordinates, z above ground — at the envs' CURRENT yaw state and wind: (n_farms, P, 3) float32, a torch CUDA tensor
        when the env returns torch.  A virtual met mast or lidar for an agent; reads the env state, never changes it
        (backend.WfStep.sample_flow with yaw=None; a point value is defined in include/wfprobe.h, PARITY UNPINNED)."""
        nd = points.dim() if hasattr(points, "dim") else np.ndim(points)
        # the same NumPy points as the probe holds (a met mast sampled every step): no new upload, which would validate and
        # synchronise.  The probe itself remembers them, so a set_probe_points on self.fi in between is seen.
        if not self.fi._probe().holds(points, nd == 3):
            self.fi.set_probe_points(points, per_farm=nd == 3)
        out = None
        if self.return_torch:
            import torch

            n = self.num_envs if farms is None else int(np.size(farms))
            P = points.shape[-2] if hasattr(points, "shape") else np.shape(points)[-2]
            out = torch.empty((n, int(P), 3), dtype=torch.float32, device=f"cuda:{self.fi.device_id}")
        return self.fi.sample_flow(None, farms=farms, out=out)

    def optimal_yaw(self, passes=(5, 4), strict=False, farms=None, wd_uncertainty=None):
        """The best static yaw for the farms' CURRENT wind — the baseline a wake-steering agent is held to: dict(yaw
        (n_farms, N), power (n_farms,) W, power_initial (n_farms,) W at zero yaw), torch CUDA tensors when the env returns
        torch.  Bounds are the env's yaw limits, the start is zero yaw.  The project's own coordinate search
        (backend.WfStep.optimize_yaw, include/wfyawopt.h; not pinned to FLORIS' optimiser), run on a handle of its own:
        the env's yaw state, accumulators, wind and buffers are read, never changed.  wd_uncertainty (a dict, see
        backend.wd_uncertainty_members): the robust baseline of include/wfrobust.h — the yaw that maximises the EXPECTED
        power over the direction offsets; the two powers are then expected powers."""
        lo, hi = self.controls["yaw"][0], self.controls["yaw"][1]
        out = None
        if self.return_torch:
            import torch

            n = self.num_envs if farms is None else int(np.size(farms))
            dev = f"cuda:{self.fi.device_id}"
            out = {"yaw": torch.empty((n, self.num_turbines), dtype=torch.float32, device=dev),
                   "power": torch.empty(n, dtype=torch.float32, device=dev),
                   "power_initial": torch.empty(n, dtype=torch.float32, device=dev)}
        return self.fi.optimize_yaw(None, farms=farms, bounds=(lo, hi), passes=passes, strict=strict, out=out,
                                    wd_uncertainty=wd_uncertainty)

    def power_gradient(self, cotangent=None, farms=None, step=1.0, strict=False):
        """How the power changes when a turbine turns, at the farms' CURRENT yaw state and wind: dict(power (n_farms, N) W
        float32 — the per-turbine power at the current yaw —, gradient (n_farms, N) W/deg float64), torch CUDA tensors when
        the env returns torch.  gradient[b, i] = sum_j cotangent[b, j] d P_j / d yaw_i; cotangent None: ones, the gradient
        of the farm power; a one-hot row gives turbine j's credit to every agent's yaw.  The derivative is the DIFFERENCE
        QUOTIENT of include/wfgrad.h at `step` degrees (backend.WfStep.yaw_gradient; the project's own definition), with
        the env's yaw limits as bounds: one-sided at a limit.  Run on a handle of its own: the env's yaw state,
        accumulators, wind and buffers are read, never changed."""
        lo, hi = self.controls["yaw"][0], self.controls["yaw"][1]
        yaw = self.fi.env_get_state(as_torch=self.return_torch)["yaw"]
        if farms is not None:
            idx = np.ascontiguousarray(farms, dtype=np.int64).reshape(-1)
            if self.return_torch:
                import torch

                yaw = yaw[torch.from_numpy(idx).to(yaw.device)]
            else:
                yaw = yaw[idx]
        if cotangent is not None and self.return_torch:
            cotangent = self._to_device(cotangent).float().reshape(yaw.shape)
        return self.fi.yaw_gradient(yaw, cotangent, farms=farms, step=step, bounds=(lo, hi), strict=strict)

    def counterfactual_rewards(self, actions, alternatives="hold", farms=None, strict=False, wind=None):
        """Per-agent counterfactuals of the joint action the env is ABOUT to take — call it BEFORE `step(actions)`:
        dict(reward_base (n_farms,), reward_alt (n_farms, N, K), difference (n_farms, N, K) = reward_base - reward_alt),
        float64, torch CUDA tensors when the env returns torch.  reward_base is the reward `step(actions)` will pay (to the
        step's tolerance); reward_alt[b, i, k] the one it would pay had turbine i alone taken alternative k:
          "hold"   the hold action (difference rewards against "did nothing"), K = 1
          "zero"   absolute zero yaw, K = 1
          "all"    discrete control: the three actions down / hold / up, K = 3 — the rows of a COMA baseline
          an action array (num_envs, N, K) in the env's encoding
        actions is the whole batch's (num_envs, N); farms picks the farms served.  Every action goes through the step's own
        budget gate, increment and clip on the env's state (include/wfcredit.h; backend.WfStep.counterfactual_rewards; the
        project's own definition).  Run on a handle of its own: the env's yaw state, accumulators, wind and buffers are
        read, never changed.  strict=True solves every row in float64: the mode for large farms and small differences.
        On a time-series episode pass wind="series": every row is solved under the series' coming row, the wind `step` will
        tick to (include/wfseries.h)."""
        self._series_keyword("counterfactual_rewards", wind, "step")
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("counterfactual_rewards needs the plain reward (DoNothingReward): the effect of a reward shaper "
                             "is not defined per agent")
        a = self._to_device(actions["yaw"] if isinstance(actions, dict) else actions)
        B, N = self.num_envs, self.num_turbines
        if tuple(a.shape) != (B, N):
            raise ValueError("actions must be (num_envs, num_turbines): the joint action of the whole batch")
        idx = None if farms is None else np.ascontiguousarray(farms, dtype=np.int64).reshape(-1)
        n = B if idx is None else idx.size

        def pick(v):
            if idx is None:
                return v
            if self.return_torch:
                import torch

                return v[torch.from_numpy(idx).to(v.device)]
            return v[idx]

        alt, alt_kind = None, "action"
        if isinstance(alternatives, str):
            if alternatives == "zero":
                alt_kind = "yaw"
            elif alternatives == "all":
                if self.continuous_control:
                    raise ValueError('alternatives="all" lists the three discrete actions: the env has continuous control')
                alt = self._to_device(np.broadcast_to(np.float32([0.0, 1.0, 2.0]), (n, N, 3)).copy())
            elif alternatives != "hold":
                raise ValueError('alternatives must be "hold", "zero", "all" or an action array (num_envs, N, K)')
        else:
            alt = self._to_device(alternatives)
            if alt.ndim != 3 or tuple(alt.shape[:2]) != (B, N):
                raise ValueError("an alternatives array must be (num_envs, num_turbines, K)")
            alt = pick(alt)
        r = self.fi.counterfactual_rewards(pick(a), alt, base_kind="action", alt_kind=alt_kind, farms=farms, strict=strict, wind=wind)
        K = 1 if alt is None else int(alt.shape[2])
        return {"reward_base": r["reward"][:, 0], "reward_alt": r["reward"][:, 1:].reshape(n, N, K), "difference": r["difference"]}

    def lookahead_returns(self, action_sequences, gamma=1.0, farms=None, strict=False, wind=None):
        """The discounted return the env would pay over the next H steps for each of K candidate action sequences, from
        the state it is in — call it BEFORE `step`: dict(returns (n_farms, K) float64, rewards (n_farms, K, H) float64,
        final_yaw (n_farms, K, N) float32, best (n_farms,) int32 — the sequence of the largest return, the lowest index among
        equal ones), torch CUDA tensors when the env returns torch.  action_sequences is {"yaw": (num_envs, K, H, N)} or
        the array itself, in the env's action encoding; farms picks the farms served.  rewards[:, k, 0] is the reward
        `step(action_sequences[:, k, 0])` will pay (to the step's tolerance).  Every action goes through the step's own budget
        gate, increment and clip, and the accumulators and the move counter advance along each sequence; the wind the env
        holds is held over the horizon (include/wflookahead.h; backend.WfStep.lookahead_returns; the project's own
        definition).  Run on a handle of its own: the env's yaw state, accumulators, wind and buffers are read, never
        changed.  strict=True solves every row in float64: the mode for near-equal candidates.  On a time-series episode
        pass wind="series": step h is solved under the series' row of tick t + 1 + h, the last row held past the end of the
        series (include/wfseries.h)."""
        self._series_keyword("lookahead_returns", wind, "steps")
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("lookahead_returns needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        a = self._to_device(action_sequences["yaw"] if isinstance(action_sequences, dict) else action_sequences)
        B, N = self.num_envs, self.num_turbines
        if a.ndim != 4 or a.shape[0] != B or a.shape[3] != N:
            raise ValueError("action_sequences must be (num_envs, K, H, num_turbines): K sequences of H joint actions per farm")
        if farms is not None:
            idx = np.ascontiguousarray(farms, dtype=np.int64).reshape(-1)
            if self.return_torch:
                import torch

                a = a[torch.from_numpy(idx).to(a.device)]
            else:
                a = a[idx]
        return self.fi.lookahead_returns(a, gamma=gamma, wind=wind, farms=farms, strict=strict,
                                         want=("returns", "rewards", "final_yaw", "best"))

    def scenario_returns(self, action_sequences, members=8, process=None, seed=0, gamma=1.0, tail=None, risk_weight=0.0,
                         anchor=None, bounds=None, farms=None, strict=False,
                         want=("expected_returns", "cvar", "score", "best")):
        """The returns of K candidate action sequences over an ensemble of `members` wind futures drawn from the wind
        process, from the state the env is in — call it BEFORE `step`: per sequence the mean over the members
        ("expected_returns"), the tail mean of the `tail` lowest member returns ("cvar"), score = (1 - risk_weight) mean +
        risk_weight cvar, and "best", the sequence of the largest score; `want` may also name "member_returns", "rewards",
        "wind_paths" and "final_yaw" (include/wfscenario.h; backend.WfStep.scenario_returns; the project's own definition).
        action_sequences is {"yaw": (num_envs, K, H, N)} or the array itself, in the env's action encoding; K M H <= 4096.
        process=None takes the env's wind_process and its distribution's speed bounds; an env without wind_process must be
        given `process` (and may be given `bounds`, default 3 to 28 m/s).  The paths start at every farm's current wind and
        revert to `anchor` (n_farms, 2), default the current wind: the planner knows the process, not the episode's
        realisation — between lookahead_returns(wind=None), which holds the wind, and wind="series", which reads the
        future.  Works on any episode kind (held wind, file series, generated): only the current wind is read.  Run on a
        handle of its own: the env's yaw state, accumulators, wind and buffers are read, never changed."""
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("scenario_returns needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        if process is None:
            if self._wind_process is None:
                raise ValueError("scenario_returns needs a wind process: this env was built without wind_process, so pass "
                                 "process=dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=)")
            process = self._wind_process
            if bounds is None and self._wind_dist is not None:
                bounds = (float(self._wind_dist.get("ws_lo", 3.0)), float(self._wind_dist.get("ws_hi", 28.0)))
        if bounds is None:
            bounds = (3.0, 28.0)
        a = self._to_device(action_sequences["yaw"] if isinstance(action_sequences, dict) else action_sequences)
        B, N = self.num_envs, self.num_turbines
        if a.ndim != 4 or a.shape[0] != B or a.shape[3] != N:
            raise ValueError("action_sequences must be (num_envs, K, H, num_turbines): K sequences of H joint actions per farm")
        if farms is not None:
            idx = np.ascontiguousarray(farms, dtype=np.int64).reshape(-1)
            if self.return_torch:
                import torch

                a = a[torch.from_numpy(idx).to(a.device)]
            else:
                a = a[idx]
        return self.fi.scenario_returns(a, members, process, seed=seed, gamma=gamma, tail=tail, risk_weight=risk_weight,
                                        anchor=anchor, bounds=bounds, farms=farms, strict=strict, want=want)

    def return_gradient(self, action_sequences, gamma=1.0, terminal=None, delta=1.0, farms=None, strict=False, wind=None):
        """The derivative of lookahead_returns' returns with respect to the action sequences, from the state the env is
        in — call it BEFORE `step`: dict(returns (n_farms, K) float64, rewards (n_farms, K, H) float64, action_gradient
        (n_farms, K, H, N) float64 [reward per degree], reward_gradient (n_farms, K, H, N) float64 — the undiscounted
        per-step quotients —, state_gradient (n_farms, K, N) float64 — with respect to the yaw the env holds —, yaw
        (n_farms, K, H, N) float32 — the trajectory —, pass_mask (n_farms, K, H, N) uint8), torch CUDA tensors when the env
        returns torch.  action_sequences is {"yaw": (num_envs, K, H, N)} or the array itself; continuous control only.
        terminal (n_farms, K, N) float64 is the derivative of a terminal value with respect to the final yaw (a critic's
        gradient), delta the perturbation in degrees.  A difference quotient at a finite step chained through the
        transition's 0/1 Jacobian (include/wfretgrad.h; backend.WfStep.return_gradient; the project's own definition).  Run
        on a handle of its own: the env's yaw state, accumulators, wind and buffers are read, never changed.  strict=True
        solves every row in float64.  On a time-series episode pass wind="series", as to lookahead_returns."""
        self._series_keyword("return_gradient", wind, "steps")
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("return_gradient needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        a = self._to_device(action_sequences["yaw"] if isinstance(action_sequences, dict) else action_sequences)
        B, N = self.num_envs, self.num_turbines
        if a.ndim != 4 or a.shape[0] != B or a.shape[3] != N:
            raise ValueError("action_sequences must be (num_envs, K, H, num_turbines): K sequences of H joint actions per farm")
        if farms is not None:
            idx = np.ascontiguousarray(farms, dtype=np.int64).reshape(-1)
            if self.return_torch:
                import torch

                a = a[torch.from_numpy(idx).to(a.device)]
            else:
                a = a[idx]
        return self.fi.return_gradient(a, gamma=gamma, wind=wind, terminal=terminal, delta=delta, farms=farms, strict=strict,
                                       want=("returns", "rewards", "action_gradient", "reward_gradient", "state_gradient", "yaw",
                                             "pass_mask"))

    def plan_actions(self, horizon, candidates=64, elites=8, sigma=None, seed=0, gamma=1.0, wind=None, mean=None, farms=None,
                     strict=False, max_eval_farms=65536, want=("first_action", "plan_return")):
        """A receding-horizon plan for every farm from the state the env is in — call it BEFORE `step`, execute
        {"yaw": first_action}, shift "mean" by one step and pass it back as `mean`: the cross-entropy method over (horizon, N)
        action sequences on the device, one glue kernel between two evaluator steps (include/wfplan.h;
        backend.WfStep.plan_actions has the arguments; the project's own definition).  Returns the outputs `want` names —
        "plan", "plan_return", "hold_return", "first_action", "final_yaw", "mean" —, torch CUDA tensors when the env returns
        torch.  Continuous control only.  Run on a handle of its own: the env's yaw state, accumulators, wind and buffers
        are read, never changed.  On a time-series episode the wind of the coming steps is not the one the env holds:
        wind="series" reads the series' coming rows on the device (include/wfseries.h), or the caller passes them as
        wind=(n_farms, horizon, 2)."""
        series = isinstance(wind, str) and wind == "series"
        if series and not self._playing:
            raise ValueError('wind="series" needs a time-series episode: this env has no wind_time_series')
        if self._playing and wind is None:
            raise NotImplementedError("plan_actions on a time-series episode needs wind=(n_farms, horizon, 2): the series tick "
                                      "precedes the step, so the wind of the coming steps is not the one the env holds "
                                      '(or wind="series": the series\' coming rows, read on the device)')
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("plan_actions needs the plain reward (DoNothingReward): the return of a shaped reward is not "
                             "defined here")
        out = None
        if self.return_torch:
            import torch

            wind = wind if wind is None or series else self._to_device(wind).double()
            mean = None if mean is None else self._to_device(mean).float()
            want = (want,) if isinstance(want, str) else tuple(want)
            n = self.num_envs if farms is None else int(np.asarray(farms).size)
            H, N = int(horizon), self.num_turbines
            shapes = {"plan": ((n, H, N), torch.float32), "plan_return": ((n,), torch.float64), "hold_return": ((n,), torch.float64),
                      "first_action": ((n, N), torch.float32), "final_yaw": ((n, N), torch.float32), "mean": ((n, H, N), torch.float32)}
            if any(k not in shapes for k in want):
                raise ValueError("want must name plan, plan_return, hold_return, first_action, final_yaw and / or mean")
            out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=f"cuda:{self.fi.device_id}") for k in want}
        return self.fi.plan_actions(horizon, candidates=candidates, elites=elites, sigma=sigma, seed=seed, gamma=gamma, wind=wind,
                                    mean=mean, farms=farms, strict=strict, max_eval_farms=max_eval_farms, want=want, out=out)

    def plan_scenarios(self, horizon, candidates=64, elites=8, members=8, process=None, sigma=None, seed=0, scenario_seed=0,
                       gamma=1.0, tail=None, risk_weight=0.0, anchor=None, bounds=None, mean=None, farms=None, strict=False,
                       max_eval_farms=65536, want=("first_action", "plan_score")):
        """A receding-horizon plan under wind uncertainty for every farm from the state the env is in — call it BEFORE
        `step`, execute {"yaw": first_action}, shift "mean" by one step and pass it back as `mean`: plan_actions' search,
        every candidate scored as scenario_returns scores a sequence, over `members` wind futures drawn from the wind process
        (include/wfscenplan.h; backend.WfStep.plan_scenarios has the arguments; the project's own definition).  Returns the
        outputs `want` names — "plan", "plan_score", "plan_expected", "plan_cvar", "plan_member_returns", "hold_score",
        "first_action", "final_yaw", "mean", "wind_paths" —, torch CUDA tensors when the env returns torch.  process=None takes
        the env's wind_process and its distribution's speed bounds, as scenario_returns does; an env without wind_process must
        be given `process` (and may be given `bounds`, default 3 to 28 m/s).  Continuous control only.  Works on any episode
        kind (held wind, file series, generated): only the current wind is read.  Run on a handle of its own: the env's yaw
        state, accumulators, wind and buffers are read, never changed."""
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("plan_scenarios needs the plain reward (DoNothingReward): the return of a shaped reward is not "
                             "defined here")
        if process is None:
            if self._wind_process is None:
                raise ValueError("plan_scenarios needs a wind process: this env was built without wind_process, so pass "
                                 "process=dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=)")
            process = self._wind_process
            if bounds is None and self._wind_dist is not None:
                bounds = (float(self._wind_dist.get("ws_lo", 3.0)), float(self._wind_dist.get("ws_hi", 28.0)))
        if bounds is None:
            bounds = (3.0, 28.0)
        out = None
        if self.return_torch:
            import torch

            anchor = None if anchor is None else self._to_device(anchor).double()
            mean = None if mean is None else self._to_device(mean).float()
            want = (want,) if isinstance(want, str) else tuple(want)
            n = self.num_envs if farms is None else int(np.asarray(farms).size)
            H, M, N = int(horizon), int(members), self.num_turbines
            f32, f64 = torch.float32, torch.float64
            shapes = {"plan": ((n, H, N), f32), "plan_score": ((n,), f64), "plan_expected": ((n,), f64), "plan_cvar": ((n,), f64),
                      "plan_member_returns": ((n, M), f64), "hold_score": ((n,), f64), "first_action": ((n, N), f32),
                      "final_yaw": ((n, N), f32), "mean": ((n, H, N), f32), "wind_paths": ((n, M, H, 2), f64)}
            if any(k not in shapes for k in want):
                raise ValueError("want must name " + ", ".join(list(shapes)[:-1]) + " and / or wind_paths")
            if 1 <= H <= 64 and 1 <= M <= 64:  # (else the library refuses by name: nothing to allocate)
                out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=f"cuda:{self.fi.device_id}") for k in want}
        return self.fi.plan_scenarios(horizon, candidates=candidates, elites=elites, members=members, process=process, sigma=sigma,
                                      seed=seed, scenario_seed=scenario_seed, gamma=gamma, tail=tail, risk_weight=risk_weight,
                                      anchor=anchor, bounds=bounds, mean=mean, farms=farms, strict=strict,
                                      max_eval_farms=max_eval_farms, want=want, out=out)

    def controller_returns(self, controllers, horizon, gamma=1.0, wind=None, filter0=None, farms=None, strict=False,
                           max_eval_farms=65536, want=("returns", "best")):
        """What each of K look-up-table controllers — table slot, filter gain alpha, deadband, preview `lead` — earns over
        the next `horizon` steps under the env's own actuator, in closed loop, from the state the env is in: call it BEFORE
        `step`; the env state is read and never changed (include/wfrollout.h; backend.WfStep.controller_returns has the
        arguments and WfStep.controller_grid builds a tuning grid; the project's own definition).  Returns the outputs
        `want` names — "returns", "rewards", "farm_power", "actions", "final_yaw", "gated", "filter_final", "best" —, torch
        CUDA tensors when the env returns torch.  controllers alpha 1, deadband 0, lead 0 is what stepping with
        `lut_action()` does; {"yaw": actions[:, k, h]} is what to give `step` to replay controller k.  The tables are those
        of `self.fi.set_yaw_table`.  Run on a handle of its own: the env's yaw state, accumulators, wind and buffers are
        read, never changed.  On a time-series episode the wind of the coming steps is not the one the env holds:
        wind="series" reads the series' coming rows on the device (include/wfseries.h), or the caller passes them as
        wind=(n_farms, horizon, 2)."""
        series = isinstance(wind, str) and wind == "series"
        if series and not self._playing:
            raise ValueError('wind="series" needs a time-series episode: this env has no wind_time_series')
        if self._playing and wind is None:
            raise NotImplementedError("controller_returns on a time-series episode needs wind=(n_farms, horizon, 2): the series "
                                      "tick precedes the step, so the wind of the coming steps is not the one the env holds "
                                      '(or wind="series": the series\' coming rows, read on the device)')
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("controller_returns needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        out = None
        if self.return_torch:
            import torch

            wind = wind if wind is None or series else self._to_device(wind).double()
            filter0 = None if filter0 is None else self._to_device(filter0).double()
            want = (want,) if isinstance(want, str) else tuple(want)
            n = self.num_envs if farms is None else int(np.asarray(farms).size)
            K, H, N = self.fi._rollout()._controllers(controllers)[1], int(horizon), self.num_turbines
            shapes = {"returns": ((n, K), torch.float64), "rewards": ((n, K, H), torch.float64), "farm_power": ((n, K, H), torch.float64),
                      "actions": ((n, K, H, N), torch.float32), "final_yaw": ((n, K, N), torch.float32), "gated": ((n, K), torch.int32),
                      "filter_final": ((n, K, 2), torch.float64), "best": ((n,), torch.int32)}
            if any(k not in shapes for k in want):
                raise ValueError("want must name returns, rewards, farm_power, actions, final_yaw, gated, filter_final and / or best")
            if 1 <= H and 1 <= K and K * H <= 4096:  # (a refused shape sizes nothing: the library names the limit)
                out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=f"cuda:{self.fi.device_id}") for k in want}
        return self.fi.controller_returns(controllers, horizon, gamma=gamma, wind=wind, filter0=filter0, farms=farms, strict=strict,
                                          max_eval_farms=max_eval_farms, want=want, out=out)

    def controller_scenarios(self, controllers, horizon, members=8, process=None, seed=0, gamma=1.0, tail=None, risk_weight=0.0,
                             anchor=None, bounds=None, filter0=None, farms=None, strict=False, max_eval_farms=65536,
                             want=("expected_returns", "cvar", "score", "best")):
        """What each of K look-up-table controllers earns over the next `horizon` steps in closed loop under each of `members`
        wind futures drawn from the wind process, from the state the env is in — call it BEFORE `step`: per controller the
        mean over the members ("expected_returns"), the tail mean of the `tail` lowest member returns ("cvar"),
        score = (1 - risk_weight) mean + risk_weight cvar, and "best", the controller of the largest score; `want` may also
        name "member_returns", "rewards", "wind_paths", "actions", "final_yaw", "gated" and "first_action" — {"yaw":
        first_action[farm, best[farm]]} is what a receding-horizon selector gives `step` (include/wfrollscen.h;
        backend.WfStep.controller_scenarios has the arguments and WfStep.controller_grid builds a tuning grid; the project's
        own definition).  process=None takes the env's wind_process and its distribution's speed bounds, exactly as
        scenario_returns does; an env without wind_process must be given `process` (and may be given `bounds`, default 3 to
        28 m/s).  The tables are those of `self.fi.set_yaw_table`.  Works on any episode kind (held wind, file series,
        generated): only the current wind is read.  Run on a handle of its own: the env's yaw state, accumulators, wind
        and buffers are read, never changed."""
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("controller_scenarios needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        if process is None:
            if self._wind_process is None:
                raise ValueError("controller_scenarios needs a wind process: this env was built without wind_process, so pass "
                                 "process=dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=)")
            process = self._wind_process
            if bounds is None and self._wind_dist is not None:
                bounds = (float(self._wind_dist.get("ws_lo", 3.0)), float(self._wind_dist.get("ws_hi", 28.0)))
        if bounds is None:
            bounds = (3.0, 28.0)
        out = None
        if self.return_torch:
            import torch

            anchor = None if anchor is None else self._to_device(anchor).double()
            filter0 = None if filter0 is None else self._to_device(filter0).double()
            want = (want,) if isinstance(want, str) else tuple(want)
            n = self.num_envs if farms is None else int(np.asarray(farms).size)
            K, H, M, N = self.fi._rollscen()._controllers(controllers)[1], int(horizon), int(members), self.num_turbines
            f32, f64, i32 = torch.float32, torch.float64, torch.int32
            shapes = {"expected_returns": ((n, K), f64), "cvar": ((n, K), f64), "score": ((n, K), f64), "member_returns": ((n, K, M), f64),
                      "rewards": ((n, K, M, H), f64), "wind_paths": ((n, M, H, 2), f64), "actions": ((n, K, M, H, N), f32),
                      "final_yaw": ((n, K, M, N), f32), "gated": ((n, K, M), i32), "first_action": ((n, K, N), f32), "best": ((n,), i32)}
            if any(k not in shapes for k in want):
                raise ValueError("want must name " + ", ".join(list(shapes)[:-1]) + " and / or best")
            if 1 <= K <= 64 and 1 <= M <= 64 and 1 <= H <= 64 and K * M * H <= 4096:  # (else the library refuses by name)
                out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=f"cuda:{self.fi.device_id}") for k in want}
        return self.fi.controller_scenarios(controllers, horizon, members, process, seed=seed, gamma=gamma, tail=tail,
                                            risk_weight=risk_weight, anchor=anchor, bounds=bounds, filter0=filter0, farms=farms,
                                            strict=strict, max_eval_farms=max_eval_farms, want=want, out=out)

    def policy_returns(self, policy, horizon, gamma=1.0, wind=None, farms=None, strict=False, max_eval_farms=65536,
                       want=("returns", "best"), kind=None, out_scale=1.0, shift=None, scale=None, use_freewind=False):
        """What each of K MLP policies earns over the next `horizon` steps under the env's own actuator, in closed loop —
        the network observing yaw, local wind and free wind after every step —, from the state the env is in: call it BEFORE
        `step`; the env state is read and never changed (include/wfpolicy.h; backend.WfStep.policy_returns has the
        arguments; the project's own definition).  `policy` is (params (K, P), spec) as policy.policy_from_torch returns
        them, or an nn.Sequential (or a list of K of one architecture) of Linear / ReLU / Tanh / Softsign, converted with
        `kind` ("central" / "shared"), out_scale, shift, scale and use_freewind (policy.policy_from_torch).  Returns the
        outputs `want` names — "returns", "rewards", "farm_power", "actions", "observations", "final_yaw", "gated", "best" —,
        torch CUDA tensors when the env returns torch; {"yaw": actions[:, k, h]} is what to give `step` to replay policy k.
        One batched step per env step, K rows per farm, nothing read back in between.  On a time-series or generated episode
        the wind of the coming steps is not the one the env holds: wind="series" passes the series' coming rows
        (`wind_preview(horizon)`), or the caller passes wind=(n_farms, horizon, 2) itself."""
        from . import policy as P

        series = isinstance(wind, str) and wind == "series"
        if series and not self._playing:
            raise ValueError('wind="series" needs a time-series episode: this env has no wind_time_series')
        if self._playing and wind is None:
            raise NotImplementedError("policy_returns on a time-series episode needs wind=(n_farms, horizon, 2): the series "
                                      "tick precedes the step, so the wind of the coming steps is not the one the env holds "
                                      '(or wind="series": the series\' coming rows)')
        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("policy_returns needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        if isinstance(policy, tuple) and len(policy) == 2 and isinstance(policy[1], dict):
            params, spec = policy
        else:
            if kind is None:
                raise ValueError('a torch module needs kind="central" or kind="shared"')
            params, spec = P.policy_from_torch(policy, kind, out_scale=out_scale, shift=shift, scale=scale, use_freewind=use_freewind)
        if series:
            wind = self.fi.wind_preview(int(horizon), first=1, farms=farms, as_torch=self.return_torch)[0]
        if self.return_torch:
            import torch

            params = self._to_device(params)
            if wind is not None:  # (float64 all the way: the rows' wind is not rounded to float32)
                dev = f"cuda:{self.fi.device_id}"
                wind = wind.to(device=dev, dtype=torch.float64) if isinstance(wind, torch.Tensor) else torch.as_tensor(np.asarray(wind, np.float64), device=dev)
        return self.fi.policy_returns(params, spec, horizon, gamma=gamma, wind=wind, farms=farms, strict=strict,
                                      max_eval_farms=max_eval_farms, want=want)

    def policy_scenarios(self, policy, horizon, members=8, process=None, seed=0, gamma=1.0, tail=None, risk_weight=0.0, anchor=None,
                         bounds=None, farms=None, strict=False, max_eval_farms=65536,
                         want=("expected_returns", "cvar", "score", "best"), kind=None, out_scale=1.0, shift=None, scale=None,
                         use_freewind=False):
        """What each of K MLP policies earns over the next `horizon` steps in closed loop under each of `members` wind futures
        drawn from the wind process, from the state the env is in — call it BEFORE `step`: per policy the mean over the
        members ("expected_returns"), the tail mean of the `tail` lowest member returns ("cvar"), score = (1 - risk_weight)
        mean + risk_weight cvar, and "best", the policy of the largest score; `want` may also name "member_returns",
        "rewards", "farm_power", "wind_paths", "actions", "observations", "final_yaw", "gated" and "first_action"
        (include/wfpolscen.h; backend.WfStep.policy_scenarios has the arguments; the project's own definition).  `policy` is
        taken as policy_returns takes it: (params (K, P), spec), an nn.Sequential or a list of K of one architecture, with
        `kind`, out_scale, shift, scale and use_freewind.  process=None takes the env's wind_process and its distribution's
        speed bounds, exactly as controller_scenarios does; an env without wind_process must be given `process` (and may be
        given `bounds`, default 3 to 28 m/s).  {"yaw": actions[:, k, m, h]} is what to give `step` to replay policy k under
        member m.  Works on any episode kind (held wind, file series, generated): only the current wind is read.  Returns
        torch CUDA tensors when the env returns torch; the env's yaw state, accumulators, wind and buffers are read, never
        changed."""
        from . import policy as P

        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("policy_scenarios needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        if process is None:
            if self._wind_process is None:
                raise ValueError("policy_scenarios needs a wind process: this env was built without wind_process, so pass "
                                 "process=dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=)")
            process = self._wind_process
            if bounds is None and self._wind_dist is not None:
                bounds = (float(self._wind_dist.get("ws_lo", 3.0)), float(self._wind_dist.get("ws_hi", 28.0)))
        if bounds is None:
            bounds = (3.0, 28.0)
        if isinstance(policy, tuple) and len(policy) == 2 and isinstance(policy[1], dict):
            params, spec = policy
        else:
            if kind is None:
                raise ValueError('a torch module needs kind="central" or kind="shared"')
            params, spec = P.policy_from_torch(policy, kind, out_scale=out_scale, shift=shift, scale=scale, use_freewind=use_freewind)
        if self.return_torch:
            params = self._to_device(params)
            anchor = None if anchor is None else self._to_device(anchor).double()
        return self.fi.policy_scenarios(params, spec, horizon, members, process, seed=seed, gamma=gamma, tail=tail,
                                        risk_weight=risk_weight, anchor=anchor, bounds=bounds, farms=farms, strict=strict,
                                        max_eval_farms=max_eval_farms, want=want)

    def search_policy(self, policy, horizon, sigma=0.5, candidates=32, elites=8, iterations=4, sigma_min=0.0, seed=0, gamma=1.0,
                      wind=None, members=None, process=None, scenario_seed=0, tail=None, risk_weight=0.0, anchor=None, bounds=None,
                      farms=None, strict=False, max_eval_farms=65536,
                      want=("best_params", "best_fitness", "init_fitness", "mean", "sigma"), kind=None, out_scale=1.0, shift=None,
                      scale=None, use_freewind=False):
        """A cross-entropy search over the weights of one MLP policy from the state the env is in, in one call and on the
        device — call it BEFORE `step`; the env state is read and never changed (include/wfpolsearch.h;
        backend.WfStep.search_policy has the arguments; the project's own definition).  `policy` is taken as policy_returns
        takes it — (params, spec) with ONE parameter vector, the start, or an nn.Sequential converted with `kind`, out_scale,
        shift, scale and use_freewind (policy.policy_from_torch).  The fitness of a candidate is the mean over the listed farms
        of policy_returns' return — wind as policy_returns takes it, "series" included —, or with `members` of
        policy_scenarios' score under the env's wind_process and speed bounds (or `process`, `bounds`).  Returns the outputs
        `want` names, torch CUDA tensors when the env returns torch; "mean" and "sigma" fed back as policy=(mean, spec) and
        sigma= warm-start the next call."""
        from . import policy as P

        if type(self.reward_shaper).__name__ != "DoNothingReward":
            raise ValueError("search_policy needs the plain reward (DoNothingReward): the return of a shaped reward is "
                             "not defined here")
        series = isinstance(wind, str) and wind == "series"
        if members is None:
            if series and not self._playing:
                raise ValueError('wind="series" needs a time-series episode: this env has no wind_time_series')
            if self._playing and wind is None:
                raise NotImplementedError("search_policy on a time-series episode needs wind=(n_farms, horizon, 2): the series "
                                          "tick precedes the step, so the wind of the coming steps is not the one the env holds "
                                          '(or wind="series": the series\' coming rows), or members= for a wind ensemble')
        else:
            if process is None:
                if self._wind_process is None:
                    raise ValueError("search_policy with members needs a wind process: this env was built without wind_process, "
                                     "so pass process=dict(ws_revert=, ws_sigma=, wd_revert=, wd_sigma=, wd_ramp=)")
                process = self._wind_process
                if bounds is None and self._wind_dist is not None:
                    bounds = (float(self._wind_dist.get("ws_lo", 3.0)), float(self._wind_dist.get("ws_hi", 28.0)))
        if bounds is None:
            bounds = (3.0, 28.0)
        if isinstance(policy, tuple) and len(policy) == 2 and isinstance(policy[1], dict):
            params, spec = policy
        else:
            if kind is None:
                raise ValueError('a torch module needs kind="central" or kind="shared"')
            params, spec = P.policy_from_torch(policy, kind, out_scale=out_scale, shift=shift, scale=scale, use_freewind=use_freewind)
        if len(tuple(params.shape)) == 2 and int(params.shape[0]) == 1:
            params = params[0]
        if len(tuple(params.shape)) != 1:
            raise ValueError("search_policy starts from ONE parameter vector (P,): pass one policy")
        if series and members is None:
            wind = self.fi.wind_preview(int(horizon), first=1, farms=farms, as_torch=self.return_torch)[0]
        if self.return_torch:
            import torch

            dev = f"cuda:{self.fi.device_id}"
            params = self._to_device(params)
            anchor = None if anchor is None else self._to_device(anchor).double()
            if wind is not None:  # (float64 all the way: the rows' wind is not rounded to float32)
                wind = wind.to(device=dev, dtype=torch.float64) if isinstance(wind, torch.Tensor) else torch.as_tensor(np.asarray(wind, np.float64), device=dev)
        return self.fi.search_policy(params, spec, horizon, sigma=sigma, candidates=candidates, elites=elites, iterations=iterations,
                                     sigma_min=sigma_min, seed=seed, gamma=gamma, wind=wind, members=members, process=process,
                                     scenario_seed=scenario_seed, tail=tail, risk_weight=risk_weight, anchor=anchor, bounds=bounds,
                                     farms=farms, strict=strict, max_eval_farms=max_eval_farms, want=want)

    def _series_keyword(self, name, wind, steps):
        """The wind keyword of counterfactual_rewards / lookahead_returns: None or "series"; a time-series episode needs
        "series", any other episode None."""
        if wind is not None and not (isinstance(wind, str) and wind == "series"):
            raise ValueError(f'{name}: wind must be None or "series"')
        if self._playing and wind is None:
            raise NotImplementedError(f"{name} is not supported on a time-series episode: the series tick precedes the step, so "
                                      f"the wind of the coming {steps} is not the one the env holds (pass wind=\"series\": the "
                                      "series' coming rows, read on the device)")
        if not self._playing and wind is not None:
            raise ValueError(f'{name}: wind="series" needs a time-series episode: this env has no wind_time_series')

    def wind_preview(self, H: int):
        """The free wind the env will observe over its next H steps, on a time-series episode: ((num_envs, H, 2) float64
        [speed, direction], available) — entry h is what `freewind_measurements` will hold after step h + 1 from here; only
        the first `available` entries are real, the rest hold the series' last wind (the step that would follow it fails
        with "exhausted").  A torch CUDA tensor when the env returns torch: one kernel launch, nothing read back
        (include/wfseries.h; backend.WfStep.wind_preview).  What a feed-forward or preview controller observes."""
        if not self._playing:
            raise ValueError("wind_preview needs a time-series episode: this env has no wind_time_series")
        return self.fi.wind_preview(H, first=1, as_torch=self.return_torch)

    def lut_target_yaw(self, table_slot: int = 0):
        """The yaw (num_envs, N) the look-up table in `table_slot` (backend.WfStep.set_yaw_table on `self.fi`) holds for
        every farm's CURRENT wind, clipped to the env's yaw bounds — a torch CUDA tensor when the env returns torch.  The
        wind is read on the device; the env state is not changed.  The project's own interpolation (include/wfrose.h)."""
        return self.fi.lut_policy(table_slot, want=("target_yaw",), as_torch=self.return_torch)["target_yaw"]

    def lut_action(self, table_slot: int = 0) -> dict:
        """The industry-baseline controller as a policy: {"yaw": action} ready for `step` — the action that moves every
        turbine from the env's current yaw towards `lut_target_yaw` under the env's control (continuous: the difference
        clipped to +-step; discrete: 0 / 1 / 2 = down / hold / up, hold inside half a step).  Reads the env state, never
        changes it; a torch CUDA tensor when the env returns torch, computed without a host round trip."""
        return {"yaw": self.fi.lut_policy(table_slot, want=("action",), as_torch=self.return_torch)["action"]}

    # -- checkpoint / resume (the env state is tiny; FLORIS itself is stateless between steps) ------
    def get_state(self) -> dict:
        """Everything needed to resume the batch: device env state, the per-farm wind, the step counter."""
        ws, wd = self.fi.get_wind()
        st = {**self.fi.env_get_state(), "wind_speed": ws, "wind_direction": wd, "num_iter": self._num_iter,
              "shaper_ref": None if self._shaper_ref is None else np.asarray(
                  self._shaper_ref.cpu() if hasattr(self._shaper_ref, "cpu") else self._shaper_ref).copy()}
        if self._model_rand is not None:  # wake-model parameter sets per farm and their assignment
            sets, set_of = self.fi.model_sets()
            st["model_sets"] = {"sets": sets, "set_of": set_of}
        if self._series is not None:  # a time-series episode: one cursor per farm (include/wfseries.h)
            cur = self.fi.series_state()
            st.update(series_t=cur["t"], series_start=cur["start"], series_prev_pending=cur["prev_pending"])
        if self._wind_process is not None:  # a generated episode: what generates the same series again, and the cursor
            if self._generated is None:
                raise ValueError("get_state: the env has not been reset")
            cur = self.fi.series_state()
            st["generated_wind"] = {**self._generated, "process": dict(self._wind_process),
                                    "dist": None if self._wind_dist is None else dict(self._wind_dist),
                                    "t": cur["t"], "prev_pending": cur["prev_pending"]}
        return st

    def set_state(self, state: dict):
        if ("series_t" in state) != (self._series is not None):
            raise ValueError("the state of a time-series episode resumes on an env with that wind_time_series, and only there: "
                             + ("this env has none" if self._series is None else "this state holds no series cursor"))
        if ("generated_wind" in state) != (self._wind_process is not None):
            raise ValueError("the state of a generated wind episode resumes on an env with a wind_process, and only there: "
                             + ("this env has none" if self._wind_process is None else "this state holds no generated wind"))
        if ("model_sets" in state) != (self._model_rand is not None):
            raise ValueError("the state of an env with model_randomization resumes on an env with model_randomization, and only there")
        if self._model_rand is not None:  # (before the env state: the sets do not touch it, and the next step needs them)
            self.fi.set_model_sets(state["model_sets"]["sets"], state["model_sets"]["set_of"])
        if self._wind_process is not None:
            # the same seed, distribution, process and tick 0 give the same bits; then the cursor
            g = state["generated_wind"]
            self._generated = {k: g[k] for k in ("seed", "T", "ws0", "wd0")}
            self.fi.generate_wind(g["T"], g["seed"], g["process"], dist=g["dist"], ws0=g["ws0"], wd0=g["wd0"])
            self.fi.series_seek(g["t"], g["prev_pending"])
        elif self._series is not None:
            # the env's own series with the state's start rows, then the cursor: the wind is the series' row again
            self.fi.set_wind_series(self._series, start=state["series_start"])
            self.fi.series_seek(state["series_t"], state["series_prev_pending"])
        else:
            self.fi.set_wind(state["wind_speed"], state["wind_direction"])
        self.fi.env_set_state(state)
        self._num_iter = int(state["num_iter"])
        ref = state.get("shaper_ref")
        self._shaper_ref = None if ref is None else self._to_device(ref)
        self._refresh_freewind()

    def close(self):
        self.fi.close()


def make_vec(env_id: str, env_batch: int, controls=("yaw",), **kw):
    """`make(env_id, env_batch=B)` shortcut."""
    from .environments import make

    return make(env_id, controls=list(controls) if not isinstance(controls, dict) else controls, env_batch=env_batch,
                **kw)
