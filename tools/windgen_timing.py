"""Times synthetic wind episodes (include/wfwindgen.h) on one GPU and writes profiles/windgen_timing.json.

Per workload (Ablaincourt x 4096, HornsRev1 x 65536; T = 502 ticks = an episode of 500 steps):
  generate       WfStep.generate_wind — the reset draw into row 0, the generating kernel over T - 1 ticks (the library's
                 choice, and each of the two kernels forced), tick 0 into the parent (one geometry pass) — beside
                 WfStep.sample_wind, the reset draw with the same geometry pass
  reset          VecWindFarmEnv.reset() with wind_process= beside the same env with wind_sampling="device" (a wind held from
                 reset to truncation: the code of the commit before this extension, unchanged by it)
  step           one tick + one fused env step of a generated episode beside the same of a file-series episode forced onto
                 the path with a geometry per farm (kernel_choice pair_table=False on both handles): the same work — wind
                 in, geometry, step.  The step's cost depends on the winds, so the generated episode starts from the file
                 series' rows at random starts and wanders little (STEP_PROCESS): both batches see one distribution
Wall-clock milliseconds around the call and a stream synchronisation, host work included; 2 warm-up rounds, then ROUNDS
rounds with the variants alternating; median / min / max / spread (max - min) of the rounds.  `comparison` states every
difference beside the larger of the two spreads.

  python tools/windgen_timing.py [rounds [out.json]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 502
PROCESS = dict(ws_revert=0.05, ws_sigma=0.25, wd_revert=0.05, wd_sigma=1.5, wd_ramp=0.5)
STEP_PROCESS = dict(ws_revert=0.05, ws_sigma=0.05, wd_revert=0.05, wd_sigma=0.3, wd_ramp=0.0)  # stays near tick 0
WORKLOADS = (("Ablaincourt_Floris", 4096, 50), ("HornsRev1_Floris", 65536, 10))  # env id, farms, steps per round


def _stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def _timed(f, sync):
    sync()
    t0 = time.perf_counter()
    f()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _file_series(rows):
    k = np.arange(rows)
    return np.stack([8.0 + 1.5 * np.sin(0.05 * k), (270.0 + 20.0 * np.sin(0.013 * k) + 0.05 * k) % 360.0], axis=1)


def workload(env_id, B, steps, rounds):
    import torch
    from wfcrl_env_amd import environments as envs
    from wfcrl_env_amd.backend import WfStep

    out = {"env": env_id, "farms": B, "T": T, "steps_per_round": steps, "rounds": rounds}
    kw = dict(env_batch=B, max_num_steps=500)
    plain = envs.make(env_id, wind_sampling="device", **kw)
    synth = envs.make(env_id, wind_process=PROCESS, **kw)
    N = plain.num_turbines
    x, y = plain.farm_case.simul_params["xcoords"], plain.farm_case.simul_params["ycoords"]
    sync = torch.cuda.synchronize
    # generate beside the reset draw, reset beside reset
    gen, gen_serial, gen_tiled, draw, r_synth, r_plain = [], [], [], [], [], []
    w = synth.fi
    for i in range(rounds + 2):
        a0 = _timed(lambda: w.generate_wind(T, 100 + i, PROCESS, kernel="serial"), sync)
        a1 = _timed(lambda: w.generate_wind(T, 100 + i, PROCESS, kernel="tiled"), sync)
        a = _timed(lambda: w.generate_wind(T, 100 + i, PROCESS), sync)
        b = _timed(lambda: plain.fi.sample_wind(100 + i), sync)
        c = _timed(lambda: synth.reset(seed=i), sync)
        d = _timed(lambda: plain.reset(seed=i), sync)
        if i >= 2:
            gen.append(a); gen_serial.append(a0); gen_tiled.append(a1); draw.append(b); r_synth.append(c); r_plain.append(d)
    out["generate_ms"], out["sample_wind_ms"] = _stats(gen), _stats(draw)
    out["generate_serial_kernel_ms"], out["generate_tiled_kernel_ms"] = _stats(gen_serial), _stats(gen_tiled)
    out["reset_wind_process_ms"], out["reset_device_sampling_ms"] = _stats(r_synth), _stats(r_plain)
    out["series_bytes"] = 16 * T * B
    out["kernels"] = w.windgen_kernel_info()
    plain.close()
    # a step of a generated episode beside a step of a file-series episode on the per-farm path
    synth.close()
    choice = dict(pair_table=False)  # (both handles alike: a generated episode has a geometry per farm anyway)
    series, w = WfStep(x, y, env_batch=B, kernel_choice=choice), WfStep(x, y, env_batch=B, kernel_choice=choice)
    series.env_config(load_coef=0.1)
    w.env_config(load_coef=0.1)
    rows = _file_series(T)
    act = (torch.rand((B, N), device="cuda") * 10.0 - 5.0).float()
    want = ("reward", "yaw", "wind_speed", "wind_direction")

    def start(h, generated, seed):
        if generated:  # tick 0 = the file series' rows at random starts: both batches see winds of one distribution
            st = np.random.default_rng(seed).integers(0, T, B)
            h.generate_wind(T, seed, STEP_PROCESS, ws0=rows[st, 0], wd0=rows[st, 1])
        else:
            h.set_wind_series(rows, seed=seed)
        h.env_reset()
        h.wind_series_step()
        h.env_step(None, want=("yaw",))

    def run(h):
        for _ in range(steps):
            h.wind_series_step()
            h.env_step(act, want=want)

    g_ms, s_ms = [], []
    for i in range(rounds + 2):
        for h, generated, acc in ((w, True, g_ms), (series, False, s_ms)):
            start(h, generated, i)
            ms = _timed(lambda: run(h), sync) / steps
            if i >= 2:
                acc.append(ms)
    out["step_generated_ms"], out["step_file_series_ms"] = _stats(g_ms), _stats(s_ms)
    out["direction_groups"] = {"generated": w.kernel_info()["direction_groups"], "file_series": series.kernel_info()["direction_groups"]}
    series.close()
    w.close()
    g, s = out["step_generated_ms"], out["step_file_series_ms"]
    out["comparison"] = {
        "generate_over_reset_device_sampling": out["generate_ms"]["median"] / out["reset_device_sampling_ms"]["median"],
        "generate_exceeds_that_reset": out["generate_ms"]["median"] > out["reset_device_sampling_ms"]["median"],
        "reset_difference_ms": out["reset_wind_process_ms"]["median"] - out["reset_device_sampling_ms"]["median"],
        "step_difference_ms": g["median"] - s["median"],
        "step_spread_ms": max(g["spread"], s["spread"]),
        "step_difference_within_spread": abs(g["median"] - s["median"]) <= max(g["spread"], s["spread"]),
    }
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    import torch

    result = {"tool": "tools/windgen_timing.py", "device": torch.cuda.get_device_name(0), "process": PROCESS, "step_process": STEP_PROCESS,
              "clock": "wall clock around the call and a stream synchronisation, host work included",
              "workloads": [workload(e, b, s, rounds) for e, b, s in WORKLOADS]}
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "windgen_timing.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["workloads"], indent=1))


if __name__ == "__main__":
    main()
