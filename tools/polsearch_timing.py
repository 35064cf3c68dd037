"""Policy search on the device (csrc/polsearch/, include/wfpolsearch.h): what a cross-entropy search over the weights of one
MLP policy costs in one call, next to the rollouts it is made of and next to the two ways a user had to write it before.
Writes profiles/polsearch_timing.json.

One MI355X, HIP events on the handle's stream, measured as tools/policy_timing.py measures, on its parent (a fused env after
three random env steps, a wind per farm held over the horizon, continuous control, gamma 0.95, tanh networks), I = 4 iterations,
E = K / 4 elites, sigma 0.3, sigma_min 0.01, default mode:
    HornsRev1 x 256 farms, K = 8 and K = 64, H = 16, central 242-64-64-80
    Ablaincourt x 4096 farms, K = 16, H = 16, shared 3-32-32-1
Per configuration, after 2 warm-up rounds, medians of `reps` rounds in which the four ways alternate:
    search_ms      (a) search_policy — torch tensors in and out —, two events per run; scorer_ms / own_ms: `reps` more runs with
                   the events split per launch: the scorer's runs and this extension's own kernels
    floor_ms       (b) I bare policy_returns calls on fixed device-resident parameters
    numpy_way_ms   (c) the hand-written way: per iteration NumPy draws on the host, upload, policy_returns, download, the mean over
                   the farms, argsort / mean / std in NumPy
    torch_way_ms   (d) the same with torch draws and mean / topk / mean / std on the device, nothing read back
    own_cost_ms = (a) - (b);  ratios (a) / (c), (a) / (d)
The ways draw different numbers (Philox on the device, NumPy's and torch's generators), so they search different populations:
only their cost is compared.
Run from the repo root on an MI355X:  python tools/polsearch_timing.py [reps, default 5] [output file]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.policy_timing import ENV, GAMMA, LAYOUTS, network  # noqa: E402
from wfcrl_env_amd.backend import WfStep  # noqa: E402

assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "polsearch_timing.json")
I, SIGMA, SIGMA_MIN = 4, 0.3, 0.01


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def workload(label, name, B, kind, widths, K, H):
    lay = LAYOUTS[name]
    x, y = np.asarray(lay["xcoords"], float), np.asarray(lay["ycoords"], float)
    N = len(x)
    rng = np.random.default_rng(7)
    params, spec = network(kind, widths, N, K, rng)
    P, E = int(params.shape[1]), max(1, K // 4)
    w = WfStep(x, y, env_batch=B)
    w.set_wind(rng.uniform(6.0, 12.0, B), rng.uniform(255.0, 285.0, B))
    w.env_config(**ENV)
    w.env_reset()
    for _ in range(3):
        w.env_step(torch.from_numpy(rng.uniform(-5.0, 5.0, (B, N)).astype(np.float32)).cuda(), want=("reward",))
    par_t = torch.from_numpy(params).cuda()
    mean_t, sigma_t = par_t[0].clone(), torch.full((P,), SIGMA, dtype=torch.float32, device="cuda")
    ret = {"returns": torch.empty((B, K), dtype=torch.float64, device="cuda")}
    out = {"best_params": torch.empty(P, dtype=torch.float32, device="cuda"), "best_fitness": torch.empty((), dtype=torch.float64, device="cuda"),
           "init_fitness": torch.empty((), dtype=torch.float64, device="cuda"), "mean": torch.empty(P, dtype=torch.float32, device="cuda"),
           "sigma": torch.empty(P, dtype=torch.float32, device="cuda")}

    def search():
        w.search_policy(mean_t, spec, H, sigma=sigma_t, candidates=K, elites=E, iterations=I, sigma_min=SIGMA_MIN, seed=1, gamma=GAMMA,
                        want=tuple(out), out=out)

    def floor():
        for _ in range(I):
            w.policy_returns(par_t, spec, H, gamma=GAMMA, want=("returns",), out=ret)

    def numpy_way():
        g = np.random.default_rng(1)
        mean, sigma = params[0].astype(np.float64), np.full(P, SIGMA)
        for _ in range(I):
            cand = mean + sigma * g.standard_normal((K, P))
            cand[0] = mean
            r = w.policy_returns(torch.from_numpy(cand.astype(np.float32)).cuda(), spec, H, gamma=GAMMA, want=("returns",), out=ret)
            fit = r["returns"].cpu().numpy().mean(axis=0)
            order = np.argsort(-fit)[:E]
            mean, sigma = cand[order].mean(axis=0), cand[order].std(axis=0) + SIGMA_MIN

    def torch_way():
        g = torch.Generator(device="cuda").manual_seed(1)
        mean, sigma = mean_t.clone(), sigma_t.clone()
        for _ in range(I):
            cand = mean + sigma * torch.randn((K, P), generator=g, device="cuda")
            cand[0] = mean
            r = w.policy_returns(cand, spec, H, gamma=GAMMA, want=("returns",), out=ret)
            elite = cand[torch.topk(r["returns"].mean(dim=0), E).indices]
            mean, sigma = elite.mean(dim=0), elite.std(dim=0, unbiased=False) + SIGMA_MIN

    ways = {"search_ms": search, "floor_ms": floor, "numpy_way_ms": numpy_way, "torch_way_ms": torch_way}
    for _ in range(2):
        for fn in ways.values():
            timed(fn)
    ms = {k: [] for k in ways}
    call = []
    for _ in range(REPS):  # alternating: they share whatever else the machine is doing
        for k, fn in ways.items():
            t = timed(fn)
            if k == "search_ms":  # the library's own two events beside the caller's: the wrapper's host time shows in the difference
                call.append(t)
                t = w.search_policy_timing()["total_ms"]
            ms[k].append(t)
    w.search_policy_timing(detail=True)
    det = []
    for _ in range(REPS):
        search()
        det.append(w.search_policy_timing())
    w.search_policy_timing(detail=False)
    torch.cuda.synchronize()
    fitness = {"init_fitness": float(out["init_fitness"].item()), "best_fitness": float(out["best_fitness"].item())}
    kernels = w.search_policy_kernel_info()
    w.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = {"workload": label, "layout": name, "turbines": N, "farms": B, "candidates": K, "elites": E, "iterations": I, "horizon": H,
         "gamma": GAMMA, "kind": kind, "widths": list(widths), "parameters": P, "mode": "default", "wind": "per farm, held", "reps": REPS}
    r.update(med)
    r.update({k + "_min": float(np.min(v)) for k, v in ms.items()})
    r.update({k + "_max": float(np.max(v)) for k, v in ms.items()})
    r.update({"search_call_ms": float(np.median(call)),
              "scorer_ms": float(np.median([d["step_ms"] for d in det])), "own_ms": float(np.median([d["glue_ms"] for d in det])),
              "search_detail_ms": float(np.median([d["total_ms"] for d in det])),
              "own_cost_ms": med["search_ms"] - med["floor_ms"], "one_rollout_ms": med["floor_ms"] / I,
              "ratio_search_over_numpy_way": med["search_ms"] / med["numpy_way_ms"],
              "ratio_search_over_torch_way": med["search_ms"] / med["torch_way_ms"],
              "search_loses_to_torch_way_beyond_spread": bool(min(ms["search_ms"]) > max(ms["torch_way_ms"])),
              "results": fitness, "kernels": kernels})
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    res = [workload("HornsRev1 x 256, K = 8, I = 4, H = 16, central 242-64-64-80, default mode", "HornsRev1_", 256, "central", (242, 64, 64, 80), 8, 16),
           workload("Ablaincourt x 4096, K = 16, I = 4, H = 16, shared 3-32-32-1, default mode", "Ablaincourt_", 4096, "shared", (3, 32, 32, 1), 16, 16),
           workload("HornsRev1 x 256, K = 64, I = 4, H = 16, central 242-64-64-80, default mode", "HornsRev1_", 256, "central", (242, 64, 64, 80), 64, 16)]
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the handle's stream; 2 warm-up rounds, median of `reps`; "
                   "the search, the bare rollouts, the NumPy way and the torch way alternate", "workloads": res}, f, indent=1)
        f.write("\n")
