"""GPU: the timing contract of the two yaw searches (include/wfyawopt.h, include/wfrobust.h: *_set_timing, *_last_timing).

Both searches are enqueued by one driver (csrc/ext/wf_ext.h: run_search), which records the events `timing()` reads: without
detail the run's first and last event only, with detail an event after every glue launch and every wf_step, per chunk.  The
input is the smallest that has every kind of interval: the row of three, four farms with a wind each, one pass of three
candidates (V = 3 visits, R = 4 rows), and an evaluator that holds two farms' rows, so the run has two chunks and one empty
interval at the chunk boundary (counted as glue).  Strict mode: the bits do not depend on the kernel family."""
import re

import numpy as np
import pytest

import yawopt_ref

pytestmark = pytest.mark.gpu

# search -> (optimize_yaw's arguments beyond the common ones, the wrapper's getter, what timing() says before any run)
SEARCHES = {
    "yawopt": (dict(max_eval_farms=8), "_yawopt", "wf_yawopt_run has not run yet"),  # R = 4: C = 2
    "robust": (dict(max_eval_farms=16, wd_uncertainty=dict(delta=(-3.0, 3.0), weight=(1.0, 1.0), frame="fixed")), "_robust",
               "neither wf_robust_optimize nor wf_robust_evaluate has run yet"),  # R M = 8: C = 2
}
# |step_ms + glue_ms - total_ms| is the event timer's rounding, not the code's: 15 float32 intervals added up in float32
# against one float32 interval over the same first and last event.  Measured on the library as it was before the searches
# shared a driver, over 20 runs of this test (totals of 0.40 .. 0.45 ms): at most 2.98e-08 ms (yawopt) and 5.215e-08 ms
# (robust) — one to two ulps of the total.  Allowed: four times the largest value seen.
SPLIT_TOL_MS = 4 * 5.215e-08


@pytest.mark.parametrize("search", list(SEARCHES))
def test_timing_contract(search):
    """timing() before a run is refused; without detail only the total is measured; with detail the intervals tile the run from
    its first to its last event — step + glue = total up to the timer's rounding (measured: 5.215e-08 ms at most; bound
    SPLIT_TOL_MS = 2.086e-07 ms) —, the chunk boundary's empty interval counted as glue; detail off again gives
    no split; the timed runs return the bits of the untimed one; the evaluator is in place."""
    from wfcrl_env_amd.backend import WfStep

    kwargs, getter, not_run = SEARCHES[search]
    ws, wd = yawopt_ref.ROW3_WIND
    w = WfStep(*yawopt_ref.ROW3, env_batch=len(ws))
    w.set_wind(ws, wd)
    ext = getattr(w, getter)()
    with pytest.raises(ValueError, match=re.escape(not_run)):  # (WF_E_INVALID, a call out of order: the wrapper's ValueError)
        ext.timing()

    def run():
        return {k: np.array(v) for k, v in w.optimize_yaw(passes=(3,), strict=True, **kwargs).items()}

    plain = run()
    t = ext.timing()
    print(f"{search} plain: {t}")
    assert t["total_ms"] > 0.0 and t["step_ms"] == 0.0 and t["glue_ms"] == 0.0, t
    ext.timing(detail=True)
    detailed = run()
    t = ext.timing()
    print(f"{search} detail: {t}, step + glue - total = {t['step_ms'] + t['glue_ms'] - t['total_ms']:.3e} ms")
    assert t["step_ms"] > 0.0 and t["glue_ms"] > 0.0, t
    assert abs(t["step_ms"] + t["glue_ms"] - t["total_ms"]) <= SPLIT_TOL_MS, t
    ext.timing(detail=False)
    again = run()
    t = ext.timing()
    assert t["total_ms"] > 0.0 and t["step_ms"] == 0.0 and t["glue_ms"] == 0.0, t
    for k in ("yaw", "power", "power_initial"):
        assert np.array_equal(detailed[k], plain[k]) and np.array_equal(again[k], plain[k]), (search, k)
    assert ext.evaluator()
    w.close()
