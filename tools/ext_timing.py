"""What tools/yawopt_timing.py, robust_timing.py, grad_timing.py, credit_timing.py and lookahead_timing.py share: the plain wf_step loop on an extension object's own
evaluator handle — the baseline their totals are divided by."""
import ctypes as C

import torch


def plain_loop_ms(w, ext, n_steps, n_eval, load=False):
    """n_steps wf_step calls on the evaluator of `ext` (an extension object of the WfStep `w` that has run: n_eval farms, its
    wind), with nothing between them, between two events on the shared stream.  load: the steps write the load output too."""
    lib, ev = w._lib, C.c_void_p(ext.evaluator())
    yaw = torch.zeros((n_eval, w.num_turbines), dtype=torch.float32, device="cuda")
    power = torch.empty_like(yaw)
    lptr = torch.empty((n_eval, w.num_turbines, 4), dtype=torch.float32, device="cuda").data_ptr() if load else None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n_steps):
        rc = lib.wf_step(ev, yaw.data_ptr(), power.data_ptr(), None, None, lptr, 1)
        assert rc == 0, rc
    b.record()
    b.synchronize()
    return a.elapsed_time(b)
