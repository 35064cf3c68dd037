"""torch autograd through the farm step: `differentiable_power` (include/wfgrad.h) and, through H steps of the fused env,
`differentiable_return` (include/wfretgrad.h; its docstring below).

    power = differentiable_power(wfstep, yaw)          # (B, N) float32, W
    (power * credit).sum().backward()                  # yaw.grad: (B, N) float32, W/deg

Forward is one plain `WfStep.step` on the handle.  Backward is ONE call of the gradient extension with
cotangent = grad_output, device pointers in and out, no host copy: the vector-Jacobian product G[i] = sum_j c_j J[i, j].

What the derivative is.  J is the DIFFERENCE QUOTIENT the header defines, at a finite step: turbine i is moved to
y+ = float32(min(y + step, hi)) and y- = float32(max(y - step, lo)), J[i, j] = (P_j(y+) - P_j(y-)) / (y+ - y-), one-sided at
a bound and exactly 0 where y+ <= y-.  It is not an analytic or adjoint derivative of the step kernels: the model has
kinks (the power table's knots, the overlap count) and `step` sets the scale at which they are seen.  The sum over j runs in
caller order in float64 and is rounded once to float32.

The wind.  Backward evaluates the quotient under the wind the handle holds AT BACKWARD TIME.  It must be the wind of the
forward: do not call set_wind / sample_wind / wind_series_step / an env step between the two.
"""
from __future__ import annotations

import torch


class _DifferentiablePower(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yaw, wfstep, step, bounds, strict):
        y = yaw.detach().contiguous()
        ctx.save_for_backward(y)
        ctx.wfstep, ctx.step, ctx.bounds, ctx.strict = wfstep, step, bounds, strict
        return wfstep.step(y)["power"]

    @staticmethod
    def backward(ctx, grad_output):
        (y,) = ctx.saved_tensors
        c = grad_output.to(torch.float32).contiguous()
        g = ctx.wfstep._grad().backward(y, c, ctx.step, ctx.bounds, ctx.strict)
        return g.to(torch.float32), None, None, None, None


def differentiable_power(wfstep, yaw, step=1.0, bounds=(-45.0, 45.0), strict=False):
    """(B, N) float32 per-turbine power of `wfstep` (a backend.WfStep) at yaw — a (B, N) float32 CUDA tensor, degrees — with
    a backward pass: yaw.grad is the float32 of the difference-quotient vector-Jacobian product described above.
      step    the perturbation h in degrees
      bounds  (lo, hi) the perturbed yaws are clipped to (default: the range the float64 oracle is defined on)
      strict  the backward pass solves every perturbed farm in float64 (validation); the forward is the handle's own step
    The wind the handle holds at backward time must be the wind of the forward."""
    if not (torch.is_tensor(yaw) and yaw.is_cuda and yaw.dtype == torch.float32):
        raise ValueError("differentiable_power needs a float32 CUDA tensor (env_batch, num_turbines)")
    if tuple(yaw.shape) != (wfstep.env_batch, wfstep.num_turbines):
        raise ValueError("yaw must be (env_batch, num_turbines)")
    return _DifferentiablePower.apply(yaw, wfstep, float(step), (float(bounds[0]), float(bounds[1])), bool(strict))


class _DifferentiableReturn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, actions, wfstep, gamma, wind, delta, strict):
        a = actions.detach().contiguous()
        r = wfstep.return_gradient(a, gamma=gamma, wind=wind, delta=delta, strict=strict, want=("returns", "action_gradient"))
        ctx.save_for_backward(r["action_gradient"])
        ctx.dtype = actions.dtype
        return r["returns"]

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        return (grad_output[..., None, None] * g).to(ctx.dtype), None, None, None, None, None


def differentiable_return(wfstep, actions, gamma=1.0, wind=None, delta=1.0, strict=False):
    """(B, K) float64 discounted H-step returns of `wfstep` (a backend.WfStep with an env state) for actions — a
    (B, K, H, N) float32 CUDA tensor in the continuous encoding — with a backward pass (include/wfretgrad.h).

        ret = differentiable_return(wfstep, actions, gamma=0.95)      # (B, K) float64
        ret.sum().backward()                                          # actions.grad: (B, K, H, N) float32, reward / deg

    Forward is ONE run of the return-gradient extension, which also keeps action_gradient; backward is
    grad_output[..., None, None] * action_gradient cast to the dtype of `actions`: no second run.

    What the derivative is.  As differentiable_power's, a DIFFERENCE QUOTIENT at a finite step: per step of the horizon
    turbine i of the yaw the transition reaches is moved to y+ = float32(min(y + delta, hi)) and y- = float32(max(y - delta, lo))
    — hi, lo the env's yaw bounds —, q = (r(y+) - r(y-)) / (y+ - y-), one-sided at a bound and exactly 0 where y+ <= y-.  It is
    chained to the actions through a 0/1 TRANSITION JACOBIAN: 1 where the budget gate, the clip to +-yaw_step and the clip to
    the yaw bounds returned their input unchanged, else 0; the dependence of later gates on the accumulated actuation is
    piecewise constant and contributes 0.  It is not an analytic or adjoint derivative of the step kernels: the model has
    kinks and `delta` sets the scale at which they are seen.

    The env state and the wind are those of the FORWARD (wind: as WfStep.lookahead_returns — None, (B, H, 2) or "series");
    nothing is read at backward time.  strict solves every row in float64."""
    if not (torch.is_tensor(actions) and actions.is_cuda and actions.dtype == torch.float32):
        raise ValueError("differentiable_return needs a float32 CUDA tensor (env_batch, K, H, num_turbines)")
    if actions.ndim != 4 or actions.shape[0] != wfstep.env_batch or actions.shape[3] != wfstep.num_turbines:
        raise ValueError("actions must be (env_batch, K, H, num_turbines)")
    return _DifferentiableReturn.apply(actions, wfstep, float(gamma), wind, float(delta), bool(strict))
