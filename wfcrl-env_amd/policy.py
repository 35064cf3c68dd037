"""MLP policies as `WfStep.policy_returns` / `VecWindFarmEnv.policy_returns` take them (include/wfpolicy.h): the network's
description (`mlp_spec`) and the conversion of torch modules into a parameter block (`policy_from_torch`).  Needs no GPU.

A policy is a deterministic MLP of 1..4 linear layers with one hidden activation, of one of two kinds:
  "central"  input the env's flattened observation, 3 N + 2 values — yaw (N), local wind speed (N), local wind direction (N),
             free wind (speed, direction) —, output N (continuous actions) or 3 N (discrete, turbine-major logits)
  "shared"   input one turbine's (yaw, wind speed, wind direction), with use_freewind also the free wind: 3 or 5 values;
             output 1 or 3; the same weights serve every turbine
A parameter vector is laid out as torch.nn.utils.parameters_to_vector lays out an nn.Sequential of nn.Linear: per layer the
weight (out, in) row-major, then the bias (out)."""
import numpy as np

KINDS = {"central": 0, "shared": 1}
ACTIVATIONS = {"relu": 1, "softsign": 2, "tanh": 3}
FINALS = {None: 0, "none": 0, "softsign": 2, "tanh": 3}
MAX_LAYERS, MAX_WIDTH, MAX_K, MAX_H = 4, 256, 64, 256


def param_count(widths) -> int:
    """P = sum_l (in_l + 1) out_l."""
    return int(sum((int(a) + 1) * int(b) for a, b in zip(widths[:-1], widths[1:])))


def mlp_spec(kind, widths, activation="tanh", final=None, out_scale=1.0, shift=None, scale=None, use_freewind=False) -> dict:
    """The description of a network: kind "central" / "shared"; widths (D, hidden..., out); activation "relu" / "softsign" /
    "tanh" of the hidden layers; final None / "softsign" / "tanh" after the last layer; out_scale multiplies the (continuous)
    output; shift, scale (D,) float64 normalise the input, x = (obs - shift) * scale (default 0 and 1); use_freewind (shared):
    the input also holds the free wind.  What depends on the env — D and the output width against its N and its action
    encoding — is checked by policy_returns."""
    if kind not in KINDS:
        raise ValueError('kind must be "central" or "shared"')
    widths = tuple(int(w) for w in widths)
    if not 2 <= len(widths) <= MAX_LAYERS + 1:
        raise ValueError("widths must name the input width, up to three hidden widths and the output width: 1..4 layers")
    if any(w < 1 for w in widths) or any(w > MAX_WIDTH for w in widths[1:-1]):
        raise ValueError("every width must be >= 1 and a hidden width at most 256")
    if activation not in ACTIVATIONS:
        raise ValueError('unknown activation: "relu", "softsign" or "tanh"')
    if final not in FINALS:
        raise ValueError('unknown final activation: None, "softsign" or "tanh"')
    if kind == "shared" and widths[0] != (5 if use_freewind else 3):
        raise ValueError("a shared policy's input width is 3, or 5 with use_freewind")
    D = widths[0]
    shift = np.zeros(D) if shift is None else np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
    scale = np.ones(D) if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
    if shift.shape != (D,) or scale.shape != (D,):
        raise ValueError("shift and scale must hold one value per input")
    if not (np.isfinite(shift).all() and np.isfinite(scale).all() and np.isfinite(out_scale)):
        raise ValueError("shift, scale and out_scale must be finite")
    return {"kind": kind, "widths": widths, "activation": activation, "final": None if final == "none" else final,
            "out_scale": float(out_scale), "shift": shift, "scale": scale, "use_freewind": bool(use_freewind)}


def _layers(module):
    """(the Linear layers, the hidden activation's name or None, the final activation's name or None) of an nn.Sequential of
    Linear / ReLU / Tanh / Softsign."""
    import torch.nn as nn

    names = {nn.ReLU: "relu", nn.Tanh: "tanh", nn.Softsign: "softsign"}
    if not isinstance(module, nn.Sequential):
        raise ValueError("a policy must be an nn.Sequential of Linear, ReLU, Tanh and Softsign modules")
    linears, hidden, final, last_was_linear = [], None, None, False
    mods = list(module)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Linear):
            if last_was_linear:
                raise ValueError("two Linear layers follow each other: every hidden layer needs the activation")
            if m.bias is None:
                raise ValueError("every Linear layer needs a bias")
            linears.append(m)
            last_was_linear = True
        elif type(m) in names:
            if not last_was_linear:
                raise ValueError("an activation must follow a Linear layer")
            name = names[type(m)]
            if i == len(mods) - 1:
                final = name
            elif hidden not in (None, name):
                raise ValueError("the hidden layers must share one activation")
            else:
                hidden = name
            last_was_linear = False
        else:
            raise ValueError(f"unsupported module {type(m).__name__}: Linear, ReLU, Tanh and Softsign are served")
    if not linears:
        raise ValueError("the policy holds no Linear layer")
    if final == "relu":
        raise ValueError("the final activation may be Tanh or Softsign (or none), not ReLU")
    for a, b in zip(linears[:-1], linears[1:]):
        if a.out_features != b.in_features:
            raise ValueError("the layers' shapes do not chain")
    return linears, hidden, final


def policy_from_torch(modules, kind, out_scale=1.0, shift=None, scale=None, use_freewind=False):
    """(params (K, P) float32, spec) of one nn.Sequential or a list of K of them with the same architecture: Linear layers with
    ReLU / Tanh / Softsign between them (one kind per network) and optionally Tanh or Softsign after the last.  params[k] is
    torch.nn.utils.parameters_to_vector(modules[k].parameters()) in float32."""
    import torch.nn as nn

    mods = [modules] if isinstance(modules, nn.Module) else list(modules)
    if not mods:
        raise ValueError("no policy given")
    arch, rows = None, []
    for m in mods:
        linears, hidden, final = _layers(m)
        a = (tuple([linears[0].in_features] + [lin.out_features for lin in linears]), hidden, final)
        if len(linears) > 1 and hidden is None:
            raise ValueError("the hidden layers need an activation")
        if arch is None:
            arch = a
        elif a != arch:
            raise ValueError("the policies must share one architecture")
        vec = []
        for lin in linears:
            vec.append(lin.weight.detach().cpu().numpy().astype(np.float32).reshape(-1))
            vec.append(lin.bias.detach().cpu().numpy().astype(np.float32).reshape(-1))
        rows.append(np.concatenate(vec))
    widths, hidden, final = arch
    spec = mlp_spec(kind, widths, hidden or "relu", final, out_scale, shift, scale, use_freewind)
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32), spec
