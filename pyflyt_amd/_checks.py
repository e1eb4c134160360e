"""The argument checks of the Python layer, one copy of each. The texts are part of the interface: tests and users match on them, so
a rule is reworded nowhere and a call site passes its own wording where the wordings differ."""
from __future__ import annotations

import torch

FLAGS = (torch.bool, torch.uint8)  # what a trajectory's terminated / truncated / episode_start and a mask may be
GATE = (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)  # pf_kl_control's gate word, as a tensor
NO_F32 = "{name} must be a float32 tensor of shape {shape}"  # (tensor(required=...): the commonest wording for what is no tensor at all)


def tensor(device, t, name, shapes, dtypes=torch.float32, required=None):
    """Every tensor whose data_ptr() crosses the C ABI is checked here: the kernels index raw pointers, so a wrongly sized, typed,
    placed or strided tensor would read or write out of bounds silently. `shapes`: the shape, or a tuple of admitted shapes (the
    first is the one a refusal names). `dtypes`: one dtype, named bare ("float32"), or a tuple of admitted ones, named as torch
    spells them ("torch.bool/torch.uint8"). `required`: None = `t` may be None (returned as it is); a text = anything that is no
    tensor, None included, is refused with that text, its {name} and {shape} filled in, and ", got <its type>". Returns `t`.
    Nothing is formatted for a tensor that passes: adam_step comes here for every gradient at every step."""
    if t is None and required is None:
        return None
    many, several = dtypes.__class__ is tuple, bool(shapes) and shapes[0].__class__ is tuple
    try:
        if (t.dtype in dtypes if many else t.dtype == dtypes) and t.device == device and t.is_contiguous() and (t.shape in shapes if several else t.shape == shapes):
            return t
    except AttributeError:  # (no tensor at all)
        pass
    shape = shapes[0] if several else tuple(shapes)
    label = "/".join(map(str, dtypes)) if many else str(dtypes).replace("torch.", "")
    must = f"{name} must be a contiguous {label} tensor of shape {shape} on {device}"
    if not torch.is_tensor(t):
        raise ValueError(f"{required.format(name=name, shape=shape) if required else must}, got {type(t).__name__}")
    raise ValueError(f"{must}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def ranked(t, name, what, dim=None):
    """`t` is a tensor with `dim` axes (None: at least one) -- asked before a shape is read off it; `what`, its {name} filled in, is
    the refusal up to ", got <its type or shape>"."""
    if not torch.is_tensor(t) or (t.dim() < 1 if dim is None else t.dim() != dim):
        raise ValueError(f"{what.format(name=name)}, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")


def unit_interval(x, name):
    if not 0.0 <= float(x) <= 1.0:  # (False for a NaN as well)
        raise ValueError(f"{name} must be finite and in [0, 1], got {x}")


def number(x, name, or_else=""):
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{name} must be a Python number{or_else}, got {type(x).__name__}")


def boolean(x, name):
    if not isinstance(x, bool):
        raise ValueError(f"{name} must be a bool, got {type(x).__name__}")


def non_negative(x, name):
    if not 0.0 <= float(x) < float("inf"):  # (False for a NaN as well)
        raise ValueError(f"{name} must be finite and >= 0, got {x}")


def positive(x, name):
    if not 0.0 < float(x) < float("inf"):  # (False for a NaN as well)
        raise ValueError(f"{name} must be finite and > 0, got {x}")
