"""pf_mlp_forward / pf_mlp_backward behind torch.autograd: a small MLP over any number of rows whose differentiable inputs are its
parameter tensors (BatchEngine.mlp_forward / mlp_backward; include/pyflyt_amd.h has the semantics). With pyflyt_amd.ppo_loss between
an actor and a critic evaluated this way, an epoch's only torch work is the optimiser's step."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable


class _Mlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, x, activation, *params):
        layers = [(params[2 * l].detach(), params[2 * l + 1].detach()) for l in range(len(params) // 2)]
        out = torch.empty(x.numel() // x.shape[-1], layers[-1][0].shape[0], dtype=torch.float32, device=x.device)
        engine.mlp_forward(x, layers, activation, out=out)
        # (x and the parameters by reference, nothing copied: backward computes the hidden activations again from them)
        ctx.engine, ctx.x, ctx.activation, ctx.layers = engine, x, activation, layers
        return out.view(x.shape[:-1] + (out.shape[-1],))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rows, out_dim = ctx.x.numel() // ctx.x.shape[-1], grad_out.shape[-1]
        g = grad_out.reshape(rows, out_dim)  # (an expanded or strided gradient, e.g. of out.sum(), becomes a tensor of its own)
        g = g.contiguous() if g.dtype == torch.float32 else g.to(torch.float32).contiguous()
        grads = ctx.engine.mlp_backward(ctx.x, g, ctx.layers, ctx.activation)
        # (the engine owns its gradient tensors and overwrites them at the next call of this shape: autograd gets copies, a few KB)
        need, flat = ctx.needs_input_grad[3:], []
        for l, (gw, gb) in enumerate(grads):
            flat += [gw.clone() if need[2 * l] else None, gb.clone() if need[2 * l + 1] else None]
        return (None, None, None, *flat)


def parse_net(net, activation=None, name="net"):
    """(layers [(weight, bias), ...], "tanh" / "relu") of what mlp and ppo_grad accept as a network: a torch.nn.Sequential of Linear
    layers with one kind of activation between them, or a list of (weight, bias) together with `activation`."""
    nn = torch.nn
    if isinstance(net, nn.Sequential):
        mods = list(net)
        if len(mods) % 2 == 0:
            raise ValueError(f"{name}: the Sequential must end with a Linear (the output layer is affine)")
        layers, acts = [], set()
        for i, m in enumerate(mods):
            if i % 2 == 0:
                if not isinstance(m, nn.Linear) or m.bias is None:
                    raise ValueError(f"{name}: module {i} must be a Linear with a bias, got {type(m).__name__}")
                layers.append((m.weight, m.bias))
            elif isinstance(m, (nn.Tanh, nn.ReLU)):
                acts.add("tanh" if isinstance(m, nn.Tanh) else "relu")
            else:
                raise ValueError(f"{name}: module {i} must be a Tanh or a ReLU, got {type(m).__name__}")
        if len(acts) > 1:
            raise ValueError(f"{name}: one kind of activation per network (Tanh or ReLU), got both")
        if activation is not None and acts and activation not in acts:
            raise ValueError(f"activation={activation!r} contradicts the Sequential's modules")
        activation = acts.pop() if acts else (activation or "tanh")
    else:
        try:
            layers = [tuple(l) for l in net]
        except TypeError:
            raise ValueError(f"{name} must be a torch.nn.Sequential or a list of (weight, bias), got {type(net).__name__}") from None
        if activation is None:
            raise ValueError("a list of (weight, bias) comes with activation='tanh' or 'relu'")
    if any(len(l) != 2 for l in layers):
        raise ValueError(f"{name}: every layer is a (weight, bias) pair")
    return layers, activation


def mlp(env_or_engine, x, net, activation=None):
    """out = mlp(env, x, net): `net` on the rows of x [..., in_dim] -> [..., out_dim], on the device's matrix units without a GEMM
    library, differentiable with respect to the network's PARAMETERS. `net` is a torch.nn.Sequential of the shape
    MLPPolicy.from_torch accepts (Linear layers with one kind of activation, Tanh or ReLU, between them; 2 or 3 Linear layers,
    hidden widths 1..64, in_dim 1..128, out_dim 1..8), or a list of (weight, bias) tensors together with activation="tanh" / "relu".
    The forward has policy_act's arithmetic bit for bit.

    x gets NO gradient: an x with requires_grad raises ValueError rather than leaving x.grad None. backward() computes the hidden
    activations again from x, which is kept BY REFERENCE, not copied: x must not be modified between this call and backward() (the
    parameters neither: an optimiser step belongs after backward(), where it always is). Nothing synchronises with the host."""
    engine = getattr(env_or_engine, "engine", env_or_engine)
    if not hasattr(engine, "mlp_forward"):
        raise ValueError(f"the first argument must be a vector env or a BatchEngine, got {type(env_or_engine).__name__}")
    layers, activation = parse_net(net, activation)
    if not torch.is_tensor(x):
        raise ValueError(f"x must be a float32 tensor of shape (..., in_dim), got {type(x).__name__}")
    if x.requires_grad:
        raise ValueError("pyflyt_amd.mlp produces no gradient for x (pf_mlp_backward differentiates the parameters only), and x requires one: "
                         "pass x.detach(), or use torch modules where the input's gradient is needed")
    return _Mlp.apply(engine, x, activation, *[t for l in layers for t in l])
