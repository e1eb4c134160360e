"""pf_ppo_loss, BatchEngine.ppo_loss and pyflyt_amd.ppo_loss on the device, against a float64 torch restatement of the contract in
include/pyflyt_amd.h (written from the contract, not from the kernels) whose gradients come from torch.autograd in float64 on the
same float32 inputs. Per-row gradients: within 8 x the deviation of an eager torch float32 evaluation of the same loss and backward
(the same precision, another operation order). Sums: within bounds derived below from gamma_N sum |t_i| of the double sums and the
float32 rounding of their terms. Exact where the contract is exact: the count, the clip fraction, the zero pattern, NaN poisoning,
c = 0, determinism, alignment, capture, the refusals.

Inputs: |z| <= 4, log_std in [-1, 0.5], logp_old = the float64 log-probability minus d with d from {-0.4, -0.1, 0, 0.1, 0.4} and
clip = 0.2: the ratios lie at 0.67, 0.905, 1, 1.105, 1.49, each more than 0.09 from 0.8 and 1.2 and so far beyond float32's error in
a log-probability (about 1e-5): all six branch cases occur and none is decided by rounding."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import MLPPolicy, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from pyflyt_amd.gym_envs import make_vec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = 2.0 ** -24, 2.0 ** -53  # unit roundoffs
CLIP = 0.2
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
SHIFTS = (-0.4, -0.1, 0.0, 0.1, 0.4)
# The grid is capped at 1024 blocks of 256 threads, and a thread takes several rows per trip of its loop, so the row count at which a
# loop makes a second, ragged trip differs per kernel:
GRID_ROWS = 1024 * 256
BIG = 2 * GRID_ROWS + 77   # ppo_main_kernel<A, generic> (two rows per trip): A != 4 and the unaligned A = 4. One trip of the other two
BIG3 = 3 * GRID_ROWS + 77  # ppo_main_kernel<4, float4> (three rows per trip); two trips of the generic kernels
BIG8 = 8 * GRID_ROWS + 77  # ppo_adv_kernel (eight rows per trip); a third trip of the float4 kernel, a fifth of the generic ones
ROWS = (1, 63, 64, 65, 257, 1000, BIG)


def f32(x):
    """A Python number as the float32 the C ABI carries."""
    return float(torch.tensor(x, dtype=torch.float32))


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)  # (a context WITHOUT an env task: any context serves)
    yield e
    e.close()


_INPUTS = {}


def inputs(M, A, seed=0, invalid=0.25):
    """float32 device tensors, computed once per (M, A, seed, invalid) and never changed."""
    key = (M, A, seed, invalid)
    if key in _INPUTS:
        return _INPUTS[key]
    g = torch.Generator().manual_seed(1000 * A + seed + M % 997)
    log_std = (torch.rand(A, generator=g, dtype=torch.float64) * 1.5 - 1.0).float()
    mean = torch.randn(M, A, generator=g, dtype=torch.float64).float()
    z = (torch.rand(M, A, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 3.99
    actions = (mean.double() + z * log_std.double().exp()).float()
    zz = (actions.double() - mean.double()) * (-log_std.double()).exp()
    assert float(zz.abs().max()) <= 4.0
    logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
    d = torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=g)]
    logp_old = (logp - d).float()
    advantages = (torch.randn(M, generator=g, dtype=torch.float64) * 2.0 + 0.3).float()
    returns = (torch.randn(M, generator=g, dtype=torch.float64) * 3.0 + 1.0).float()
    value = (returns.double() + torch.randn(M, generator=g, dtype=torch.float64)).float()
    valid = torch.rand(M, generator=g) >= invalid
    valid[0] = True
    x = dict(mean=mean, log_std=log_std, value=value, actions=actions, logp_old=logp_old, advantages=advantages, returns=returns, valid=valid)
    _INPUTS[key] = {k: v.to(DEV).contiguous() for k, v in x.items()}
    return _INPUTS[key]


def reference(x, dtype, clip, vf_coef, ent_coef, normalize, valid):
    """The contract in `dtype` arithmetic on the float32 inputs, gradients by torch.autograd. mu and sigma are float64 in either
    case (the contract accumulates them in double and hands the rows their float32 roundings). Returns a dict of float64 values."""
    clip, vf_coef, ent_coef = f32(clip), f32(vf_coef), f32(ent_coef)
    M, A = x["mean"].shape
    v = torch.ones(M, dtype=torch.bool, device=DEV) if valid is None else valid.bool()
    c = int(v.sum())
    w = 1.0 / c if c else 0.0
    zero = torch.zeros((), dtype=dtype, device=DEV)
    mean, log_std, value = (x[k].to(dtype).requires_grad_(True) for k in ("mean", "log_std", "value"))
    act, lpo, adv, ret = (x[k].to(dtype) for k in ("actions", "logp_old", "advantages", "returns"))
    a64 = x["advantages"].double()
    mu = float(torch.where(v, a64, 0.0).sum()) * w
    sigma = math.sqrt(float(torch.where(v, (a64 - mu) ** 2, 0.0).sum()) * w)
    a = (adv - f32(mu)) * f32(1.0 / max(sigma, 1e-8)) if normalize else adv
    z = (act - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    d = logp - lpo
    r = torch.exp(d)
    u, vv = r * a, torch.clamp(r, 1.0 - clip, 1.0 + clip) * a
    surr = torch.minimum(u, vv)
    wt = torch.tensor(w, dtype=dtype, device=DEV)
    policy_loss = -(torch.where(v, surr, zero).sum() * wt)
    value_loss = 0.5 * (torch.where(v, (value - ret) ** 2, zero).sum() * wt)
    H = (log_std + (0.5 + HALF_LOG_2PI)).sum()
    loss = policy_loss + vf_coef * value_loss - ent_coef * H
    gm, gv, gls = torch.autograd.grad(loss, [mean, value, log_std])
    with torch.no_grad():
        kl_t = torch.where(v, (r - 1.0) - d, zero)
        clipped = int((v & ((r - 1.0).abs() > clip)).sum())
        rv, dv = ret.double(), (value - ret).double()
        m_r, m_d = float(torch.where(v, rv, 0.0).sum()) * w, float(torch.where(v, dv, 0.0).sum()) * w
        var_r = float(torch.where(v, rv * rv, 0.0).sum()) * w - m_r * m_r
        var_d = float(torch.where(v, dv * dv, 0.0).sum()) * w - m_d * m_d
        ev = 1.0 - var_d / var_r if var_r != 0.0 else float("nan")
        inf = torch.tensor(float("inf"), dtype=dtype, device=DEV)
        stats = [float(c), float(loss), float(policy_loss), float(value_loss), float(H), float(kl_t.sum() * wt), w * clipped, mu, sigma, ev,
                 float(torch.where(v, r, inf).min()), float(torch.where(v, r, -inf).max())]
        return dict(grad_mean=gm.double(), grad_value=gv.double(), grad_log_std=gls.double(), stats=stats, clipped=clipped, c=c, w=w, valid=v,
                    z=z.double(), logp=logp.double(), d=d.double(), r=r.double(), a=a.double(), surr=surr.double(), dv=(value - ret).double(),
                    ret=ret.double(), adv=a64, kl_t=kl_t.double(), log_std=log_std.detach().double(), live=(u <= vv) & v, var_r=var_r, var_d=var_d)


def gamma_n(terms):
    return terms * U64 / (1.0 - terms * U64)


def bounds(ref, M, A, vf_coef, ent_coef):
    """The largest admissible |device - float64| of grad_log_std [A] and of stats 1-11, from the float64 reference's own rows.
    Double sums of N <= M + 16 terms in any order are off by at most g = gamma_N sum |t_i| (Higham (4.4)); the reference sums the
    same terms in double and is off by as much, hence 2 g. The terms themselves are float32 results; with u = 2^-24:
      z      = (x - m) * expf(-log_std): one rounding, expf within one ulp (2 u), one rounding: relative 4 u; z^2: 9 u.
      logp   : term ((-z/2) z - log_std) - k: 9 u z^2 / 2 + u (|t| + |t| + k); A adds of partial sums no larger than sum |t|:
               e_l = u (sum_c (4.5 z_c^2 + 2 |t_c| + 1) + A sum_c |t_c| + |d|) including the rounding of d = logp - logp_old.
      r      = expf(d): relative e_l + 2 u.        a: (A - mu32) * inv32, two roundings: relative 2 u.
      surr   = min(r a, clamp(r) a): relative e_l + 2 u + 2 u + u, and u more for the float32 rounding of 1 -+ clip: e_l + 6 u.
      gl     = ((-w32) a) r: w32 one rounding, two products: relative e_l + 2 u + 2 u + 3 u = e_l + 7 u.
      t_ic   = gl (z^2 - 1): |gl| ((e_l + 8 u) |z^2 - 1| + 9 u z^2 + u |z^2 - 1|).
      kl term (r - 1) - d: r - 1 is exact (r in [1/2, 2]); r (e_l + 2 u) + e_l + u |term|.
      dv     = value - returns: one rounding; its square is taken in double: relative 2 u (1 + u).
    Every bound carries a factor 1.02 for the products of these first-order terms."""
    v, w, u = ref["valid"], ref["w"], U32
    g = 2.0 * gamma_n(M + 16)
    z, ls = ref["z"], ref["log_std"]
    t = -0.5 * z * z - ls - HALF_LOG_2PI
    abs_t = t.abs().sum(-1)
    e_l = u * ((4.5 * z * z + 2.0 * t.abs() + 1.0).sum(-1) + A * abs_t + ref["d"].abs())

    def total(x):  # over the valid rows: a number for [M], per column for [M, A]
        return float(torch.where(v, x, 0.0).sum()) if x.dim() == 1 else torch.where(v[:, None], x, 0.0).sum(0)

    surr, r, dv = ref["surr"].abs(), ref["r"], ref["dv"]
    b_pl = 1.02 * w * (total(surr * (e_l + 6.0 * u)) + g * total(surr))
    b_vl = 1.02 * 0.5 * w * (total(dv * dv) * (2.0 * u + g))
    H_abs = float((ls + (0.5 + HALF_LOG_2PI)).abs().sum())
    b_H = 1.02 * (gamma_n(2 * A + 2) * 2.0 * H_abs + A * U64)  # (the constant 1/2 (1 + log 2 pi) is itself rounded once)
    b_loss = b_pl + f32(vf_coef) * b_vl + f32(ent_coef) * b_H + 8.0 * U64 * (abs(ref["stats"][2]) + abs(ref["stats"][3]) + H_abs)
    kl_t = ref["kl_t"].abs()
    b_kl = 1.02 * w * (total(r * (e_l + 2.0 * u) + e_l + u * kl_t) + g * total(kl_t))
    adv = ref["adv"]
    b_mu = 1.02 * (g * w * total(adv.abs()) + 2.0 * U64 * abs(ref["stats"][7]))
    b_var = 1.02 * 4.0 * g * w * total(adv * adv)  # s2 / c - mu^2: both no larger than sum A^2 / c
    sigma = ref["stats"][8]
    b_sigma = b_var / sigma if sigma * sigma > b_var else math.sqrt(b_var)  # |sqrt x - sqrt y| <= |x - y| / sqrt x, and <= sqrt |x - y|
    ret = ref["ret"]
    b_var_r = 1.02 * 4.0 * g * w * total(ret * ret)
    m_d = w * abs(total(dv))
    b_var_d = 1.02 * (4.0 * g * w * total(dv * dv) + 2.0 * u * w * total(dv * dv) + 2.0 * m_d * u * w * total(dv.abs()))
    var_r, var_d = ref["var_r"], ref["var_d"]
    b_ev = 1.02 * (b_var_d + abs(var_d / var_r) * b_var_r) / (var_r - b_var_r) if var_r > b_var_r else float("inf")
    b_r = 1.02 * r * (e_l + 4.0 * u)  # per row: the logp difference's error and two ulps of expf
    gl = torch.where(ref["live"], w * ref["a"] * r, 0.0).abs()
    zz1 = (z * z - 1.0).abs()
    t_err = gl[:, None] * ((e_l[:, None] + 8.0 * u) * zz1 + 9.0 * u * z * z + u * zz1)
    b_gls = 1.02 * (total(t_err) + g * total(gl[:, None] * zz1)) + 2.0 * u * (ref["grad_log_std"].abs() + f32(ent_coef))  # (+ the float32 output)
    return dict(grad_log_std=b_gls, stats={1: b_loss, 2: b_pl, 3: b_vl, 4: b_H, 5: b_kl, 7: b_mu, 8: b_sigma, 9: b_ev}, r=b_r)


def call(eng, x, valid="own", clip=CLIP, vf_coef=0.5, ent_coef=0.01, normalize=True, **change):
    """BatchEngine.ppo_loss on x; the outputs cloned (the engine owns them) and synchronised."""
    t = dict(x, **change)
    v = t["valid"] if isinstance(valid, str) else valid
    out = eng.ppo_loss(t["mean"], t["log_std"], t["value"], t["actions"], t["logp_old"], t["advantages"], t["returns"], valid=v, clip=clip,
                       vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=normalize)
    out = [o.clone() for o in out]
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_against_fp64(eng, M, A, vf_coef=0.5, ent_coef=0.01, normalize=True, valid="own", seed=0):
    x = inputs(M, A, seed)
    v = x["valid"] if isinstance(valid, str) else valid
    kw = dict(clip=CLIP, vf_coef=vf_coef, ent_coef=ent_coef, normalize=normalize)
    gm, gv, gls, stats = call(eng, x, valid=v, **kw)
    ref = reference(x, torch.float64, valid=v, **kw)
    eager = reference(x, torch.float32, valid=v, **kw)
    vb = ref["valid"]
    # exact: the count, the clip fraction, the rows whose gradient is zero
    st = stats.tolist()
    assert st[0] == ref["c"]
    assert st[6] == ref["w"] * ref["clipped"] and round(st[6] * st[0]) == ref["clipped"]
    assert st[12:] == [0.0] * 4
    assert torch.equal(gm != 0, ref["grad_mean"] != 0)
    assert not bool(gm[~vb].any()) and not bool(gv[~vb].any())
    if M >= 257:  # all six branch cases are there: below, inside and above the clip range with either sign of the advantage
        low, high, pos = ref["r"] < 0.8, ref["r"] > 1.2, ref["a"] > 0
        for rng in (low, high, ~low & ~high):
            assert bool((rng & pos & vb).any()) and bool((rng & ~pos & vb).any())
        assert bool((ref["live"] & (low | high)).any()) and bool((~ref["live"] & vb).any())
    # per-row gradients: 8 x the float32 eager evaluation's own deviation
    for name, got in (("grad_mean", gm), ("grad_value", gv)):
        e32 = float((eager[name] - ref[name]).abs().max())
        dev = float((got.double() - ref[name]).abs().max())
        print(f"M={M} A={A} {name}: device deviation {dev:.3e}, eager float32 deviation {e32:.3e}, ratio {dev / e32 if e32 else float('nan'):.3f}")
        assert dev <= 8.0 * e32, (name, dev, e32)
    # sums
    b = bounds(ref, M, A, vf_coef, ent_coef)
    err = (gls.double() - ref["grad_log_std"]).abs()
    print(f"M={M} A={A} grad_log_std: worst error / bound {float((err / b['grad_log_std']).max()):.3f}")
    assert bool((err <= b["grad_log_std"]).all()), (err, b["grad_log_std"])
    for slot, bound in b["stats"].items():
        want = ref["stats"][slot]
        if math.isnan(want):
            assert math.isnan(st[slot]), (slot, st[slot])
            continue
        print(f"M={M} A={A} stats[{slot}]: {st[slot]!r} against {want!r}, error / bound {abs(st[slot] - want) / bound if bound else float('nan'):.3f}")
        assert abs(st[slot] - want) <= bound, (slot, st[slot], want, bound)
    i_lo, i_hi = int(torch.where(vb, ref["r"], math.inf).argmin()), int(torch.where(vb, ref["r"], -math.inf).argmax())
    assert abs(st[10] - ref["stats"][10]) <= float(b["r"][i_lo]) and abs(st[11] - ref["stats"][11]) <= float(b["r"][i_hi]), (st[10:12], ref["stats"][10:12])
    return gm, gv, gls, stats


# ---------------------------------------------------------------------------------------------- 1. shapes and widths
CASES = [(M, A) for A in (4, 6) for M in ROWS] + [(BIG3, 4), (BIG8, 4), (BIG8, 6)] + [(M, A) for A in (7, 1) for M in (1, 65, 1000)]


@pytest.mark.parametrize("M, A", CASES)
def test_against_fp64(eng, M, A):
    check_against_fp64(eng, M, A)


@pytest.mark.parametrize("M", (65, 1000, BIG, BIG3))
def test_unaligned_rows_take_the_generic_path_and_agree_bit_for_bit(eng, M):
    x = inputs(M, 4)
    aligned = call(eng, x)
    shifted = {}
    for name in ("mean", "actions"):
        buf = torch.empty(4 * M + 1, dtype=torch.float32, device=DEV)
        view = buf[1:].view(M, 4)
        view.copy_(x[name])
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        shifted[name] = view
    for change in (shifted, dict(mean=shifted["mean"]), dict(actions=shifted["actions"])):
        for p, q in zip(aligned, call(eng, x, **change)):
            assert same_bits(p, q)


# ---------------------------------------------------------------------------------------------- 2. flags and coefficients
@pytest.mark.parametrize("A", (4, 6))
@pytest.mark.parametrize("normalize, vf_coef, ent_coef", [(False, 0.5, 0.01), (True, 0.0, 0.01), (True, 0.5, 0.0), (False, 0.0, 0.0), (False, 1.0, 0.25)])
def test_flags_and_coefficients(eng, A, normalize, vf_coef, ent_coef):
    gm, gv, gls, stats = check_against_fp64(eng, 1000, A, vf_coef=vf_coef, ent_coef=ent_coef, normalize=normalize)
    if vf_coef == 0.0:
        assert not bool(gv.any())
    assert float(stats[8]) > 0 and float(stats[7]) != 0  # (mu and sigma are reported whether or not they are applied)


@pytest.mark.parametrize("M, A", [(65, 4), (1000, 7), (BIG, 4)])
def test_no_mask_equals_a_mask_of_ones(eng, M, A):
    x = inputs(M, A)
    ones = torch.ones(M, dtype=torch.bool, device=DEV)
    a, b, c = call(eng, x, valid=None), call(eng, x, valid=ones), call(eng, x, valid=ones.to(torch.uint8))
    for p, q, r in zip(a, b, c):
        assert same_bits(p, q) and same_bits(p, r)
    assert float(a[3][0]) == M
    check_against_fp64(eng, M, A, valid=None)


# ---------------------------------------------------------------------------------------------- 3. poison, c = 0, determinism
@pytest.mark.parametrize("M, A", [(257, 4), (1000, 6), (BIG, 4), (BIG3, 4), (BIG8, 4)])
def test_poison_in_invalid_rows_reaches_nothing(eng, M, A):
    x = inputs(M, A)
    bad = ~x["valid"]
    assert int(bad.sum()) > M // 8
    clean = call(eng, x)
    poisoned = {}
    for name in ("mean", "actions", "logp_old", "advantages", "returns", "value"):
        t = x[name].clone()
        t[bad] = float("nan")
        poisoned[name] = t
    for p, q in zip(clean, call(eng, x, **poisoned)):
        assert same_bits(p, q)
    shifted = {}  # the same on the generic path
    if A == 4:
        for name in ("mean", "actions"):
            buf = torch.empty(4 * M + 1, dtype=torch.float32, device=DEV)
            shifted[name] = buf[1:].view(M, 4)
            shifted[name].copy_(poisoned[name])
        for p, q in zip(clean, call(eng, x, **{**poisoned, **shifted})):
            assert same_bits(p, q)
    gm, gv = clean[0], clean[1]
    zero_bits = torch.zeros((), dtype=torch.int32, device=DEV)
    assert bool((gm[bad].view(torch.int32) == zero_bits).all()) and bool((gv[bad].view(torch.int32) == zero_bits).all())  # +0, not -0
    assert torch.isfinite(clean[3]).all() and torch.isfinite(clean[2]).all()


@pytest.mark.parametrize("M, A", [(1, 4), (257, 4), (1000, 7)])
def test_no_valid_row(eng, M, A):
    x = inputs(M, A)
    none = torch.zeros(M, dtype=torch.bool, device=DEV)
    nan = {name: torch.full_like(x[name], float("nan")) for name in ("mean", "actions", "logp_old", "advantages", "returns", "value")}
    for change in ({}, nan):
        gm, gv, gls, stats = call(eng, x, valid=none, ent_coef=0.25, **change)
        assert not bool(gm.any()) and not bool(gv.any())
        assert torch.equal(gls, torch.full((A,), -0.25, device=DEV))
        H = float((x["log_std"].double() + (0.5 + HALF_LOG_2PI)).sum())
        st = stats.tolist()
        assert st[0] == 0.0 and st[2] == 0.0 and st[3] == 0.0 and st[5:9] == [0.0] * 4
        assert abs(st[4] - H) <= 1e-14 * (1 + abs(H)) and abs(st[1] + 0.25 * H) <= 1e-14 * (1 + abs(H))
        assert math.isnan(st[9]) and st[10] == math.inf and st[11] == -math.inf and st[12:] == [0.0] * 4


@pytest.mark.parametrize("M, A", [(1000, 4), (BIG, 4), (BIG, 6), (BIG3, 4), (BIG8, 4)])
def test_same_bits_on_every_call_and_stream(eng, M, A):
    x = inputs(M, A)
    first = call(eng, x)
    second = call(eng, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = call(eng, x)
    torch.cuda.current_stream().wait_stream(side)
    for p, q, r in zip(first, second, third):
        assert same_bits(p, q) and same_bits(p, r)


# ---------------------------------------------------------------------------------------------- 4. refusals, through the raw ABI
def test_error_paths_name_the_argument(eng):
    M, A = 65, 4
    x = inputs(M, A)
    out = dict(grad_mean=torch.zeros(M, A, device=DEV), grad_value=torch.zeros(M, device=DEV), grad_log_std=torch.zeros(A, device=DEV),
               stats=torch.zeros(16, dtype=torch.float64, device=DEV))
    scalars = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, normalize_advantage=1)

    def block(**change):
        a = L.PfPpoLoss()
        vals = dict(scalars, **{k: v for k, v in x.items()}, **out)
        for key, val in {**vals, **change}.items():
            setattr(a, key, val if isinstance(val, (float, int)) or val is None else val.data_ptr())
        return a

    def refused(fragment, rows=M, width=A, **change):
        rc = eng.lib.pf_ppo_loss(eng._ctx, C.byref(block(**change)), rows, width, eng._stream())
        msg = eng.lib.pf_last_error(eng._ctx).decode()
        assert rc == L.ERR_ARG and fragment in msg, (rc, msg)

    assert eng.lib.pf_ppo_loss(eng._ctx, C.byref(block()), M, A, eng._stream()) == 0  # (the unchanged block is accepted)
    assert eng.lib.pf_ppo_loss(eng._ctx, C.byref(block(valid=None)), M, A, eng._stream()) == 0
    refused("rows", rows=0)
    refused("width", width=0)
    refused("width", width=9)
    for name in ("mean", "log_std", "actions", "logp_old", "advantages", "returns", "value", "grad_mean", "grad_value", "grad_log_std", "stats"):
        refused(name, **{name: None})
    for bad in (0.0, -0.2, float("nan"), float("inf")):
        refused("clip", clip=bad)
    for name in ("vf_coef", "ent_coef"):
        for bad in (-0.5, float("nan"), float("inf")):
            refused(name, **{name: bad})
    refused("normalize_advantage", normalize_advantage=2)
    assert eng.lib.pf_ppo_loss(None, C.byref(block()), M, A, eng._stream()) == L.ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="actions must be a contiguous"):
        eng.ppo_loss(x["mean"], x["log_std"], x["value"], x["actions"][:, :3], x["logp_old"], x["advantages"], x["returns"])
    # an engine WITH an env task serves as well
    hover = BatchEngine(build_params("quadx", "hover"), 64, device=DEV)
    a, b = call(eng, x), call(hover, x)
    for p, q in zip(a, b):
        assert same_bits(p, q)
    hover.close()


# ---------------------------------------------------------------------------------------------- 5. the autograd wrapper
def hand_written_loss(actor, critic, log_std, obs, x, dtype, vf_coef, ent_coef):
    """What examples/07 writes out by hand (population advantage normalisation, masked means), in `dtype`."""
    v = x["valid"]
    w = v.to(dtype) / v.sum()
    adv = x["advantages"].to(dtype)
    adv = adv - (adv * w).sum()
    adv = adv / (adv.pow(2) * w).sum().sqrt().clamp_min(1e-8)
    o = obs.to(dtype)
    logp = torch.distributions.Normal(actor(o), log_std.exp()).log_prob(x["actions"].to(dtype)).sum(-1)
    ratio = (logp - x["logp_old"].to(dtype)).exp()
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
    value_loss = 0.5 * ((critic(o).squeeze(-1) - x["returns"].to(dtype)).pow(2) * w).sum()
    entropy = (log_std + (0.5 + HALF_LOG_2PI)).sum()
    return -(surrogate * w).sum() + vf_coef * value_loss - ent_coef * entropy


def test_autograd_wrapper_against_the_hand_written_loss(eng):
    M, A, D = 1000, 4, 12
    vf_coef, ent_coef = 0.5, 0.0078125  # (exact in float32)
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(M, D, generator=g).to(DEV)
    nn = torch.nn
    torch.manual_seed(11)
    actor = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, A)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)
    log_std = nn.Parameter(torch.linspace(-0.8, 0.2, A, device=DEV))
    with torch.no_grad():  # a batch whose ratios sit away from the clip bounds under THIS actor, as in inputs()
        mean = actor(obs)
        gi = torch.Generator().manual_seed(6)
        z = ((torch.rand(M, A, generator=gi, dtype=torch.float64) * 2.0 - 1.0) * 3.9).to(DEV)
        actions = (mean.double() + z * log_std.double().exp()).float()
        zz = (actions.double() - mean.double()) * (-log_std.double()).exp()
        logp = (-0.5 * zz * zz - log_std.double() - HALF_LOG_2PI).sum(-1)
        d = torch.tensor(SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=gi)].to(DEV)
        base = inputs(M, A)
        x = dict(actions=actions, logp_old=(logp - d).float(), advantages=base["advantages"], returns=base["returns"], valid=base["valid"])
    import copy

    actor64, critic64, log_std64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), nn.Parameter(log_std.detach().double())

    def grads(params):
        out = [p.grad.double().clone() for p in params]
        for p in params:
            p.grad = None
        return out

    p32 = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    p64 = list(actor64.parameters()) + list(critic64.parameters()) + [log_std64]
    hand_written_loss(actor64, critic64, log_std64, obs, x, torch.float64, vf_coef, ent_coef).backward()
    g64 = grads(p64)
    loss32 = hand_written_loss(actor, critic, log_std, obs, x, torch.float32, vf_coef, ent_coef)
    loss32.backward()
    g32 = grads(p32)
    e32 = max(float((a - b).abs().max()) for a, b in zip(g32, g64))
    kw = dict(clip=CLIP, vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=True)
    loss, stats = pyflyt_amd.ppo_loss(eng, actor(obs), log_std, critic(obs), x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], **kw)
    assert loss.dtype == torch.float32 and loss.shape == () and loss.requires_grad and stats.shape == (16,) and not stats.requires_grad
    loss.backward()
    ours = grads(p32)
    dev = max(float((a - b).abs().max()) for a, b in zip(ours, g64))
    print(f"wrapper: parameter gradients deviate {dev:.3e} from float64, the float32 hand-written loss {e32:.3e}, ratio {dev / e32:.3f}")
    assert dev <= 8.0 * e32, (dev, e32)
    assert abs(float(loss) - float(loss32)) <= 1e-5 * (1.0 + abs(float(loss32)))
    assert pyflyt_amd.ppo_stats_dict(stats)["valid_rows"] == int(x["valid"].sum())
    # a grad_output other than 1 scales the gradients: another float32 evaluation of three times the loss
    loss, _ = pyflyt_amd.ppo_loss(eng, actor(obs), log_std, critic(obs), x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], **kw)
    (3.0 * loss).backward()
    tripled = grads(p32)
    assert max(float((a - 3.0 * b).abs().max()) for a, b in zip(tripled, g64)) <= 8.0 * 3.0 * e32
    assert all(float((a.abs().sum())) > 0 for a in tripled)
    # the gradients wait in the engine's buffers: a backward after the next call is refused, not wrong
    stale, _ = pyflyt_amd.ppo_loss(eng, actor(obs), log_std, critic(obs), x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], **kw)
    pyflyt_amd.ppo_loss(eng, actor(obs), log_std, critic(obs), x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], **kw)
    with pytest.raises(RuntimeError, match="before the next ppo_loss"):
        stale.backward()


# ---------------------------------------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("mode", ("next_step", "same_step"))
def test_collect_feeds_ppo_loss(mode):
    n, k = 1024, 48
    env = make_vec("PyFlyt/QuadX-Hover-v4", n, seed=1, autoreset_mode=mode, max_duration_seconds=1.0)  # (episodes finish inside the batch)
    obs, _ = env.reset(seed=1)
    D = obs.shape[1]
    nn = torch.nn
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, 4)).to(DEV)
    critic = nn.Sequential(nn.Linear(D, 32), nn.Tanh(), nn.Linear(32, 1)).to(DEV)
    log_std = nn.Parameter(torch.full((4,), -0.5, device=DEV))
    policy = MLPPolicy.from_torch(actor, log_std=log_std)
    b = env.collect(policy, critic, k)
    o = b["obs"].reshape(-1, D)
    loss, stats = pyflyt_amd.ppo_loss(env, actor(o), log_std, critic(o), b, clip=CLIP, vf_coef=1.0)
    loss.backward()
    s = pyflyt_amd.ppo_stats_dict(stats)
    assert s["valid_rows"] == int(b["valid"].sum())
    if mode == "next_step":
        assert s["valid_rows"] < n * k  # (reset steps: the mask matters)
    else:
        assert s["valid_rows"] == n * k
    assert all(math.isfinite(s[name]) for name in ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "explained_variance"))
    assert abs(s["approx_kl"]) < 1e-4 and s["clip_fraction"] == 0.0 and abs(s["ratio_min"] - 1.0) < 1e-3 and abs(s["ratio_max"] - 1.0) < 1e-3  # (the policy that acted)
    for p in list(actor.parameters()) + list(critic.parameters()) + [log_std]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    env.close()


def test_example_08_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "08_ppo_fused_loss.py"), "4096", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    num = r"([-+0-9.eE]+|nan|inf)"
    rows = re.findall(rf"loss {num}, approx_kl {num}, clip_fraction {num}, explained variance {num}", out.stdout)
    assert len(rows) == 2 and all(math.isfinite(float(v)) for r in rows for v in r), out.stdout


# ---------------------------------------------------------------------------------------------- 7. capture
def test_ppo_loss_is_capturable(eng):
    M, A = 1000, 4
    x = inputs(M, A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = call(eng, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.ppo_loss(x["mean"], x["log_std"], x["value"], x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"], clip=CLIP,
                           vf_coef=0.5, ent_coef=0.01, normalize_advantage=True)
    for _ in range(2):
        for o in out:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for p, q in zip(out, eager):
            assert same_bits(p, q)
    assert float(eager[3][0]) > 0 and float(eager[0].abs().sum()) > 0
