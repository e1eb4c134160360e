"""pf_ppo_loss_opt / pf_ppo_grad_opt and their Python layers on the device: value clipping and the bounds loss.

The reference is a float64 restatement of the contract in include/pyflyt_amd.h (pf_ppo_loss's clauses and the two options'), written
from the contract, with gradients from torch.autograd on the same float32 inputs. Per-row gradients: within 8 x the deviation of an
eager torch float32 evaluation from the float64 one. Sums: test_gpu_ppo_loss.py's bounds(), extended by the new terms (below). Exact
where the contract is exact: options off, slot 12, slots 14 / 15, the zero pattern, NaN poisoning, c = 0, alignment, determinism, the
network gradients of the fused call against the composition.

Inputs: test_gpu_ppo_loss.py's, plus values_old = V - e with e from {-0.6, -0.1, 0, 0.1, 0.6} and clip_vf = 0.25: every |e| is at
least 0.15 from the threshold. Rows where the two squared errors are closer than 1e-3 (a thousand times float32's error in these O(1)
quantities) are redrawn, so no branch is decided by rounding; the tests assert it on the float64 reference. Bounds: [-1, 1] on some
columns, one column open below, one fully open; the means are standard normal and fall on both sides. The hinge is continuous, so
it needs no margin."""
import ctypes as C
import math
import os

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import MLPPolicy, PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from pyflyt_amd.gym_envs import make_vec
from test_gpu_mlp import grid_cap
from test_gpu_ppo_grad import COEF, case, layers_of, on_device, params_of, reorder_bounds, sequential
from test_gpu_ppo_loss import BIG, BIG3, CLIP, HALF_LOG_2PI, U32, U64, bounds, f32, gamma_n, inputs, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP_VF, BOUNDS_COEF = 0.25, 0.0625  # (both exact in float32)
E_SHIFTS = (-0.6, -0.1, 0.0, 0.1, 0.6)
MODES = ("vclip", "bounds", "both")


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    yield e
    e.close()


GRAD_BOX = 0.125  # the fused tests' box: a freshly initialised actor's means are a few tenths, and must fall on both sides of it


def box(A, half=1.0):
    """(low, high): [-half, half]; column 2 (mod 4) open below, column 3 (mod 4) fully open."""
    lo = [(-math.inf if c % 4 >= 2 else -half) for c in range(A)]
    hi = [(math.inf if c % 4 == 3 else half) for c in range(A)]
    return lo, hi


def values_old_for(value, returns, g):
    """values_old = V - e on the host in float64, rounded to float32; rows whose two squared errors are within 1e-3 are redrawn (at
    last with e = 0.1: a row inside the clip range compares nothing)."""
    M = value.shape[0]
    V, R = value.double().cpu(), returns.double().cpu()
    e = torch.tensor(E_SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=g)]
    for attempt in range(4):
        vo = (V - e).float().double()
        ee = V - vo
        vc = torch.where(ee > 0, vo + CLIP_VF, vo - CLIP_VF)
        close = (ee.abs() > CLIP_VF) & (((vc - R) ** 2 - (V - R) ** 2).abs() < 1e-3)
        if not bool(close.any()):
            break
        fresh = torch.tensor(E_SHIFTS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=g)] if attempt < 2 else torch.full((M,), 0.1, dtype=torch.float64)
        e = torch.where(close, fresh, e)
    assert not bool(close.any())
    return (V - e).float()


_OPT = {}


def opt_inputs(M, A, seed=0):
    key = (M, A, seed)
    if key not in _OPT:
        x = dict(inputs(M, A, seed))
        g = torch.Generator().manual_seed(77 + M % 1009 + 13 * A + seed)
        x["values_old"] = values_old_for(x["value"], x["returns"], g).to(DEV)
        _OPT[key] = x
    return _OPT[key]


def reference(x, dtype, mode, valid, clip=CLIP, vf_coef=0.5, ent_coef=0.01, normalize=True, clip_vf=CLIP_VF, bounds_coef=BOUNDS_COEF):
    """The contract in `dtype` on the float32 inputs; mu and sigma in float64, handed to the rows as float32 (as the contract says)."""
    clip, vf_coef, ent_coef, clip_vf, bounds_coef = (f32(t) for t in (clip, vf_coef, ent_coef, clip_vf, bounds_coef))
    vclip, bnd = mode in ("vclip", "both"), mode in ("bounds", "both")
    M, A = x["mean"].shape
    v = torch.ones(M, dtype=torch.bool, device=DEV) if valid is None else valid.bool()
    c = int(v.sum())
    w = 1.0 / c if c else 0.0
    zero = torch.zeros((), dtype=dtype, device=DEV)
    mean, log_std, value = (x[k].detach().to(dtype).requires_grad_(True) for k in ("mean", "log_std", "value"))
    act, lpo, adv, ret, vo = (x[k].detach().to(dtype) for k in ("actions", "logp_old", "advantages", "returns", "values_old"))
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
    dv = value - ret
    e = value - vo
    out = (e.abs() > clip_vf) & v
    vc = torch.where(e > 0, vo + clip_vf, vo - clip_vf)  # (no gradient: V_old is data)
    dc = vc - ret
    use_c = out & (dc * dc > dv * dv) if vclip else torch.zeros_like(v)
    sq = torch.where(use_c, dc * dc, dv * dv)
    value_loss = 0.5 * (torch.where(v, sq, zero).sum() * wt)
    H = (log_std + (0.5 + HALF_LOG_2PI)).sum()
    lo, hi = (torch.tensor(t, dtype=dtype, device=DEV) for t in box(A))
    hx, lx = torch.clamp(mean - hi, min=0.0), torch.clamp(lo - mean, min=0.0)
    brow = (hx * hx + lx * lx).sum(-1)
    bounds_loss = torch.where(v, brow, zero).sum() * wt if bnd else zero
    loss = policy_loss + vf_coef * value_loss - ent_coef * H + bounds_coef * bounds_loss
    gm, gv, gls = torch.autograd.grad(loss, [mean, value, log_std])
    with torch.no_grad():
        kl_t = torch.where(v, (r - 1.0) - d, zero)
        clipped = int((v & ((r - 1.0).abs() > clip)).sum())
        rv, dvd = ret.double(), dv.double()
        m_r, m_d = float(torch.where(v, rv, 0.0).sum()) * w, float(torch.where(v, dvd, 0.0).sum()) * w
        var_r = float(torch.where(v, rv * rv, 0.0).sum()) * w - m_r * m_r
        var_d = float(torch.where(v, dvd * dvd, 0.0).sum()) * w - m_d * m_d
        ev = 1.0 - var_d / var_r if var_r != 0.0 else float("nan")
        inf = torch.tensor(float("inf"), dtype=dtype, device=DEV)
        n_out = int(out.sum()) if vclip else 0
        stats = [float(c), float(loss), float(policy_loss), float(value_loss), float(H), float(kl_t.sum() * wt), w * clipped, mu, sigma, ev,
                 float(torch.where(v, r, inf).min()), float(torch.where(v, r, -inf).max()), w * n_out, float(bounds_loss)]
        f64 = lambda t: t.detach().double()  # noqa: E731
        return dict(grad_mean=f64(gm), grad_value=f64(gv), grad_log_std=f64(gls), stats=stats, clipped=clipped, c=c, w=w, valid=v,
                    z=f64(z), logp=f64(logp), d=f64(d), r=f64(r), a=f64(a), surr=f64(surr), dv=f64(dv), ret=f64(ret),
                    adv=a64, kl_t=f64(kl_t), log_std=f64(log_std), live=(u <= vv) & v, var_r=var_r, var_d=var_d,
                    out=out, use_c=use_c & v, e=f64(e), dc=f64(dc), vc=f64(vc), sq=f64(sq), brow=f64(brow), n_out=n_out,
                    outside=((hx > 0) | (lx > 0)).any(-1), hx=f64(hx), lx=f64(lx))


def opt_bounds(ref, M, A, mode, vf_coef, ent_coef, bounds_coef=BOUNDS_COEF):
    """bounds() of test_gpu_ppo_loss.py with the options' terms. With u = 2^-24 and g the double sums' 2 gamma_N:
      value: vc = V_old +- clip_vf is one rounding (u |vc|), dc = vc - R another (u |dc|); the chosen difference x is squared in double:
             |x^2 - exact| <= 2 |x| (u |x| + [use_c] u |vc|) (1 + u). Rows on the unclipped branch keep 2 u x^2.
      bounds: hx, lx one rounding each; a square is two more relative u (3 u); the row's 2 A terms are added in float32: (2 A) u more."""
    b = bounds(ref, M, A, vf_coef, ent_coef)
    v, w, u = ref["valid"], ref["w"], U32
    g = 2.0 * gamma_n(M + 16)
    total = lambda t: float(torch.where(v, t, 0.0).sum())  # noqa: E731
    st = dict(b["stats"])
    b_loss = st[1]
    if mode in ("vclip", "both"):
        x = torch.where(ref["use_c"], ref["dc"], ref["dv"]).abs()
        b_vl = 1.02 * 0.5 * w * (total(2.0 * x * (u * x + torch.where(ref["use_c"], u * ref["vc"].abs(), 0.0))) + g * total(x * x))
        b_loss = b_loss - f32(vf_coef) * st[3] + f32(vf_coef) * b_vl + 8.0 * U64 * abs(ref["stats"][3])
        st[3] = b_vl
    b_bl = 0.0
    if mode in ("bounds", "both"):
        b_bl = 1.02 * w * total(ref["brow"]) * ((3.0 + 2.0 * A) * u + g)
        b_loss = b_loss + f32(bounds_coef) * b_bl + 8.0 * U64 * abs(f32(bounds_coef) * ref["stats"][13])
    st[1], st[13] = b_loss, b_bl
    return dict(b, stats=st)


def options_of(x, A, mode, clip_vf=CLIP_VF, bounds_coef=BOUNDS_COEF, half=1.0):
    kw = {}
    if mode in ("vclip", "both"):
        kw.update(clip_vf=clip_vf, values_old=x["values_old"])
    if mode in ("bounds", "both"):
        kw.update(action_bounds=box(A, half), bounds_coef=bounds_coef)
    return kw


def call(eng, x, mode, valid="own", clip=CLIP, vf_coef=0.5, ent_coef=0.01, normalize=True, **change):
    t = dict(x, **change)
    v = t["valid"] if isinstance(valid, str) else valid
    A = t["mean"].shape[-1]
    kw = options_of(t, A, mode) if mode else {}
    out = eng.ppo_loss(t["mean"], t["log_std"], t["value"], t["actions"], t["logp_old"], t["advantages"], t["returns"], valid=v, clip=clip,
                       vf_coef=vf_coef, ent_coef=ent_coef, normalize_advantage=normalize, **kw)
    out = [o.clone() for o in out]
    torch.cuda.synchronize()
    return out


def check_loss(eng, M, A, mode, vf_coef=0.5, ent_coef=0.01, normalize=True):
    x = opt_inputs(M, A)
    kw = dict(clip=CLIP, vf_coef=vf_coef, ent_coef=ent_coef, normalize=normalize)
    gm, gv, gls, stats = call(eng, x, mode, **kw)
    ref = reference(x, torch.float64, mode, x["valid"], **kw)
    eager = reference(x, torch.float32, mode, x["valid"], **kw)
    vb, st = ref["valid"], stats.tolist()
    # no branch is decided by rounding (on the float64 reference)
    assert float(((ref["e"].abs() - CLIP_VF).abs()).min()) > 0.14
    assert float(torch.where(ref["out"], (ref["dc"] ** 2 - ref["dv"] ** 2).abs(), 1.0).min()) >= 1e-3
    # exact things
    assert st[0] == ref["c"] and st[6] == ref["w"] * ref["clipped"]
    assert st[12] == ref["w"] * ref["n_out"] and round(st[12] * st[0]) == ref["n_out"]
    assert st[14] == 0.0 and st[15] == 0.0
    if mode == "vclip":
        assert st[13] == 0.0
    if mode == "bounds":
        assert st[12] == 0.0
    assert torch.equal(gm != 0, ref["grad_mean"] != 0)
    assert torch.equal(gv == 0, ref["use_c"] | ~vb | (ref["grad_value"] == 0))
    assert not bool(gm[~vb].any()) and not bool(gv[~vb].any()) and not bool(gv[ref["use_c"]].any())
    if M >= 257:
        inside, e = ~ref["out"] & vb, ref["e"]
        if mode != "bounds":
            assert bool(inside.any()) and bool((ref["out"] & (e > 0)).any()) and bool((ref["out"] & (e < 0)).any())
            assert bool(ref["use_c"].any()) and bool((ref["out"] & ~ref["use_c"]).any())
        if mode != "vclip":
            assert bool((ref["hx"] > 0)[vb].any()) and bool((ref["lx"] > 0)[vb].any())
            dead_outside = vb & ~ref["live"] & ref["outside"]  # the surrogate's branch is dead, the bounds term is not
            assert bool(dead_outside.any()) and bool(gm[dead_outside].any(-1).all())
    for name, got in (("grad_mean", gm), ("grad_value", gv)):
        e32 = float((eager[name] - ref[name]).abs().max())
        dev = float((got.double() - ref[name]).abs().max())
        print(f"M={M} A={A} {mode} {name}: device deviation {dev:.3e}, eager float32 deviation {e32:.3e}")
        assert dev <= 8.0 * e32, (name, dev, e32)
    b = opt_bounds(ref, M, A, mode, vf_coef, ent_coef)
    err = (gls.double() - ref["grad_log_std"]).abs()
    assert bool((err <= b["grad_log_std"]).all()), (err, b["grad_log_std"])
    for slot, bound in b["stats"].items():
        want = ref["stats"][slot]
        if math.isnan(want):
            assert math.isnan(st[slot]), (slot, st[slot])
            continue
        print(f"M={M} A={A} {mode} stats[{slot}]: {st[slot]!r} against {want!r}, bound {bound:.3e}")
        assert abs(st[slot] - want) <= bound, (slot, st[slot], want, bound)
    return gm, gv, gls, stats


# ---------------------------------------------------------------------------------------------- 1. pf_ppo_loss_opt
CASES = [(M, A) for A in (4, 6) for M in (1, 63, 64, 65, 257, 1000)] + [(BIG, 6), (BIG3, 4)] + [(M, A) for A in (7, 1) for M in (1, 65, 1000)]


@pytest.mark.parametrize("M, A", CASES)
def test_loss_against_fp64(eng, M, A):
    check_loss(eng, M, A, "both")


@pytest.mark.parametrize("mode", ("vclip", "bounds"))
@pytest.mark.parametrize("M, A", [(257, 4), (1000, 6), (1000, 7)])
def test_each_option_alone(eng, M, A, mode):
    gm, gv, _, _ = check_loss(eng, M, A, mode)
    plain = call(eng, opt_inputs(M, A), None)
    assert same_bits(gm, plain[0]) if mode == "vclip" else same_bits(gv, plain[1])  # (the other option's output is pf_ppo_loss's)


@pytest.mark.parametrize("M, A", [(65, 4), (1000, 6), (BIG3, 4)])
def test_options_off_is_the_existing_function(eng, M, A):
    x = opt_inputs(M, A)
    plain = call(eng, x, None)
    off = [o.clone() for o in eng.ppo_loss(x["mean"], x["log_std"], x["value"], x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"],
                                           clip=CLIP, vf_coef=0.5, ent_coef=0.01, action_bounds=box(A), bounds_coef=0.0)]
    # the raw entry point with an options block whose options are both off, and with no block
    raw = []
    for block in (L.PfPpoOptions(), None):
        outs = [torch.empty_like(t) for t in plain]
        a = L.PfPpoLoss()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = CLIP, 0.5, 0.01, 1
        for name in ("mean", "log_std", "actions", "logp_old", "advantages", "returns", "value", "valid"):
            setattr(a, name, x[name].data_ptr())
        a.grad_mean, a.grad_value, a.grad_log_std, a.stats = (t.data_ptr() for t in outs)
        L.check(eng.lib.pf_ppo_loss_opt(eng._ctx, C.byref(a), None if block is None else C.byref(block), M, A, eng._stream()), eng._ctx)
        torch.cuda.synchronize()
        raw.append(outs)
    for other in (off, *raw):
        for p, q in zip(plain, other):
            assert same_bits(p, q)
    assert plain[3][12:].tolist() == [0.0] * 4


@pytest.mark.parametrize("M", (65, 1000, BIG3))
def test_unaligned_rows_agree_bit_for_bit(eng, M):
    x = opt_inputs(M, 4)
    aligned = call(eng, x, "both")
    shifted = {}
    for name in ("mean", "actions"):
        buf = torch.empty(4 * M + 1, dtype=torch.float32, device=DEV)
        shifted[name] = buf[1:].view(M, 4)
        shifted[name].copy_(x[name])
        assert shifted[name].data_ptr() % 16 == 4
    for p, q in zip(aligned, call(eng, x, "both", **shifted)):
        assert same_bits(p, q)


@pytest.mark.parametrize("M, A", [(257, 4), (1000, 6), (BIG, 6)])
def test_poison_in_invalid_rows_reaches_nothing(eng, M, A):
    x = opt_inputs(M, A)
    bad = ~x["valid"]
    assert int(bad.sum()) > M // 8
    clean = call(eng, x, "both")
    poisoned = {}
    for name in ("values_old", "mean", "value", "returns", "actions"):
        t = x[name].clone()
        t[bad] = float("nan")
        poisoned[name] = t
    for p, q in zip(clean, call(eng, x, "both", **poisoned)):
        assert same_bits(p, q)
    zero_bits = torch.zeros((), dtype=torch.int32, device=DEV)
    assert bool((clean[0][bad].view(torch.int32) == zero_bits).all()) and bool((clean[1][bad].view(torch.int32) == zero_bits).all())


@pytest.mark.parametrize("M, A", [(1, 4), (257, 6)])
def test_no_valid_row(eng, M, A):
    x = opt_inputs(M, A)
    none = torch.zeros(M, dtype=torch.bool, device=DEV)
    nan = {name: torch.full_like(x[name], float("nan")) for name in ("mean", "value", "values_old")}
    for change in ({}, nan):
        gm, gv, gls, stats = call(eng, x, "both", valid=none, ent_coef=0.25, **change)
        assert not bool(gm.any()) and not bool(gv.any())
        assert torch.equal(gls, torch.full((A,), -0.25, device=DEV))
        st = stats.tolist()
        assert st[0] == 0.0 and st[3] == 0.0 and st[12:] == [0.0] * 4


@pytest.mark.parametrize("M, A", [(1000, 4), (BIG, 6)])
def test_same_bits_on_every_call_and_stream(eng, M, A):
    x = opt_inputs(M, A)
    first = call(eng, x, "both")
    for p, q in zip(first, call(eng, x, "both")):
        assert same_bits(p, q)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = call(eng, x, "both")
    for p, q in zip(first, third):
        assert same_bits(p, q)


def _raises(fragment, fn):
    with pytest.raises(PyFlytAmdError) as e:
        fn()
    assert e.value.code == L.ERR_ARG and fragment in str(e.value), str(e.value)


def test_loss_refusals_name_the_argument(eng):
    M, A = 65, 4
    x = opt_inputs(M, A)
    outs = [torch.empty(M, A, device=DEV), torch.empty(M, device=DEV), torch.empty(A, device=DEV), torch.empty(16, dtype=torch.float64, device=DEV)]

    def run(**kw):
        o = L.PfPpoOptions()
        o.clip_vf, o.values_old, o.bounds_coef = CLIP_VF, x["values_old"].data_ptr(), BOUNDS_COEF
        for c in range(8):
            o.bounds_lo[c], o.bounds_hi[c] = -1.0, 1.0
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(o, k)[val[0]] = val[1]
            else:
                setattr(o, k, val)
        a = L.PfPpoLoss()
        a.clip, a.vf_coef, a.ent_coef, a.normalize_advantage = CLIP, 0.5, 0.01, 1
        for name in ("mean", "log_std", "actions", "logp_old", "advantages", "returns", "value", "valid"):
            setattr(a, name, x[name].data_ptr())
        a.grad_mean, a.grad_value, a.grad_log_std, a.stats = (t.data_ptr() for t in outs)
        return lambda: L.check(eng.lib.pf_ppo_loss_opt(eng._ctx, C.byref(a), C.byref(o), M, A, eng._stream()), eng._ctx)

    who = "pf_ppo_loss_opt: "
    for bad in (0.0, -1.0, math.inf, math.nan):
        _raises(who + "clip_vf", run(clip_vf=bad))
    for bad in (-1.0, math.inf, math.nan):
        _raises(who + "bounds_coef", run(bounds_coef=bad))
    _raises(who + "bounds_lo", run(bounds_lo=(1, math.nan)))
    _raises(who + "bounds_hi", run(bounds_hi=(3, math.nan)))
    _raises(who + "bounds_lo must be <= bounds_hi", run(bounds_lo=(2, 2.0)))
    run(bounds_lo=(5, math.nan), clip_vf=CLIP_VF)()  # (a column past A is not read)
    run(clip_vf=math.nan, values_old=None)()         # (clip_vf is read only with values_old)
    torch.cuda.synchronize()


def hand_written(x, mean, log_std, value, mode):
    """A float64 loss written by hand for the autograd wrapper, from the contract's formulas."""
    v, A = x["valid"], mean.shape[-1]
    w = 1.0 / float(v.sum())
    a64 = x["advantages"].double()
    mu = float(a64[v].mean())
    sigma = math.sqrt(float(((a64[v] - mu) ** 2).mean()))
    a = (a64 - f32(mu)) * f32(1.0 / max(sigma, 1e-8))
    z = (x["actions"].double() - mean) * torch.exp(-log_std)
    r = torch.exp((-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1) - x["logp_old"].double())
    surr = torch.minimum(r * a, torch.clamp(r, 1.0 - f32(CLIP), 1.0 + f32(CLIP)) * a)
    R, vo = x["returns"].double(), x["values_old"].double()
    sq = (value - R) ** 2
    if mode != "bounds":
        sq = torch.maximum(sq, (vo + torch.clamp(value - vo, -CLIP_VF, CLIP_VF) - R) ** 2)  # SB3's form: the same thing where no row sits on a threshold
    lo, hi = (torch.tensor(t, dtype=torch.float64, device=DEV) for t in box(A))
    b = (torch.clamp(mean - hi, min=0) ** 2 + torch.clamp(lo - mean, min=0) ** 2).sum(-1)
    loss = -w * surr[v].sum() + f32(0.5) * 0.5 * w * sq[v].sum() - f32(0.01) * (log_std + 0.5 + HALF_LOG_2PI).sum()
    return loss + (BOUNDS_COEF * w * b[v].sum() if mode != "vclip" else 0.0)


@pytest.mark.parametrize("mode", MODES)
def test_autograd_wrapper_against_a_hand_written_loss(eng, mode):
    M, A = 1000, 6
    x = {k: v.detach() for k, v in opt_inputs(M, A).items()}
    leaves = [x[k].clone().requires_grad_(True) for k in ("mean", "log_std", "value")]
    kw = options_of(x, A, mode)
    loss, stats = pyflyt_amd.ppo_loss(eng, leaves[0], leaves[1], leaves[2], x["actions"], x["logp_old"], x["advantages"], x["returns"], valid=x["valid"],
                                      clip=CLIP, vf_coef=0.5, ent_coef=0.01, **kw)
    (2.0 * loss).backward()  # (backward scales the option gradients as it does the others; a factor of 2 is exact)
    ref = [x[k].double().requires_grad_(True) for k in ("mean", "log_std", "value")]
    want = hand_written(x, *ref, mode)
    want.backward()
    # the hand-written float64 loss and the restated contract are the same function: their gradients agree to float64's rounding
    r64 = reference(x, torch.float64, mode, x["valid"])
    r32 = reference(x, torch.float32, mode, x["valid"])
    for r, name in zip(ref, ("grad_mean", "grad_log_std", "grad_value")):
        assert float((r.grad - r64[name]).abs().max()) <= 1e-12 * (1.0 + float(r64[name].abs().max())), name
    bnd = opt_bounds(r64, M, A, mode, 0.5, 0.01)
    assert abs(float(loss.detach()) - float(want)) <= bnd["stats"][1] + 2.0 ** -23 * abs(float(want))  # (the sum's bound and the float32 scalar)
    # the wiring: what backward() hands out is the engine's own tensors, scaled
    gm, gv, gls, _ = call(eng, x, mode)
    assert torch.equal(leaves[0].grad, 2.0 * gm) and torch.equal(leaves[2].grad, 2.0 * gv) and torch.equal(leaves[1].grad, 2.0 * gls)
    # per-row gradients: 8 x the eager float32 evaluation's own deviation; grad_log_std: the sums' bound
    for got, name in ((leaves[0], "grad_mean"), (leaves[2], "grad_value")):
        e32 = float((r32[name] - r64[name]).abs().max())
        dev = float((0.5 * got.grad.double() - r64[name]).abs().max())
        assert dev <= 8.0 * e32, (name, dev, e32)
    assert bool(((0.5 * leaves[1].grad.double() - r64["grad_log_std"]).abs() <= bnd["grad_log_std"]).all())
    d = pyflyt_amd.ppo_stats_dict(stats, options=True)
    assert len(d) == 14 and len(pyflyt_amd.ppo_stats_dict(stats)) == 12
    assert (d["value_clip_fraction"] > 0) == (mode != "bounds") and (d["bounds_loss"] > 0) == (mode != "vclip")


# ---------------------------------------------------------------------------------------------- 2. pf_ppo_grad_opt
GRAD_NETS = (0, 2)  # test_gpu_ppo_grad.py's NETS: Hover's D = 21, A = 4 and the dogfight's D = 123, A = 6


def grad_case(eng, rows, net):
    """test_gpu_ppo_grad.py's case with values_old = V - e, V the critic's float64 forward."""
    c = case(rows, net, "quarter")
    if "values_old" not in c:
        import copy
        with torch.no_grad():
            V = copy.deepcopy(c["critic"]).double()(c["x"].double()).squeeze(-1)
        c["values_old"] = values_old_for(V, c["returns"], torch.Generator().manual_seed(rows + net))
    return c


def big_rows(eng, net):
    c = case(1, net, "quarter")
    return 64 * (2 * grid_cap(eng, [(w.to(DEV), b.to(DEV)) for w, b in layers_of(c["actor"])]) + 1) + 37


def run_grad(eng, actor, critic, log_std, b, activation, mode, values_old, fused, coef=COEF):
    A = log_std.shape[0]
    kw = options_of(dict(values_old=values_old), A, mode, half=GRAD_BOX) if mode else {}
    ps = params_of(actor, critic, log_std)
    for p in ps:
        p.grad = None
    mean = value = None
    if fused:
        stats = pyflyt_amd.ppo_grad(eng, b["x"], actor, critic, log_std, b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"], **coef, **kw)
    else:
        mean, value = pyflyt_amd.mlp(eng, b["x"], actor), pyflyt_amd.mlp(eng, b["x"], critic)
        loss, stats = pyflyt_amd.ppo_loss(eng, mean, log_std, value, b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"], **coef, **kw)
        loss.backward()
    grads = [p.grad.clone() for p in ps]
    torch.cuda.synchronize()
    return (grads, stats.clone()) if fused else (grads, stats.clone(), mean.detach(), value.detach())


def opt_reorder_bounds(b, log_std, mean, value, values_old, stats, coef, mode):
    """test_gpu_ppo_grad.py's reorder_bounds (per slot M 2^-53 w sum |t_i| over the actual per-row terms, in float64 on the host from
    the composed path's means and values, plus 8 ulps; per column for grad_log_std) extended by the two new raw sums: the chosen
    square of the value loss replaces (V - R)^2 in slots 3 and 1 (slot 9 keeps (V - R)^2: reorder_bounds' own), and the row term b of
    the bounds loss enters slots 13 and 1 (bounds_coef times it). grad_log_std has no new term."""
    bound, gb = reorder_bounds(b, log_std, mean, value, stats, coef)
    M, A = mean.shape
    v = torch.ones(M, dtype=torch.bool, device=DEV) if b["valid"] is None else b["valid"].bool()
    c = float(v.sum())
    w = 1.0 / c if c else 0.0
    k = M * U64
    sabs = lambda t: float(torch.where(v, t.abs(), 0.0).sum())  # noqa: E731
    V, R, vo = value.double().reshape(-1), b["returns"].double(), values_old.double()
    b1 = bound[1]
    if mode in ("vclip", "both"):
        e, dv = V - vo, V - R
        vc = torch.where(e > 0, vo + CLIP_VF, vo - CLIP_VF)
        dc = vc - R
        sq = torch.where((e.abs() > CLIP_VF) & (dc * dc > dv * dv), dc * dc, dv * dv)
        b3 = 0.5 * w * k * sabs(sq) + 8.0 * U64 * w * sabs(sq)
        b1 = b1 - coef["vf_coef"] * bound[3] + coef["vf_coef"] * b3 + 8.0 * U64 * w * sabs(sq)
        bound[3] = b3
    if mode in ("bounds", "both"):
        lo, hi = (torch.tensor(t, dtype=torch.float64, device=DEV) for t in box(A, GRAD_BOX))
        m = mean.double()
        if M >= 63:  # means fall on both sides of the box: the bounds term is live in this comparison
            assert bool((m > hi)[v].any()) and bool((m < lo)[v].any())
        brow = (torch.clamp(m - hi, min=0.0) ** 2 + torch.clamp(lo - m, min=0.0) ** 2).sum(-1)
        bound[13] = w * k * sabs(brow) + 8.0 * U64 * w * sabs(brow)
        b1 = b1 + f32(BOUNDS_COEF) * bound[13] + 8.0 * U64 * f32(BOUNDS_COEF) * w * sabs(brow)
    bound[1] = b1
    return bound, gb


@pytest.mark.parametrize("net", GRAD_NETS)
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 129, "cap"])
def test_fused_call_equals_the_composition(eng, rows, net):
    rows = big_rows(eng, net) if rows == "cap" else rows
    c = grad_case(eng, rows, net)
    actor, critic, log_std, b = on_device(c)
    vo = c["values_old"].to(DEV)
    for mode in (MODES if rows in (65, 129) else ("both",)):
        want, ws, mean, value = run_grad(eng, actor, critic, log_std, b, c["activation"], mode, vo, fused=False)
        bound, gb = opt_reorder_bounds(b, log_std, mean, value, vo, ws, COEF, mode)
        got, gs = run_grad(eng, actor, critic, log_std, b, c["activation"], mode, vo, fused=True)
        for g, w in zip(got[:-1], want[:-1]):
            assert torch.equal(g, w), float((g - w).abs().max())
        gs, ws = gs.tolist(), ws.tolist()
        for slot in (0, 4, 6, 7, 8, 10, 11, 12, 14, 15):
            assert gs[slot] == ws[slot], (slot, gs[slot], ws[slot])
        # the summed outputs: test_gpu_ppo_grad.py's reordering bound, extended by the options' sums
        for slot in (1, 2, 3, 5, 9, 13):
            if math.isnan(ws[slot]):
                assert math.isnan(gs[slot]), (slot, gs[slot])
                continue
            print(f"rows {rows} net {net} {mode} stats[{slot}]: {abs(gs[slot] - ws[slot]):.2e} <= {bound[slot]:.2e}")
            assert abs(gs[slot] - ws[slot]) <= bound[slot], (slot, gs[slot], ws[slot], bound[slot])
        if mode == "vclip":
            assert gs[13] == 0.0 and ws[13] == 0.0
        elif rows >= 63:
            assert ws[13] > 0.0
        for cix, (g, w) in enumerate(zip(got[-1].tolist(), want[-1].tolist())):
            lim = gb[cix] + 2.0 ** -23 * abs(w)  # (one float32 ulp of the result)
            assert abs(g - w) <= lim, (cix, g, w, lim)
    # options off: the existing call, bit for bit
    plain, ps_ = run_grad(eng, actor, critic, log_std, b, c["activation"], None, vo, fused=True)
    kw = dict(action_bounds=box(log_std.shape[0]), bounds_coef=0.0)
    for p in params_of(actor, critic, log_std):
        p.grad = None
    off = pyflyt_amd.ppo_grad(eng, b["x"], actor, critic, log_std, b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"], **COEF, **kw)
    for p, q in zip(plain, [p.grad for p in params_of(actor, critic, log_std)]):
        assert torch.equal(p, q)
    assert same_bits(off, ps_) and off[12:].tolist() == [0.0] * 4


def test_fused_call_poison_determinism_and_refusals(eng):
    rows, net = 129, 0
    c = grad_case(eng, rows, net)
    actor, critic, log_std, b = on_device(c)
    vo = c["values_old"].to(DEV)
    first, s1 = run_grad(eng, actor, critic, log_std, b, c["activation"], "both", vo, fused=True)
    bad = ~b["valid"]
    vo_nan = vo.clone()
    vo_nan[bad] = float("nan")
    second, s2 = run_grad(eng, actor, critic, log_std, b, c["activation"], "both", vo_nan, fused=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third, s3 = run_grad(eng, actor, critic, log_std, b, c["activation"], "both", vo, fused=True)
    for other, s in ((second, s2), (third, s3)):
        assert same_bits(s1, s)
        for p, q in zip(first, other):
            assert same_bits(p, q)
    la, lc = layers_of(actor), layers_of(critic)
    args = (b["x"], la, lc, log_std.detach(), b["actions"], b["logp_old"], b["advantages"], b["returns"])
    mine = eng._ppo_grad[(rows, *(tuple((int(w.shape[0]), int(w.shape[1])) for w, _ in ls) for ls in (la, lc)))]  # this call's outputs and workspace
    _raises("pf_ppo_grad_opt: values_old and workspace overlap", lambda: eng.ppo_grad(*args, valid=b["valid"], clip_vf=CLIP_VF,
                                                                                      values_old=mine["workspace"].view(torch.float32)[:rows]))
    _raises("pf_ppo_grad_opt: values_old and actor_grad_w[0] overlap", lambda: eng.ppo_grad(*args, valid=b["valid"], clip_vf=CLIP_VF,
                                                                                            values_old=mine["grads"][0][0][0].view(-1)[:rows]))
    # the library's own refusals of the options (the Python layer refuses first, so these go in raw)
    qa, qc = eng._mlp_block(b["x"], la, c["activation"])[0], eng._mlp_block(b["x"], lc, c["activation"])[0]
    a = mine["args"]
    a.actor, a.critic = C.addressof(qa), C.addressof(qc)
    for field, val, text in (("clip_vf", 0.0, "clip_vf must be finite and > 0"), ("clip_vf", math.inf, "clip_vf must be finite and > 0"),
                             ("bounds_coef", -1.0, "bounds_coef must be finite and >= 0"), ("bounds_coef", math.nan, "bounds_coef must be finite and >= 0"),
                             ("bounds_lo", (1, math.nan), "bounds_lo must not hold a NaN"), ("bounds_lo", (2, 2.0), "bounds_lo must be <= bounds_hi")):
        o = L.PfPpoOptions()
        o.clip_vf, o.values_old, o.bounds_coef = CLIP_VF, vo.data_ptr(), BOUNDS_COEF
        for col in range(8):
            o.bounds_lo[col], o.bounds_hi[col] = -1.0, 1.0
        if isinstance(val, tuple):
            getattr(o, field)[val[0]] = val[1]
        else:
            setattr(o, field, val)
        _raises("pf_ppo_grad_opt: " + text, lambda: L.check(eng.lib.pf_ppo_grad_opt(eng._ctx, C.byref(a), C.byref(o), rows, mine["workspace"].data_ptr(), mine["bytes"],
                                                                                    eng._stream()), eng._ctx))
    for kw, text in ((dict(clip_vf=0.0, values_old=vo), "clip_vf"), (dict(clip_vf=CLIP_VF), "values_old"), (dict(values_old=vo), "values_old comes with clip_vf"),
                     (dict(bounds_coef=-1.0, action_bounds=box(4)), "bounds_coef"), (dict(bounds_coef=0.1), "action_bounds is required"),
                     (dict(bounds_coef=0.1, action_bounds=([0.0] * 3, [1.0] * 3)), "action_bounds"),
                     (dict(bounds_coef=0.1, action_bounds=([2.0] * 4, [1.0] * 4)), "low must be <= high"),
                     (dict(bounds_coef=0.1, action_bounds=([math.nan] * 4, [1.0] * 4)), "NaN")):
        with pytest.raises(ValueError, match=text):
            eng.ppo_grad(*args, valid=b["valid"], **kw)


# ---------------------------------------------------------------------------------------------- 3. from collect()
def _policy(env, A, D):
    torch.manual_seed(5)
    actor, critic = sequential([D, 64, 64, A], "tanh").to(DEV), sequential([D, 64, 1], "tanh").to(DEV)
    log_std = torch.nn.Parameter(torch.full((A,), -0.5, device=DEV))
    return actor, critic, log_std


@pytest.mark.parametrize("autoreset", ("next_step", "same_step"))
def test_collect_to_ppo_grad_with_options_on_hover(autoreset):
    env = make_vec("PyFlyt/QuadX-Hover-v4", num_envs=256, device=DEV, seed=3, autoreset_mode=autoreset, max_duration_seconds=0.5)
    try:
        env.reset(seed=3)
        D, A = env.single_observation_space.shape[0], env.single_action_space.shape[0]
        actor, critic, log_std = _policy(env, A, D)
        policy = MLPPolicy.from_torch(actor, log_std=log_std)
        batch = env.collect(policy, critic, 24)  # (20-step episodes)
        x = batch["obs"].reshape(-1, D)
        stats = pyflyt_amd.ppo_grad(env, x, actor, critic, log_std, batch, clip_vf=0.2, action_bounds=(env.single_action_space.low, env.single_action_space.high),
                                    bounds_coef=1e-4)
        d = pyflyt_amd.ppo_stats_dict(stats, options=True)
        assert d["valid_rows"] == int(batch["valid"].sum()) and math.isfinite(d["loss"])
        assert bool(batch["terminated"].any() | batch["truncated"].any())  # (episodes end inside the batch: the mode matters)
        assert d["value_clip_fraction"] == 0.0  # (the first epoch: the new values are the batch's)
        assert d["bounds_loss"] >= 0.0 and all(torch.isfinite(p.grad).all() for p in params_of(actor, critic, log_std))
    finally:
        env.close()


def test_collect_to_ppo_grad_with_options_on_the_dogfight_with_an_opponent():
    from test_gpu_ma_collect import env_policy, make_env

    env = make_env(("dogfight", 2, 16))
    try:
        D, A = env.engine.obs_dim, env.engine.action_dim
        actor, critic, log_std = _policy(env, A, D)
        policy = MLPPolicy.from_torch(actor, log_std=log_std)
        batch = env.collect(policy, critic, 16, opponent=env_policy(env, seed=9))
        sp = env.action_space(env.possible_agents[0])
        stats = pyflyt_amd.ppo_grad(env, batch["obs"].reshape(-1, D), actor, critic, log_std, batch, clip_vf=0.2, action_bounds=(sp.low, sp.high), bounds_coef=1e-4)
        d = pyflyt_amd.ppo_stats_dict(stats, options=True)
        assert 0 < d["valid_rows"] == int(batch["valid"].sum()) < batch["valid"].numel() and math.isfinite(d["loss"])
        assert d["value_clip_fraction"] == 0.0 and d["bounds_loss"] >= 0.0
        assert all(torch.isfinite(p.grad).all() for p in params_of(actor, critic, log_std))
    finally:
        env.close()
