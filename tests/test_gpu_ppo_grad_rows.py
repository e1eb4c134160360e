"""pf_ppo_grad_rows, BatchEngine.ppo_grad(rows=) and pyflyt_amd.ppo_grad(rows=) on the device.

The reference of every case is BatchEngine.ppo_grad WITHOUT rows= on torch-gathered contiguous copies, t[idx.long()], of the seven
per-row tensors (x, actions, logp_old, advantages, returns, valid, values_old). The comparison is torch.equal on every weight and bias
gradient and on grad_log_std, and the bits of all sixteen stats slots (so the NaN of slot 9 at c = 0 is compared too, and a -0 would
not pass for a +0).

The batch has rows_total = 20 000 rows; m is 1, 63 / 64 / 65 (the ragged tile) and 64 * 256 + 1 = 16 385 (257 tiles on 256 workgroups:
workgroup 0 strides to a second tile, whose rows come through the indices that were loaded a tile ahead). The networks are
test_gpu_ppo_grad.py's five (a second chunk of x at D = 65 and 123). Index lists: the identity over the first m rows, the reverse, a
slice of a seeded permutation, a list with duplicates, m copies of one row."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import pyflyt_amd
from pyflyt_amd import PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine
from test_gpu_ppo_grad import COEF, NETS, case, layers_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTAL = 20000
SIZES = (1, 63, 64, 65, 64 * 256 + 1)
PER_ROW = ("x", "actions", "logp_old", "advantages", "returns", "valid", "values_old")
OPTIONS = ("off", "vclip", "bounds", "both")


@pytest.fixture(scope="module")
def eng():
    e = BatchEngine(build_params("quadx", "none"), 64, device=DEV)
    yield e
    e.close()


_BATCHES = {}


def batch(net, valid="quarter"):
    """The networks' layers, log_std and the TOTAL rows of one (network, valid) case on the device: made once, never changed."""
    key = (net, valid)
    if key not in _BATCHES:
        c = case(TOTAL, net, valid)
        b = {k: (None if c[k] is None else c[k].to(DEV).contiguous()) for k in ("x", "actions", "logp_old", "advantages", "returns", "valid")}
        g = torch.Generator().manual_seed(77 + net)
        b["values_old"] = (c["returns"] + 0.6 * torch.randn(TOTAL, generator=g)).to(DEV)  # (|V - V_old| on both sides of clip_vf = 0.2)
        actor, critic = copy.deepcopy(c["actor"]).to(DEV), copy.deepcopy(c["critic"]).to(DEV)
        _BATCHES[key] = dict(b=b, actor=layers_of(actor), critic=layers_of(critic), log_std=c["log_std"].to(DEV), activation=c["activation"], A=NETS[net][2])
    return _BATCHES[key]


def option_kw(B, b, mode):
    A, kw = B["A"], {}
    if mode in ("vclip", "both"):
        kw.update(clip_vf=0.2, values_old=b["values_old"])
    if mode in ("bounds", "both"):
        kw.update(action_bounds=([-0.05 * (c + 1) for c in range(A)], [0.04 * (c + 1) for c in range(A)]), bounds_coef=0.25)
    return kw


def run(eng, B, b, mode="off", rows=None):
    """[every gradient, grad_log_std, stats] of BatchEngine.ppo_grad on the tensors of b, as copies."""
    ga, gc, gls, stats = eng.ppo_grad(b["x"], B["actor"], B["critic"], B["log_std"], b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"],
                                      actor_activation=B["activation"], critic_activation=B["activation"], rows=rows, **COEF, **option_kw(B, b, mode))
    return [t.clone() for net in (ga, gc) for pair in net for t in pair] + [gls.clone(), stats.clone()]


def gathered(b, idx):
    return {k: (None if b[k] is None else b[k][idx.long()].contiguous()) for k in PER_ROW}


def same(got, want):
    assert len(got) == len(want)
    for i, (u, v) in enumerate(zip(got[:-1], want[:-1])):
        assert torch.equal(u, v), f"output {i} of {len(got)}"
    assert torch.equal(got[-1].view(torch.int64), want[-1].view(torch.int64)), (got[-1].tolist(), want[-1].tolist())


def patterns(m, seed=3):
    """The index lists of the module's docstring, by name, int32 on the device."""
    g = torch.Generator().manual_seed(seed + m)
    perm = torch.randperm(TOTAL, generator=g)
    dup = perm[:m].clone()
    dup[m // 2:] = dup[: m - m // 2].clone()  # (the second half repeats the first: every row but perhaps one is named twice)
    lists = dict(identity=torch.arange(m), reverse=torch.arange(TOTAL - 1, TOTAL - 1 - m, -1), permutation=perm[100:100 + m] if m + 100 <= TOTAL else perm[:m],
                 duplicates=dup, one_row=torch.full((m,), int(perm[0])))
    return {k: v.to(torch.int32).to(DEV).contiguous() for k, v in lists.items()}


# ---------------------------------------------------------------------------------------------- 1. sizes, networks, index lists
@pytest.mark.parametrize("net", range(len(NETS)))
@pytest.mark.parametrize("m", SIZES)
def test_bits_of_the_gathered_call(eng, m, net):
    B = batch(net)
    b = B["b"]
    for name, idx in patterns(m).items():
        got = run(eng, B, b, rows=idx)
        same(got, run(eng, B, gathered(b, idx)))
        assert got[-1][14] == 0.0, name
        if name == "identity":  # (nothing gathered at all: the plain call on the first m rows)
            first = {k: (None if b[k] is None else b[k][:m]) for k in PER_ROW}
            same(got, run(eng, B, first))


@pytest.mark.parametrize("net", [0, 1])
def test_three_tiles_per_workgroup(eng, net):
    """m = 64 * 512 + 1 slots (more than the batch has rows: the list repeats them) are 513 tiles: workgroup 0 walks three, so its third
    tile's indices are the ones requested TWO tiles ahead inside the loop, which no smaller m reaches."""
    B, m = batch(net), 64 * 512 + 1
    idx = torch.randint(0, TOTAL, (m,), generator=torch.Generator().manual_seed(13 + net)).to(torch.int32).to(DEV)
    for mode in ("off", "both"):
        same(run(eng, B, B["b"], mode, rows=idx), run(eng, B, gathered(B["b"], idx), mode))


# ---------------------------------------------------------------------------------------------- 2. validity and the options
@pytest.mark.parametrize("mode", OPTIONS)
@pytest.mark.parametrize("valid", [None, "quarter", "none"])
def test_validity_and_options(eng, valid, mode):
    for net, m in ((0, 65), (1, 64 * 256 + 1), (4, 63)):
        B = batch(net, valid)
        b = B["b"]
        lists = patterns(m, seed=11)
        for name in ("permutation", "duplicates"):
            got = run(eng, B, b, mode, rows=lists[name])
            same(got, run(eng, B, gathered(b, lists[name]), mode))
            s = got[-1].tolist()
            assert s[14] == 0.0 and s[15] == 0.0
            if valid == "none":
                assert s[0] == 0.0 and s[9] != s[9]
            else:
                assert s[0] > 0.0 and (s[12] > 0.0) == (mode in ("vclip", "both")) and (s[13] > 0.0) == (mode in ("bounds", "both"))


# ---------------------------------------------------------------------------------------------- 3. the rows nobody names are not read
@pytest.mark.parametrize("net, m", [(0, 65), (1, 64 * 256 + 1), (2, 64)])
def test_unnamed_rows_are_never_read(eng, net, m):
    B = batch(net)
    b = B["b"]
    for name, idx in patterns(m, seed=5).items():
        named = torch.zeros(TOTAL, dtype=torch.bool, device=DEV)
        named[idx.long()] = True
        p = {}
        for k in PER_ROW:
            p[k] = b[k].clone()
            if k == "valid":
                p[k][~named] = True  # (a byte has no NaN: an unnamed row that were read would be a valid row of NaN)
            else:
                p[k][~named] = float("nan")
        assert bool(torch.isnan(p["x"]).any()) == (int(named.sum()) < TOTAL)
        for mode in ("off", "both"):
            same(run(eng, B, p, mode, rows=idx), run(eng, B, gathered(b, idx), mode))


# ---------------------------------------------------------------------------------------------- 4. indices outside the batch
@pytest.mark.parametrize("valid", ["quarter", None])
@pytest.mark.parametrize("net, m", [(0, 65), (1, 64 * 256 + 1)])
def test_out_of_range_slots_are_invalid_rows_and_counted(eng, net, m, valid):
    """Near misses only: -1, rows_total and rows_total + 1. Every per-row tensor is a view into a larger allocation of this test's own
    with four guard rows of NaN (0xFF for the bytes: valid rows) in front and behind: a dereferenced bad index lands in owned memory
    and shows as a mismatch."""
    B = batch(net, valid)
    b, GUARD = B["b"], 4
    v = dict(b)
    if valid is None:
        v["valid"] = None
    for k in PER_ROW:
        if b[k] is None:
            continue
        big = torch.full((TOTAL + 2 * GUARD, *b[k].shape[1:]), float("nan"), device=DEV) if b[k].dtype == torch.float32 else \
            torch.full((TOTAL + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        view = big[GUARD:GUARD + TOTAL]
        view.copy_(b[k].to(big.dtype))
        assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + GUARD * big[0].numel() * big.element_size()
        v[k] = view
    idx = patterns(m, seed=9)["permutation"].clone()
    slots = [0, m // 2, m - 1] if m == 65 else [5, 63, 64, 8000, 16383, 16384]  # (the second tile of workgroup 0 included)
    bad = [-1, TOTAL, TOTAL + 1]
    for i, s in enumerate(slots):
        idx[s] = bad[i % 3]
    ref_idx = idx.clone()
    ref_idx[slots] = 0
    for mode in ("off", "both"):
        got = run(eng, B, v, mode, rows=idx)
        r = gathered(b, ref_idx)
        r["valid"] = torch.ones(m, dtype=torch.bool, device=DEV) if r["valid"] is None else r["valid"].clone()
        r["valid"][slots] = False
        want = run(eng, B, r, mode)
        assert want[-1][14] == 0.0
        want[-1][14] = float(len(slots))
        same(got, want)
        assert pyflyt_amd.ppo_stats_dict(got[-1], options=True, rows=True)["index_out_of_range"] == len(slots)


# ---------------------------------------------------------------------------------------------- 5. determinism, streams, capture
def test_same_bits_on_every_stream_and_repetition(eng):
    B = batch(0)
    idx = patterns(64 * 256 + 1, seed=21)["permutation"]
    first = run(eng, B, B["b"], "both", rows=idx)
    same(run(eng, B, B["b"], "both", rows=idx), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        second = run(eng, B, B["b"], "both", rows=idx)
    side.synchronize()
    same(second, first)


def test_four_minibatches_in_one_graph(eng):
    B = batch(0)
    b = B["b"]
    parts = pyflyt_amd.minibatches(TOTAL, 4, device=torch.device(DEV), generator=torch.Generator(device=DEV).manual_seed(4))
    assert [p.numel() for p in parts] == [5000] * 4 and all(p.dtype == torch.int32 and p.device == torch.device(DEV) for p in parts)
    assert sorted(torch.cat(parts).tolist()) == list(range(TOTAL))
    eager = [run(eng, B, b, "both", rows=p) for p in parts]
    for e, p in zip(eager, parts):
        same(e, run(eng, B, gathered(b, p), "both"))
    kept = [[torch.empty_like(t) for t in e] for e in eager]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p, out in zip(parts, kept):
            ga, gc, gls, stats = eng.ppo_grad(b["x"], B["actor"], B["critic"], B["log_std"], b["actions"], b["logp_old"], b["advantages"], b["returns"],
                                              valid=b["valid"], actor_activation=B["activation"], critic_activation=B["activation"], rows=p, **COEF,
                                              **option_kw(B, b, "both"))
            for dst, src in zip(out, [t for net in (ga, gc) for pair in net for t in pair] + [gls, stats]):
                dst.copy_(src)
    for _ in range(2):
        for out in kept:
            for t in out:
                t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for out, e in zip(kept, eager):
            same(out, e)


# ---------------------------------------------------------------------------------------------- 6. an epoch of minibatches
def test_an_epoch_of_minibatches_against_gathered_copies(eng):
    c = case(TOTAL, 0, "quarter")
    b = batch(0)["b"]
    nets = [(copy.deepcopy(c["actor"]).to(DEV), copy.deepcopy(c["critic"]).to(DEV), torch.nn.Parameter(c["log_std"].to(DEV))) for _ in range(2)]
    params = [list(a.parameters()) + list(k.parameters()) + [l] for a, k, l in nets]
    opts = [pyflyt_amd.Adam(eng, p, lr=3e-4, max_grad_norm=0.5) for p in params]
    kw = dict(clip_vf=0.2, bounds_coef=0.25, action_bounds=([-0.05] * 4, [0.04] * 4), **COEF)
    for epoch in range(2):
        for idx in pyflyt_amd.minibatches(TOTAL, 3, device=torch.device(DEV), generator=torch.Generator(device=DEV).manual_seed(epoch)):
            (a1, c1, l1), (a2, c2, l2) = nets
            opts[0].zero_grad()
            s1 = pyflyt_amd.ppo_grad(eng, b["x"], a1, c1, l1, b["actions"], b["logp_old"], b["advantages"], b["returns"], valid=b["valid"],
                                     values_old=b["values_old"], rows=idx, **kw)
            opts[0].step()
            g = gathered(b, idx)
            opts[1].zero_grad()
            s2 = pyflyt_amd.ppo_grad(eng, g["x"], a2, c2, l2, g["actions"], g["logp_old"], g["advantages"], g["returns"], valid=g["valid"],
                                     values_old=g["values_old"], **kw)
            opts[1].step()
            assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    for u, v in zip(*params):
        assert torch.equal(u, v)
    assert not torch.equal(params[0][0], c["actor"][0].weight.to(DEV))  # (the steps moved something)


# ---------------------------------------------------------------------------------------------- 7. the refusals that need the device
def test_device_side_refusals(eng):
    B = batch(0)
    b, m = B["b"], 200
    idx = patterns(m)["permutation"]
    run(eng, B, b, rows=idx)  # (the engine's tensors of m rows exist from here on)
    with pytest.raises(ValueError, match=r"rows must be a contiguous int32 tensor of shape \(200,\) on cuda\S*, got torch.int32 \(200,\) on cpu"):
        run(eng, B, b, rows=idx.cpu())
    with pytest.raises(ValueError, match=r"rows must be a contiguous int32 tensor of shape \(200,\) on cuda\S*, got torch.int64"):
        run(eng, B, b, rows=idx.long())
    key = next(k for k in eng._ppo_grad if k != "stats" and k[0] == m and k[1][0] == (64, 21))
    inside = eng._ppo_grad[key]["workspace"].view(torch.int32)[:m]
    with pytest.raises(PyFlytAmdError, match="pf_ppo_grad_rows: row_index and workspace overlap") as e:
        run(eng, B, b, rows=inside)
    assert e.value.code == L.ERR_ARG
    stats = eng._ppo_grad["stats"]
    with pytest.raises(PyFlytAmdError, match="pf_ppo_grad_rows: row_index and stats overlap"):
        run(eng, B, b, rows=stats.view(torch.int32)[:1])
    same(run(eng, B, b, rows=idx), run(eng, B, gathered(b, idx)))  # (and the engine still serves the call)


# ---------------------------------------------------------------------------------------------- 8. the example
def test_example_18_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "18_ppo_minibatches.py"), "256", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("iter ")]
    assert len(lines) == 2 and "nan" not in out.stdout.lower() and all("out of range 0," in l for l in lines)
