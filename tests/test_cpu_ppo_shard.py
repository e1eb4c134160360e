"""The host side of the sharded PPO calls (pf_ppo_adv_sums, pf_adv_sums_add, pf_ppo_grad_shard, pf_ppo_shard_combine, pf_moments_merge):
the header's text, the bindings, the refusals of the C functions that need no device (a NULL ctx, bad scalars), and what the Python
layer refuses before it reaches a device: make_vec(devices=...), Replicas, ppo_grad_sharded's lists, the engine methods' tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from bare_engine import bare_engine
import pyflyt_amd
from pyflyt_amd import _lib as L
from pyflyt_amd.gym_envs import make_vec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 31) - 64
NAMES = ("pf_ppo_adv_sums", "pf_adv_sums_add", "pf_ppo_grad_shard", "pf_ppo_shard_combine", "pf_moments_merge", "pf_sizeof_ppo_shard_combine")


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "pyflyt_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"int\s+pf_ppo_adv_sums\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+float\s*\*\s*advantages\s*,\s*const\s+uint8_t\s*\*\s*valid\s*,"
                     r"\s*const\s+int32_t\s*\*\s*row_index\s*,\s*int64_t\s+m,\s*int64_t\s+rows_total,\s*double\s*\*\s*sums\s*,\s*void\s*\*\s*stream\s*\)", bare)
    assert re.search(r"int\s+pf_ppo_grad_shard\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_ppo_grad_args\s*\*\s*\w+,\s*const\s+pf_ppo_options\s*\*\s*\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*row_index\s*,\s*int64_t\s+m,\s*int64_t\s+rows_total,\s*const\s+double\s*\*\s*adv_sums\s*,"
                     r"\s*double\s*\*\s*shard_block\s*,\s*void\s*\*\s*workspace,\s*size_t\s+workspace_bytes,\s*void\s*\*\s*stream\s*\)", bare)
    assert re.search(r"int\s+pf_ppo_shard_combine\s*\(\s*pf_ctx\s*\*\s*\w+,\s*const\s+pf_ppo_shard_combine_args\s*\*\s*\w+,\s*void\s*\*\s*stream\s*\)", bare)
    assert re.search(r"int\s+pf_adv_sums_add\s*\(\s*pf_ctx\s*\*\s*\w+,\s*double\s*\*\s*dst\s*,\s*const\s+double\s*\*\s*const\s+src\[\]\s*,\s*int\s+n_src,\s*void\s*\*\s*stream\s*\)", bare)
    assert re.search(r"int\s+pf_moments_merge\s*\(\s*pf_ctx\s*\*\s*\w+,\s*double\s*\*\s*dst\s*,\s*const\s+double\s*\*\s*const\s+src\[\]\s*,\s*int\s+n_src,\s*int\s+D,"
                     r"\s*void\s*\*\s*stream\s*\)", bare)
    contract = text.split("#define PF_PPO_MAX_SHARDS")[0].rsplit("SHARDED PPO", 1)[1]
    for fragment in ("weights its\n * rows by 1 / (its own valid count)", "come from ALL shards", "no collective", "no atomics", "in the same order before they divide",
                     "a->stats and a->grad_log_std must be NULL", "7 min r", "9..16 the sums behind grad_log_std", "20 this shard's valid count",
                     "21 its out-of-range slots", "SHARE of the joint gradient", "pf_ppo_grad_workspace_bytes(actor, critic, m)", "ascending shard order",
                     "ONE flat contiguous buffer of numel floats", "With ONE shard every", "bits of pf_ppo_grad_rows", "slot 14 the sum of the shards' out-of-range counts",
                     "A block with count 0 merges as nothing", "copied, bit for bit", "Added\n * without a new PF_ABI_VERSION"):
        assert fragment in contract, fragment
    assert "#define PF_ABI_VERSION 10" in text and L.PF_ABI_VERSION == 10
    assert L.PF_PPO_MAX_SHARDS == 16 and L.PF_PPO_SHARD_WORDS == 24
    for name in NAMES:
        assert name in L.EXPORTS


def test_bindings():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} is not built")
    lib, raw = L.lib(), C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
    assert lib.pf_abi_version() == 10
    assert lib.pf_sizeof_ppo_shard_combine() == C.sizeof(L.PfPpoShardCombine)
    fields = dict(L.PfPpoShardCombine._fields_)
    assert C.sizeof(fields["blocks"]) == C.sizeof(fields["grads"]) == 16 * C.sizeof(C.c_void_p)
    vp, i64 = C.c_void_p, C.c_int64
    assert list(lib.pf_ppo_adv_sums.argtypes) == [vp, vp, vp, vp, i64, i64, vp, vp]
    assert list(lib.pf_adv_sums_add.argtypes) == [vp, vp, C.POINTER(vp), C.c_int, vp]
    assert list(lib.pf_moments_merge.argtypes) == [vp, vp, C.POINTER(vp), C.c_int, C.c_int, vp]
    assert list(lib.pf_ppo_grad_shard.argtypes) == [vp, C.POINTER(L.PfPpoGradArgs), C.POINTER(L.PfPpoOptions), vp, i64, i64, vp, vp, vp, C.c_size_t, vp]
    assert list(lib.pf_ppo_shard_combine.argtypes) == [vp, C.POINTER(L.PfPpoShardCombine), vp]


def test_c_functions_refuse_bad_scalars_and_a_null_ctx():
    lib = L.lib()
    err = lambda: lib.pf_last_error(None).decode()  # noqa: E731
    buf = (C.c_double * 64)()  # (never read: every call here is refused on the host)
    p = C.cast(buf, C.c_void_p)
    src = (C.c_void_p * 16)(*([p.value] * 16))
    g, a = L.PfPpoGradArgs(), L.PfPpoShardCombine()
    for m, text in ((0, "m must be >= 1"), (-1, "m must be >= 1"), (BIG, "m must be below 2^31 - 64"), (4, "ctx is required")):
        assert lib.pf_ppo_adv_sums(None, p, None, None, m, 8, p, None) == L.ERR_ARG and err().startswith("pf_ppo_adv_sums: " + text), err()
        assert lib.pf_ppo_grad_shard(None, C.byref(g), None, None, m, 8, p, p, None, 0, None) == L.ERR_ARG
        assert err().startswith("pf_ppo_grad_shard: " + text), err()
    assert lib.pf_ppo_grad_shard(None, C.byref(g), None, p, 4, 0, p, p, None, 0, None) == L.ERR_ARG and err().startswith("pf_ppo_grad_shard: rows_total must be >= 1")
    for n in (0, 17, -1):
        a.n_shards = n
        assert lib.pf_ppo_shard_combine(None, C.byref(a), None) == L.ERR_ARG and err() == "pf_ppo_shard_combine: n_shards must be in 1..PF_PPO_MAX_SHARDS (16)"
        assert lib.pf_adv_sums_add(None, p, src, n, None) == L.ERR_ARG and err() == "pf_adv_sums_add: n_src must be in 1..PF_PPO_MAX_SHARDS (16)"
        assert lib.pf_moments_merge(None, p, src, n, 1, None) == L.ERR_ARG and err() == "pf_moments_merge: n_src must be in 1..PF_PPO_MAX_SHARDS (16)"
    for D in (0, 129, -5):
        assert lib.pf_moments_merge(None, p, src, 1, D, None) == L.ERR_ARG and err() == "pf_moments_merge: D must be in 1..128"
    a.n_shards = 2
    assert lib.pf_ppo_shard_combine(None, C.byref(a), None) == L.ERR_ARG and err() == "pf_ppo_shard_combine: ctx is required"
    assert lib.pf_ppo_shard_combine(None, None, None) == L.ERR_ARG and err() == "pf_ppo_shard_combine: ctx is required"
    assert lib.pf_adv_sums_add(None, p, src, 16, None) == L.ERR_ARG and err() == "pf_adv_sums_add: ctx is required"
    assert lib.pf_moments_merge(None, p, src, 1, 128, None) == L.ERR_ARG and err() == "pf_moments_merge: ctx is required"
    assert lib.pf_ppo_grad_rows(None, C.byref(g), None, p, 4, 8, None, 0, None) == L.ERR_ARG and err() == "pf_ppo_grad_rows: ctx is required"  # (as it was)


def test_make_vec_refuses_bad_device_lists():
    with pytest.raises(ValueError, match="devices must name at least one device"):
        make_vec("PyFlyt/QuadX-Hover-v4", 8, devices=[])
    with pytest.raises(ValueError, match=r"num_envs must be an int of at least one env per device \(3\), got 2"):
        make_vec("PyFlyt/QuadX-Hover-v4", 2, devices=["cuda:0", "cuda:0", "cuda:0"])
    with pytest.raises(ValueError, match="devices must be a list of devices"):
        make_vec("PyFlyt/QuadX-Hover-v4", 8, devices=3)
    with pytest.raises(ValueError, match="device comes with a plain make_vec"):
        make_vec("PyFlyt/QuadX-Hover-v4", 8, devices=["cuda:0"], device="cuda:0")
    with pytest.raises(KeyError):
        make_vec("PyFlyt/Rocket-Landing-v4", 8, devices=["cuda:0"])


def nets(A=4, D=21):
    nn = torch.nn
    return dict(actor=nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, A)), critic=nn.Sequential(nn.Linear(D, 8), nn.Tanh(), nn.Linear(8, 1)),
                log_std=nn.Parameter(torch.zeros(A)))


def test_replicas_on_one_device_are_the_masters():
    m = nets()
    rep = pyflyt_amd.Replicas(m, ["cpu", "cpu"])
    assert len(rep) == 2 and rep[0] is rep[1] and rep[1]["actor"] is m["actor"] and rep.devices == [torch.device("cpu")] * 2
    rep.sync()  # (nothing to copy)
    assert "Replicas" in pyflyt_amd.__all__ and "ppo_grad_sharded" in pyflyt_amd.__all__
    for modules, devices, text in (({}, ["cpu"], "modules must be a non-empty dict"), (m, [], "devices must name at least one device"),
                                   (m, 3, "devices must be a list of devices"), (dict(actor=3), ["cpu"], r"modules\['actor'\] must be a torch.nn.Module or a tensor"),
                                   (m, ["meta", "cpu"], r"modules\['actor'\] must live on devices\[0\] \(meta\)")):
        with pytest.raises(ValueError, match=text):
            pyflyt_amd.Replicas(modules, devices)
    meta = pyflyt_amd.Replicas(m, ["cpu", "meta"])  # (a second device that needs no hardware: copies are made, of the masters' shapes)
    assert meta[1]["actor"] is not m["actor"] and meta[1]["actor"][0].weight.device.type == "meta" and meta[1]["log_std"].shape == (4,)
    assert len(meta._pairs) == 9


def test_ppo_grad_sharded_checks_its_lists():
    eng, M, A = bare_engine(), 6, 4
    rep = pyflyt_amd.Replicas(nets(A), ["cpu", "cpu"])
    xs = [torch.zeros(M, 21)] * 2
    batches = [(torch.zeros(M, A), torch.zeros(M), torch.zeros(M), torch.zeros(M))] * 2
    call = pyflyt_amd.ppo_grad_sharded
    for kw, text in ((dict(xs=xs[:1]), r"xs must be a list with one entry per shard \(2\), got 1"), (dict(batches=batches * 2), r"batches must be a list with one entry per shard \(2\), got 4"),
                     (dict(rows=[None]), r"rows must be a list with one entry per shard \(2\), got 1"), (dict(valid=torch.zeros(M)), r"valid must be a list with one entry per shard \(2\), got Tensor"),
                     (dict(xs=None), "xs and batches are required"), (dict(rep=3), "rep must be a Replicas, got int"),
                     (dict(rep=pyflyt_amd.Replicas(nets(A), ["cpu"])), "rep holds 1 devices, the env 2 shards"),
                     (dict(env=[eng, 5]), r"shards\[1\] must be a vector env or a BatchEngine, got int"),
                     (dict(rep=pyflyt_amd.Replicas(nets(A), ["cpu", "meta"])), r"shards\[1\] lives on cpu, rep\[1\] on meta"),
                     (dict(rep=pyflyt_amd.Replicas(dict(actor=nets(A)["actor"]), ["cpu", "cpu"])), r"rep lacks \['critic', 'log_std'\]"),
                     (dict(rows=[torch.zeros(4, dtype=torch.int64), None]), r"rows must be a contiguous int32 tensor of shape \(4,\) on cpu, got torch.int64"),
                     (dict(clip=0.0), "clip must be finite and > 0")):
        args = dict(env=[eng, eng], xs=xs, rep=rep, batches=batches)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            call(args.pop("env"), args.pop("xs"), args.pop("rep"), args.pop("batches"), **args)


def test_engine_methods_check_their_tensors():
    eng = bare_engine()
    f64 = torch.float64
    with pytest.raises(ValueError, match="advantages must be a float32 tensor with at least one axis, got list"):
        eng.ppo_adv_sums([1.0])
    with pytest.raises(ValueError, match=r"valid must be a contiguous torch.bool/torch.uint8 tensor of shape \(6,\)"):
        eng.ppo_adv_sums(torch.zeros(6), valid=torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="rows must be a 1-D int32 tensor of row numbers"):
        eng.ppo_adv_sums(torch.zeros(6), rows=[0, 1])
    with pytest.raises(ValueError, match=r"out must be a contiguous float64 tensor of shape \(4,\)"):
        eng.ppo_adv_sums(torch.zeros(6), out=torch.zeros(4))
    with pytest.raises(ValueError, match=r"blocks must be a list of 1..16 tensors \(PF_PPO_MAX_SHARDS\), got 0"):
        eng.adv_sums_add([])
    with pytest.raises(ValueError, match=r"blocks must be a list of 1..16 tensors \(PF_PPO_MAX_SHARDS\), got 17"):
        eng.adv_sums_add([torch.zeros(4, dtype=f64)] * 17)
    with pytest.raises(ValueError, match=r"blocks\[1\] must be a contiguous float64 tensor of shape \(4,\)"):
        eng.adv_sums_add([torch.zeros(4, dtype=f64), torch.zeros(4)])
    with pytest.raises(ValueError, match="dst must hold 1 \\+ 2 D doubles with D in 1..128, got 4"):
        eng.moments_merge(torch.zeros(4, dtype=f64), [torch.zeros(4, dtype=f64)])
    with pytest.raises(ValueError, match="dst must hold 1 \\+ 2 D doubles with D in 1..128, got 259"):
        eng.moments_merge(torch.zeros(259, dtype=f64), [torch.zeros(259, dtype=f64)])
    with pytest.raises(ValueError, match=r"blocks\[0\] must be a contiguous float64 tensor of shape \(43,\)"):
        eng.moments_merge(torch.zeros(43, dtype=f64), [torch.zeros(3, dtype=f64)])
    block, flat, sums = torch.zeros(24, dtype=f64), torch.zeros(10), torch.zeros(4, dtype=f64)
    with pytest.raises(ValueError, match=r"blocks\[0\] must be a contiguous float64 tensor of shape \(24,\)"):
        eng.ppo_shard_combine([sums], sums, [flat], torch.zeros(4))
    with pytest.raises(ValueError, match=r"flats must hold one flat gradient per block \(1\), got 2"):
        eng.ppo_shard_combine([block], sums, [flat, flat], torch.zeros(4))
    with pytest.raises(ValueError, match=r"flats\[1\] must be a contiguous float32 tensor of shape \(10,\)"):
        eng.ppo_shard_combine([block, block], sums, [flat, torch.zeros(11)], torch.zeros(4))
    with pytest.raises(ValueError, match="ent_coef must be finite and >= 0"):
        eng.ppo_shard_combine([block], sums, [flat], torch.zeros(4), ent_coef=-1.0)
    with pytest.raises(ValueError, match="value_clip must be a bool"):
        eng.ppo_shard_combine([block], sums, [flat], torch.zeros(4), value_clip=1)
    with pytest.raises(ValueError, match="log_std's length \\(the action width\\) must be in 1..8, got 9"):
        eng.ppo_shard_combine([block], sums, [flat], torch.zeros(9))
    assert eng.grad_numel([(8, 21), (4, 8)], [(8, 21), (1, 8)]) == 8 * 21 + 8 + 4 * 8 + 4 + 8 * 21 + 8 + 8 + 1
