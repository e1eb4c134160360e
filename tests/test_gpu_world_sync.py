"""pf_world_sync on the device against a numpy restatement of its seven rules (include/pyflyt_amd.h), written from the contract:
random latch / flag / reward / exclude rows with NaN rewards on latched lanes, worlds of 1, 4, 6 and 64 lanes -- with 6, worlds
straddle the kernel's 256-thread workgroups --, and the C refusals with their messages."""
import ctypes as C

import numpy as np
import pytest
import torch

from pyflyt_amd import PyFlytAmdError, build_params
from pyflyt_amd import _lib as L
from pyflyt_amd.engine import BatchEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 257), (4, 1028), (6, 1026), (64, 320)]


def ref_world_sync(A, terminated, truncated, reward, done, exclude):
    """The rules, lane by lane, from the latch as it was when the call began."""
    n = done.shape[0]
    was = done != 0
    waiting = np.repeat(was.reshape(n // A, A).all(axis=1), A)
    valid = ~was & ~(exclude != 0 if exclude is not None else np.zeros(n, dtype=bool))
    new_reward = np.where(was, np.float32(0.0), reward)
    new_term, new_trunc = np.where(was, 0, terminated).astype(np.uint8), np.where(was, 0, truncated).astype(np.uint8)
    ended = ~was & ((terminated | truncated) != 0)
    new_done = np.where(waiting, 0, (was | ended)).astype(np.uint8)
    return dict(reward=new_reward, terminated=new_term, truncated=new_trunc, done=new_done, valid=valid.astype(np.uint8), reset=waiting.astype(np.uint8))


def make_case(A, n, seed, with_exclude):
    rng = np.random.default_rng(seed)
    W = n // A
    done = (rng.random(n) < 0.4).astype(np.uint8)
    d = done.reshape(W, A)
    # several worlds that wait for their reset, the first and the last among them (the edges of the grid) ...
    all_done = np.concatenate(([0, W - 1], 1 + rng.choice(W - 2, size=min(5, max(0, W // 3 - 2)), replace=False)))
    d[all_done] = 1
    if A > 1:  # ... and several with all but one agent done, the one left at either end and in the middle
        rest = np.setdiff1d(np.arange(W), all_done)
        for j, w in enumerate(rng.choice(rest, size=min(7, max(2, len(rest) // 2)), replace=False)):
            d[w] = 1
            d[w, (0, A - 1, A // 2)[j % 3]] = 0
    done = d.reshape(n)
    terminated = (rng.random(n) < 0.3).astype(np.uint8)
    truncated = (rng.random(n) < 0.3).astype(np.uint8)
    reward = rng.normal(size=n).astype(np.float32)
    latched = np.flatnonzero(done)
    reward[latched[::2]] = np.nan  # a dead lane's NaN must reach nothing
    reward[np.flatnonzero(done == 0)[:1]] = -0.0  # (a live lane's reward stays as it is, to the sign of a zero)
    exclude = (rng.random(n) < 0.5).astype(np.uint8) if with_exclude else None
    # "non-zero" is the rule, not bit 0: the set bytes are 1, 2, 0x80 and 0xFF in turn
    for x in (done, terminated, truncated, exclude):
        if x is not None:
            x *= np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)[np.arange(n) % 4]
    return dict(terminated=terminated, truncated=truncated, reward=reward, done=done, exclude=exclude)


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(n):
        if n not in made:
            made[n] = BatchEngine(build_params("quadx", "hover", autoreset="off", seed=1), n, device=DEV)
        return made[n]

    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("A, n", SHAPES)
@pytest.mark.parametrize("with_exclude", [False, True])
def test_against_the_rules(engines, A, n, with_exclude):
    eng = engines(n)
    c = make_case(A, n, seed=100 * A + int(with_exclude), with_exclude=with_exclude)
    d = (c["done"] != 0).reshape(n // A, A)
    assert int(d.all(axis=1).sum()) >= 2 and (A == 1 or int((d.sum(axis=1) == A - 1).sum()) >= 2)  # (the seeded worlds are there)
    assert np.isnan(c["reward"][c["done"] != 0]).any() and not np.isnan(c["reward"][c["done"] == 0]).any()
    for flag_dtype in (torch.uint8, torch.bool):  # (uint8: the bytes as they are; bool: torch's 0 / 1)
        if flag_dtype == torch.bool:
            c = {k: ((v != 0).astype(np.uint8) if v is not None and k != "reward" else v) for k, v in c.items()}
        want = ref_world_sync(A, **c)
        assert set(np.unique(np.concatenate([want[x] for x in ("done", "valid", "reset")]))) == {0, 1}  # (these three are written 0 / 1)
        t = {k: (None if v is None else torch.as_tensor(v, device=DEV).contiguous()) for k, v in c.items()}
        for k in ("terminated", "truncated", "done"):
            t[k] = t[k].to(flag_dtype) if flag_dtype == torch.bool else t[k]
        valid = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        reset = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        out = eng.world_sync(t["terminated"], t["truncated"], t["reward"], t["done"], A, exclude=t["exclude"], valid_out=valid, reset_out=reset)
        assert out[0] is valid and out[1] is reset
        torch.cuda.synchronize()
        got = dict(reward=t["reward"], terminated=t["terminated"], truncated=t["truncated"], done=t["done"], valid=valid, reset=reset)
        for name, w in want.items():
            g = got[name].view(torch.uint8).cpu().numpy() if name != "reward" else got[name].cpu().numpy()
            if name == "reward":  # exact, bits included: +0.0 where latched, the input's bits elsewhere
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name
            else:
                assert np.array_equal(g, w), (name, flag_dtype)


def test_a_world_goes_round(engines):
    """Three calls on one latch: the agents of a world end one after the other, the world waits, is named for its reset, and is open again."""
    A, n = 4, 1028
    eng = engines(n)
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    z = lambda: torch.zeros(n, dtype=torch.bool, device=DEV)
    term, trunc, rew = z(), z(), torch.ones(n, device=DEV)
    term[4:7] = True  # world 1: agents 0-2 end
    valid, reset = eng.world_sync(term, trunc, rew, done, A)
    assert bool(valid.all()) and not bool(reset.any()) and done.tolist()[4:8] == [1, 1, 1, 0]
    term, trunc, rew = z(), z(), torch.ones(n, device=DEV)
    trunc[7] = True   # the last one ends
    valid, reset = eng.world_sync(term, trunc, rew, done, A)
    assert valid.tolist()[4:8] == [False, False, False, True] and not bool(reset.any()) and done.tolist()[4:8] == [1, 1, 1, 1]
    assert rew.tolist()[4:8] == [0.0, 0.0, 0.0, 1.0] and bool(trunc[7])
    term, trunc, rew = z(), z(), torch.ones(n, device=DEV)
    term[5] = True    # (a flag of the wasted step: blanked, and it latches nothing)
    valid, reset = eng.world_sync(term, trunc, rew, done, A)
    assert not bool(valid[4:8].any()) and bool(valid[:4].all()) and bool(valid[8:].all())
    assert reset.tolist()[4:8] == [True] * 4 and int(reset.sum()) == 4 and int(done.sum()) == 0 and not bool(term[5])


def test_engine_latch_and_env_reset():
    eng = BatchEngine(build_params("quadx", "hover", autoreset="off", seed=1), 1028, device=DEV)
    eng.env_reset()
    eng.env_reset(mask=torch.ones(1028, dtype=torch.bool, device=DEV))
    assert eng._world_done is None  # (made at first use only: env_reset touches the latch only once it exists)
    assert eng.world_done.dtype == torch.uint8 and tuple(eng.world_done.shape) == (1028,)
    eng.world_done.fill_(1)
    mask = torch.zeros(1028, dtype=torch.bool, device=DEV)
    mask[8:12] = True
    eng.env_reset(mask=mask)
    assert int(eng.world_done.sum()) == 1024 and not bool(eng.world_done[8:12].any())
    eng.env_reset()
    assert int(eng.world_done.sum()) == 0
    eng.close()


def test_c_refusals(engines):
    eng = engines(1028)
    lib, ctx = eng.lib, eng._ctx
    flags = [torch.zeros(1028, dtype=torch.uint8, device=DEV) for _ in range(5)]
    reward = torch.zeros(1028, device=DEV)
    fields = dict(terminated=flags[0], truncated=flags[1], reward=reward, done=flags[2], valid_out=flags[3], reset_out=flags[4])

    def block(skip=None):
        a = L.PfWorldSync()
        for name, t in fields.items():
            setattr(a, name, None if name == skip else t.data_ptr())
        return a

    def refused(a, A, text, c=ctx):
        rc = lib.pf_world_sync(c, None if a is None else C.byref(a), A, None)
        assert rc == L.ERR_ARG
        msg = lib.pf_last_error(c).decode()
        assert msg == f"pf_world_sync: {text}", msg

    refused(None, 4, "the argument block is required")
    refused(block(), 4, "ctx is required", c=None)
    for name in fields:
        refused(block(skip=name), 4, f"{name} is required")
    for A in (0, -4, 65):
        refused(block(), A, "agents_per_world must be in 1..64")
    for A in (3, 8, 64):  # 1028 = 4 x 257
        refused(block(), A, "agents_per_world must divide the context's lane count n")
    with pytest.raises(PyFlytAmdError, match="pf_world_sync: done is required"):
        L.check(lib.pf_world_sync(ctx, C.byref(block(skip="done")), 4, None), ctx)
    assert lib.pf_world_sync(ctx, C.byref(block()), 4, None) == 0  # (and the good block runs: exclude may be NULL)
    torch.cuda.synchronize()
