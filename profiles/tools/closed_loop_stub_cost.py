"""The Python of the stepwise closed loop alone, on a CPU: BatchEngine.rollout_policy_steps and rollout_policy_worlds on an engine made
without a context, over host tensors, against a stub library whose four entry points return 0 (compiled here with `cc`). What is left
is what the loop costs the host per env step: the row arithmetic, the block updates and the foreign calls. torch.cuda.device and the
stream handle, which need a GPU, are replaced by no-ops: the same on every tree this runs on. Where a device-bound leg of
profiles/closed_loop/nothing_moved.txt lands outside, this is where a cause in the Python would show.

Nanoseconds per env step: the least of `--samples` samples of `--calls` calls each (the least: on a shared CPU everything above it is
someone else). Prints one JSON line. No GPU, no libpyflyt_amd.so."""
import argparse
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyflyt_amd import MLPPolicy, build_params  # noqa: E402
from pyflyt_amd import _lib as L  # noqa: E402
from pyflyt_amd.engine import BatchEngine  # noqa: E402

STUB = """
int pf_policy_act(void* c, void* q, void* a, unsigned s, void* st) { return 0; }
int pf_env_step(void* c, void* b, void* st) { return 0; }
int pf_world_sync(void* c, void* w, int a, void* st) { return 0; }
int pf_env_reset(void* c, void* b, void* m, void* st) { return 0; }
"""


def stub_lib(tmp):
    src, so = os.path.join(tmp, "stub.c"), os.path.join(tmp, "libstub.so")
    open(src, "w").write(STUB)
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", src, "-o", so])
    lib = C.CDLL(so)
    lib.pf_policy_act.argtypes = [C.c_void_p, C.POINTER(L.PfPolicy), C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pf_env_step.argtypes = [C.c_void_p, C.POINTER(L.PfBuffers), C.c_void_p]
    lib.pf_world_sync.argtypes = [C.c_void_p, C.POINTER(L.PfWorldSync), C.c_int, C.c_void_p]
    lib.pf_env_reset.argtypes = [C.c_void_p, C.POINTER(L.PfBuffers), C.c_void_p, C.c_void_p]
    return lib


def engine(lib, params, n, obs_dim, same_step):
    """What BatchEngine.__init__ makes, without the context and on the host."""
    eng = object.__new__(BatchEngine)
    eng.lib, eng.params, eng.n, eng.obs_dim, eng.device, eng._ctx, eng._index = lib, params, n, obs_dim, torch.device("cpu"), C.c_void_p(1), 0
    eng.state, eng.obs, eng.reward = torch.zeros(16, n, 4), torch.zeros(n, obs_dim), torch.zeros(n)
    eng.terminated, eng.truncated = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    eng.final_obs = torch.zeros(n, obs_dim) if same_step else None
    eng.final_info = torch.zeros(n, 2, dtype=torch.int32) if same_step else None
    for name in ("out_state", "link_pos", "ctrl_ratio", "modes", "start_vel", "armed", "out_aux", "out_contact", "out_contact_peers"):
        setattr(eng, name, None)
    eng._buf, eng._prepared, eng._cur_obs = L.PfBuffers(), {}, eng.obs
    eng._stream = lambda: C.c_void_p(0)
    return eng


def policy(eng):
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(eng.obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, eng.action_dim))
    return MLPPolicy.from_torch(net, log_std=torch.full((eng.action_dim,), -1.0))


def least_ns(call, k, samples, calls):
    call()
    best = float("inf")
    for _ in range(samples):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        best = min(best, (time.perf_counter() - t0) * 1e9 / (calls * k))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=100)
    args = ap.parse_args()
    torch.cuda.device = contextlib.nullcontext  # (takes the device as its enter_result and selects nothing)
    res = {"unit": "host ns per env step, least sample", "stub": "four entry points that return 0"}
    with tempfile.TemporaryDirectory(prefix="pf_stub_") as tmp:
        lib = stub_lib(tmp)
        k = 100
        for mode in ("next_step", "same_step"):
            eng = engine(lib, build_params("fixedwing", "waypoints", seed=1, autoreset=mode), 1024, 30, mode == "same_step")
            pol = policy(eng)
            res[f"steps.{mode}"] = least_ns(lambda: eng.rollout_policy_steps(pol, k), k, args.samples, args.calls)
        k = 64
        P = build_params("fixedwing", "dogfight", seed=1, autoreset="off", angle_representation="euler", vehicle_options=dict(drone_model="acrowing"),
                         dogfight=dict(team_size=2))
        eng = engine(lib, P, 1024, 60, False)
        pol = policy(eng)
        res["worlds"] = least_ns(lambda: eng.rollout_policy_worlds(pol, k, 4), k, args.samples, args.calls)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
