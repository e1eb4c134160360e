"""A BatchEngine without a context, for the CPU tests of the argument checks (tests/test_cpu_{gae,traj_stats,ppo_loss,mlp,adam}.py):
what the engine's methods check before they reach the library needs the lane count, the observation width, the device and the
parameters only. Never __init__: that needs a GPU."""
import torch

from pyflyt_amd import build_params
from pyflyt_amd.engine import BatchEngine

N = 8


def bare_engine(autoreset="next_step", obs_dim=21):
    eng = object.__new__(BatchEngine)
    eng.n, eng.obs_dim, eng.device, eng.params, eng._ctx = N, obs_dim, torch.device("cpu"), build_params("quadx", "hover", autoreset=autoreset), None
    return eng
