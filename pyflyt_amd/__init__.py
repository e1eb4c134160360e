"""pyflyt_amd -- MI355X-native batched UAV-physics step behind PyFlyt-shaped APIs.

Only the hot path of jjshoots/PyFlyt is implemented: Aviary.step() + the
per-drone control/physics/state loop + the 6-DoF integrator, as hand-written HIP kernels for
gfx950 called through a C ABI (include/pyflyt_amd.h). There is no CPU fallback.
"""
from . import _lib
from ._lib import PyFlytAmdError
from .params import build_params
from .moments import RunningMoments
from .policy import MLPPolicy
from .ppo import minibatches, ppo_grad, ppo_loss, ppo_stats_dict
from .nets import mlp
from .optim import Adam
from .sharded import Replicas, ppo_grad_sharded

__all__ = ["_lib", "PyFlytAmdError", "build_params", "MLPPolicy", "RunningMoments", "ppo_loss", "ppo_grad", "ppo_stats_dict", "minibatches", "mlp", "Adam", "Replicas", "ppo_grad_sharded"]
__version__ = "0.1.0"
