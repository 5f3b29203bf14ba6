"""DDP strategy: replicated parameters, per-parameter async grad all-reduce
overlapped with backward's dX compute.

Capability parity with ``/root/reference/tiny_deepspeed/core/zero/ddp/``
(wrapper.py:15-40, module.py:27-147, optim.py:18-33). The collective is
enqueued on the comm stream right after dW is produced and the dX GEMM runs
concurrently — true overlap, without the reference's
torch.cuda.synchronize() flaw.
"""

from .. import optim as base_optim
from ._grad import strategy_swap_map, ALLREDUCE
from .comm import default_comm
from .wrapper import ModelWrapper


class DDP(ModelWrapper):
    swap_map = strategy_swap_map(ALLREDUCE)


class _DDPOptimMixin:
    """Local step; the only distributed action is waiting for in-flight
    grad all-reduces (device-side) before the first update. Clipping
    (max_grad_norm) needs no collective either: after that wait every rank
    holds the same averaged gradients, so the base _reduce_sumsq (identity)
    gives every rank the same global norm."""

    def __init__(self, parameters, comm=None, **kw):
        super().__init__(parameters, **kw)
        self.comm = comm if comm is not None else default_comm()

    def pre_step(self):
        self.comm.sync()


class DDPSGD(_DDPOptimMixin, base_optim.SGD):
    pass


class DDPAdamW(_DDPOptimMixin, base_optim.AdamW):
    pass
