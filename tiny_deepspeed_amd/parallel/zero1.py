"""ZeRO-1 strategy: optimizer-state sharding.

Capability parity with ``/root/reference/tiny_deepspeed/core/zero/zero1/``:
gradients are average-REDUCED to the owning rank during backward (half the
traffic of all-reduce), optimizer state (m/v/momentum/master) exists only
on the owner, the owner updates its partition and broadcasts refreshed
parameters to all ranks at step end.
"""

from .. import optim as base_optim
from ._grad import strategy_swap_map, REDUCE_KEEP
from ._zero_optim import _ZeroOptimMixin
from .wrapper import ModelWrapper


class Zero1(ModelWrapper):
    swap_map = strategy_swap_map(REDUCE_KEEP)

    def __init__(self, module, parts, comm=None):
        super().__init__(module, parts=parts, comm=comm)


class Zero1SGD(_ZeroOptimMixin, base_optim.SGD):
    pass


class Zero1AdamW(_ZeroOptimMixin, base_optim.AdamW):
    pass
