"""ZeRO-2 strategy: optimizer-state + gradient sharding.

Capability parity with ``/root/reference/tiny_deepspeed/core/zero/zero2/``.
After the average-reduce to the owner, NON-owner ranks actually release the
gradient memory: the last reference to dW is dropped once the collective
is enqueued and the stream-ordered caching allocator reclaims the block
when RCCL is done (the reference could only shrink grad.data to 1 element
and wished for a C++ plugin — zero2/module.py:26-36).
"""

from .. import optim as base_optim
from ._grad import strategy_swap_map, REDUCE_SHARD
from ._zero_optim import _ZeroOptimMixin
from .wrapper import ModelWrapper


class Zero2(ModelWrapper):
    swap_map = strategy_swap_map(REDUCE_SHARD)

    def __init__(self, module, parts, comm=None):
        super().__init__(module, parts=parts, comm=comm)


class Zero2SGD(_ZeroOptimMixin, base_optim.SGD):
    pass


class Zero2AdamW(_ZeroOptimMixin, base_optim.AdamW):
    pass
