"""Order of ops and collectives inside the strategy modules' callbacks.

What the comm/compute overlap depends on and no loss-parity test can see:
dW is published before db is computed and both before dX (the dX GEMM runs
under the in-flight collectives), ZeRO-3 issues the neighbour's gathers
before this module's compute, and the fused lm_head path publishes its dW
exactly once. Proven on gloo world 1 with TDSA_COMM_FORCE=1, where every
collective really runs, by recording the op and collective calls.
"""

from collections import OrderedDict

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tiny_deepspeed_amd as tdsa
from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.parallel.comm import CommContext
from tests.test_comm_force import world1_pg  # noqa: F401  (fixture)

OPS = ("linear_forward", "linear_weight_grad", "linear_bias_grad",
       "linear_input_grad")
COLLECTIVES = ("all_reduce_avg", "reduce_avg_to", "gather_broadcast")
WRAPPERS = {"ddp": tdsa.DDP, "zero1": tdsa.Zero1, "zero2": tdsa.Zero2,
            "zero3": tdsa.Zero3}
GRAD_COLLECTIVE = {"ddp": "all_reduce_avg", "zero1": "reduce_avg_to",
                   "zero2": "reduce_avg_to", "zero3": "reduce_avg_to"}


def _wrap(strategy, model):
    comm = CommContext()
    assert comm.force and not comm._inactive()
    if strategy == "ddp":
        return tdsa.DDP(model, comm=comm)
    parts, _ = tdsa.partition_tensors(
        OrderedDict(model.named_parameters()), ["cpu"])
    return WRAPPERS[strategy](model, parts, comm=comm)


def _record(monkeypatch, comm):
    """Log (name, args, result) of every Linear op and of the collectives
    the strategies issue from their callbacks."""
    log = []

    def recording(name, fn):
        def wrapper(*args, **kwargs):
            out = fn(*args, **kwargs)
            log.append((name, args, out))
            return out
        return wrapper

    for name in OPS:
        monkeypatch.setattr(ops, name, recording(name, getattr(ops, name)))
    for name in COLLECTIVES:
        monkeypatch.setattr(comm, name, recording(name, getattr(comm, name)))
    return log


def _three_linears(strategy, monkeypatch):
    """One forward/backward of three biased Linear(8, 8); returns the
    modules and the forward and backward halves of the call log."""
    torch.manual_seed(0)
    wrapped = _wrap(strategy, nn.Sequential(*[nn.Linear(8, 8)
                                              for _ in range(3)]))
    log = _record(monkeypatch, wrapped.comm)
    y = wrapped(torch.randn(4, 8))
    n_fwd = len(log)
    y.square().mean().backward()
    wrapped.comm.sync()
    return list(wrapped.module), log[:n_fwd], log[n_fwd:]


def _ptr(t):
    return t.data_ptr()


@pytest.mark.parametrize("strategy", ["ddp", "zero1", "zero2", "zero3"])
def test_backward_publishes_dw_then_db_then_computes_dx(
        world1_pg, monkeypatch, strategy):  # noqa: F811
    mods, _, bwd = _three_linears(strategy, monkeypatch)
    steps = [e for e in bwd if e[0] != "gather_broadcast"]
    coll = GRAD_COLLECTIVE[strategy]
    assert [e[0] for e in steps] == [
        "linear_weight_grad", coll, "linear_bias_grad", coll,
        "linear_input_grad"] * 3
    for k, mod in enumerate(reversed(mods)):
        wgrad, wcoll, bgrad, bcoll, igrad = steps[5 * k:5 * k + 5]
        # each collective carries the gradient just computed, full shape
        assert wcoll[1][0] is wgrad[2] and wgrad[2].shape == (8, 8)
        assert bcoll[1][0] is bgrad[2] and bgrad[2].shape == (8,)
        # and the dX that follows is this module's
        assert _ptr(igrad[1][1]) == _ptr(mod.weight)


def test_zero3_prefetches_neighbour_before_compute(
        world1_pg, monkeypatch):  # noqa: F811
    mods, fwd, bwd = _three_linears("zero3", monkeypatch)

    def gathers_of(log, mod):
        want = {_ptr(mod.weight), _ptr(mod.bias)}
        idx = [i for i, e in enumerate(log)
               if e[0] == "gather_broadcast" and _ptr(e[1][0]) in want]
        assert len(idx) == 2, (len(idx), [e[0] for e in log])
        return idx

    def nth(log, name, n):
        return [i for i, e in enumerate(log) if e[0] == name][n]

    for i in (0, 1):
        assert max(gathers_of(fwd, mods[i + 1])) < nth(fwd, "linear_forward", i)
    # backward visits the modules in reverse: the k-th dW is module 2-k's
    for i in (2, 1):
        assert (max(gathers_of(bwd, mods[i - 1]))
                < nth(bwd, "linear_weight_grad", 2 - i))


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(8, 16, bias=False)

    def forward(self, x, targets):
        return self.proj.project_cross_entropy(x, targets)


@pytest.mark.parametrize("strategy", ["ddp", "zero3"])
def test_fused_lmhead_publishes_dw_once(world1_pg, monkeypatch,  # noqa: F811
                                        strategy):
    torch.manual_seed(0)
    wrapped = _wrap(strategy, _Head())
    weight = wrapped.module.proj.weight
    w_ref = weight.detach().clone().requires_grad_(True)
    x = torch.randn(8, 8)
    tg = torch.randint(0, 16, (8,))
    log = _record(monkeypatch, wrapped.comm)
    wrapped(x, tg).backward()
    wrapped.comm.sync()
    published = [e for e in log if e[0] == GRAD_COLLECTIVE[strategy]]
    assert len(published) == 1
    assert published[0][1][0].shape == (16, 8)
    F.cross_entropy(F.linear(x, w_ref), tg).backward()
    torch.testing.assert_close(weight.grad, w_ref.grad, rtol=0, atol=1e-6)
