"""Gradient clipping by global norm (max_grad_norm=) on the CPU: the torch
oracle in one process, parity of every strategy over gloo at world 2, the
rank that owns nothing still entering the collective, and argument checks.

AdamW is nearly blind to a constant gradient scale (clipped and unclipped
losses of the tiny model differ by 1e-4..6e-4), so the loss-parity tests use
SGD, whose update is proportional to the clip coefficient."""

import pytest
import torch

from tests import _clip_workers as C
from tests.dist_utils import run_distributed
from tiny_deepspeed_amd import AdamW, SGD, Zero1SGD, ops

STRATEGIES = ["ddp", "zero1", "zero2", "zero3", "zero2flat"]

# single-device reference of the issue: Single + clip_grad_norm_(1.0) + SGD
TABLE_NORM = [1.1664, 1.1131, 0.9954, 0.9215]
TABLE_CLIPPED = [4.56737, 4.45392, 4.26994, 4.07085]
TABLE_UNCLIPPED = [4.56737, 4.43620, 4.23672, 4.03655]


# ---- 1. torch oracle -------------------------------------------------------
_OURS = {
    "sgd": lambda named, m: SGD(named, lr=1e-2, momentum=0.9,
                                max_grad_norm=m),
    "adamw": lambda named, m: AdamW(named, lr=1e-2, weight_decay=0.1,
                                    max_grad_norm=m),
}
_TORCH = {
    "sgd": lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9),
    "adamw": lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.1),
}


def _assert_clipped_and_not(norms, m):
    assert any(n > m for n in norms) and any(n < m for n in norms), (norms, m)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clip_matches_torch_oracle(kind):
    """The set-up of tests/test_optim.py::_run; m = 0.7 lies inside the run's
    norms (0.36 .. 1.03 unclipped), so some steps clip and some do not."""
    m = 0.7
    torch.manual_seed(0)
    ours_mod = torch.nn.Linear(8, 8)
    torch.manual_seed(0)
    ref_mod = torch.nn.Linear(8, 8)
    ours = _OURS[kind](ours_mod.named_parameters(), m)
    ref = _TORCH[kind](ref_mod.parameters())
    assert ours.last_grad_norm is None
    torch.manual_seed(42)
    norms = []
    for _ in range(5):
        x = torch.randn(4, 8)
        ours_mod(x).square().mean().backward()
        ref_mod(x).square().mean().backward()
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_mod.parameters(), m)
        ours.step()
        ref.step()
        ref.zero_grad()
        got = ours.last_grad_norm
        assert got.dim() == 0 and got.dtype == torch.float32
        torch.testing.assert_close(got, ref_norm, rtol=1e-6, atol=0.0)
        norms.append(float(got))
    _assert_clipped_and_not(norms, m)
    for p1, p2 in zip(ours_mod.parameters(), ref_mod.parameters()):
        assert torch.allclose(p1, p2, atol=1e-6), (p1 - p2).abs().max()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clip_bf16_master_matches_torch_oracle(kind):
    """bf16 parameters: the norm and the scaled update are fp32 over the bf16
    gradients, so the oracle is clip_grad_norm_ + torch.optim on fp32 shadow
    parameters whose .grad is grad.float(); masters must match it."""
    m = 0.5
    torch.manual_seed(0)
    mod = torch.nn.Linear(16, 16).to(torch.bfloat16)
    shadow = [torch.nn.Parameter(p.detach().float().clone())
              for p in mod.parameters()]
    ours = _OURS[kind](mod.named_parameters(), m)
    ref = _TORCH[kind](shadow)
    torch.manual_seed(42)
    norms = []
    for i in range(5):
        # a growing input scale spreads the norms to both sides of m
        x = (torch.randn(4, 16) * (0.5 + 0.5 * i)).to(torch.bfloat16)
        mod(x).float().square().mean().backward()
        for s, p in zip(shadow, mod.parameters()):
            s.grad = p.grad.float()
        ref_norm = torch.nn.utils.clip_grad_norm_(shadow, m)
        ours.step()
        ref.step()
        torch.testing.assert_close(ours.last_grad_norm, ref_norm, rtol=1e-6,
                                   atol=0.0)
        norms.append(float(ref_norm))
        for (n, p), s in zip(mod.named_parameters(), shadow):
            assert torch.allclose(ours.master[n], s, atol=1e-6), \
                (i, n, (ours.master[n] - s).abs().max())
            assert torch.equal(p.data, ours.master[n].to(torch.bfloat16))
    _assert_clipped_and_not(norms, m)


# ---- 2. strategy parity over gloo ------------------------------------------
@pytest.fixture(scope="module")
def single_ref():
    return {mode: C.single_device_run(mode) for mode in ("torch", None)}


def test_single_device_reference(single_ref):
    """The reference itself: the issue's table, steps 1-2 clip and 3-4 do
    not, ours equals torch's, and clipping moves the loss by more than 0.01
    from step 2 on (50x the parity tolerance: a wrong norm cannot pass)."""
    losses, norms = single_ref["torch"]
    plain, _ = single_ref[None]
    assert norms == pytest.approx(TABLE_NORM, abs=1e-4)
    assert losses == pytest.approx(TABLE_CLIPPED, abs=2e-4)
    assert plain == pytest.approx(TABLE_UNCLIPPED, abs=2e-4)
    assert [n > C.MAX_NORM for n in norms] == [True, True, False, False]
    for a, b in zip(losses[1:], plain[1:]):
        assert abs(a - b) > 0.01, (losses, plain)
    ours_losses, ours_norms = C.single_device_run("ours")
    assert ours_losses == pytest.approx(losses, abs=2e-4)
    assert ours_norms == pytest.approx(norms, rel=1e-5)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_clip_parity_vs_single_device(strategy, single_ref):
    exp_losses, exp_norms = single_ref["torch"]
    results = run_distributed(C.train_strategy_clip, world=2,
                              args=(strategy,))
    assert sorted(results) == [0, 1]
    for rank, (losses, norms) in results.items():
        assert losses == pytest.approx(exp_losses, abs=2e-4), (
            f"{strategy} rank {rank}: {losses} != {exp_losses}")
        assert norms == pytest.approx(exp_norms, rel=1e-5), (
            f"{strategy} rank {rank}: {norms} != {exp_norms}")


# ---- 3. a rank that owns nothing still takes part --------------------------
class _StubComm:
    """Rank 0 of 2, every collective recorded and none performed."""

    rank = 0
    world_size = 2

    def __init__(self):
        self.calls = []

    def _inactive(self):
        return False

    def sync(self):
        self.calls.append(("sync",))

    def broadcast_bucketed(self, tensors_with_src, **kw):
        self.calls.append(("broadcast_bucketed", len(tensors_with_src)))

    def all_reduce_sum(self, t):
        self.calls.append(("all_reduce_sum", t.clone()))
        return t


def test_rank_without_parameters_enters_the_norm_all_reduce():
    torch.manual_seed(0)
    lin = torch.nn.Linear(8, 8)
    parts = {n: 1 for n, _ in lin.named_parameters()}  # all on the other rank
    comm = _StubComm()
    opt = Zero1SGD(lin.named_parameters(), param_part_table=parts,
                   ranks_map=["cpu", "cpu"], comm=comm, lr=0.1, momentum=0.9,
                   max_grad_norm=1.0)
    before = [p.detach().clone() for p in lin.parameters()]
    lin(torch.randn(4, 8)).square().mean().backward()
    opt.step()
    reduces = [c for c in comm.calls if c[0] == "all_reduce_sum"]
    assert len(reduces) == 1, comm.calls
    sent = reduces[0][1]
    assert sent.dim() == 0 and sent.dtype == torch.float32
    assert sent.item() == 0.0
    # after pre_step's sync, before the parameter broadcast
    names = [c[0] for c in comm.calls]
    assert names.index("sync") < names.index("all_reduce_sum") \
        < names.index("broadcast_bucketed")
    assert float(opt.last_grad_norm) == 0.0
    for p, b in zip(lin.parameters(), before):
        assert torch.equal(p, b)


# ---- 4. argument checks ----------------------------------------------------
@pytest.mark.parametrize("cls", [SGD, AdamW])
@pytest.mark.parametrize("bad", [0, -1, 0.0, -1.0])
def test_max_grad_norm_must_be_positive(cls, bad):
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="max_grad_norm"):
        cls(lin.named_parameters(), lr=1e-2, max_grad_norm=bad)


@pytest.mark.parametrize("cls", [SGD, AdamW])
def test_no_clipping_leaves_last_grad_norm_none(cls):
    lin = torch.nn.Linear(4, 4)
    opt = cls(lin.named_parameters(), lr=1e-2, max_grad_norm=None)
    lin(torch.randn(2, 4)).sum().backward()
    opt.step()
    assert opt.last_grad_norm is None


@pytest.mark.parametrize("cls,kw", [(SGD, dict(momentum=0.9)), (AdamW, {})])
def test_state_dict_format_unchanged_by_clipping(cls, kw):
    def sd_of(**extra):
        torch.manual_seed(0)
        lin = torch.nn.Linear(4, 4)
        opt = cls(lin.named_parameters(), lr=1e-2, **kw, **extra)
        lin(torch.randn(2, 4)).sum().backward()
        opt.step()
        return opt.state_dict()

    plain, clipped = sd_of(), sd_of(max_grad_norm=1.0)
    assert set(plain) == set(clipped) == {"t", "lr", "state"}
    assert set(plain["state"]) == set(clipped["state"])
    for key in plain["state"]:
        assert set(plain["state"][key]) == set(clipped["state"][key])


def test_grad_sumsq_cpu():
    z = ops.grad_sumsq([])
    assert z.dim() == 0 and z.dtype == torch.float32 and z.item() == 0.0
    assert ops.grad_sumsq([torch.empty(0), torch.empty(0, 3)]).item() == 0.0
    ts = [torch.full((3,), 2.0), torch.empty(0),
          torch.ones(5, dtype=torch.bfloat16)]
    s = ops.grad_sumsq(ts)
    assert s.dtype == torch.float32 and s.item() == 17.0


def test_clip_coef_uses_torch_constants():
    norm, coef = ops.clip_coef(torch.tensor(4.0), 1.0)
    assert norm.item() == 2.0
    assert coef.item() == pytest.approx(1.0 / (2.0 + 1e-6), rel=1e-7)
    _, coef = ops.clip_coef(torch.tensor(0.25), 1.0)
    assert coef.item() == 1.0
    _, coef = ops.clip_coef(torch.tensor(0.0), 1.0)
    assert coef.item() == 1.0
