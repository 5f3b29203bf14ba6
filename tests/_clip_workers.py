"""Gradient-clipping runs for tests/test_grad_clip.py: the single-device
references and the worker executed inside spawned gloo ranks (dist_utils).
Model, batch and seed are those of tests/_dist_workers.py."""

from collections import OrderedDict

import torch

from tests._dist_workers import CFG, ITERS, batch, make_cfg  # noqa: F401

MAX_NORM = 1.0
SGD_KW = dict(lr=0.1, momentum=0.9)


def single_device_run(clip):
    """(losses, norms) of Single + SGD. clip: "torch" clips with
    torch.nn.utils.clip_grad_norm_ in front of an unclipped SGD (the oracle),
    "ours" uses SGD(max_grad_norm=), None does not clip (norms are torch's)."""
    import tiny_deepspeed_amd as tdsa
    from tiny_deepspeed_amd.models import GPT2Model

    torch.manual_seed(0)
    model = tdsa.Single(GPT2Model(make_cfg()))
    kw = dict(SGD_KW, max_grad_norm=MAX_NORM) if clip == "ours" else SGD_KW
    opt = tdsa.SGD(model.named_parameters(), **kw)
    x, y = batch()
    losses, norms = [], []
    for _ in range(ITERS):
        _, loss = model(x, y)
        loss.backward()
        if clip != "ours":
            norm = torch.nn.utils.clip_grad_norm_(
                list(model.parameters()),
                MAX_NORM if clip == "torch" else float("inf"))
        opt.step()
        if clip == "ours":
            norm = opt.last_grad_norm
        losses.append(loss.item())
        norms.append(float(norm))
    return losses, norms


def train_strategy_clip(rank, world, strategy):
    """(losses, last_grad_norm per step) of one rank under `strategy` with
    SGD(max_grad_norm=MAX_NORM)."""
    import tiny_deepspeed_amd as tdsa
    from tiny_deepspeed_amd.models import GPT2Model

    torch.manual_seed(0)
    model = GPT2Model(make_cfg())
    ranks_map = ["cpu"] * world
    kw = dict(SGD_KW, max_grad_norm=MAX_NORM)
    x, y = batch()
    if strategy == "ddp":
        model = tdsa.DDP(model)
        opt = tdsa.DDPSGD(model.named_parameters(), **kw)
    elif strategy == "zero2flat":
        model = tdsa.Zero2Flat(model)
        opt = tdsa.Zero2FlatSGD(model, **kw)
    else:
        with torch.device("meta"):
            meta = GPT2Model(make_cfg())
        parts, _ = tdsa.partition_tensors(
            OrderedDict(meta.named_parameters()), ranks_map)
        wrap = {"zero1": tdsa.Zero1, "zero2": tdsa.Zero2,
                "zero3": tdsa.Zero3}[strategy]
        optc = {"zero1": tdsa.Zero1SGD, "zero2": tdsa.Zero2SGD,
                "zero3": tdsa.Zero3SGD}[strategy]
        model = wrap(model, parts)
        opt = optc(model.named_parameters(), param_part_table=parts,
                   ranks_map=ranks_map, **kw)
    losses, norms = [], []
    for _ in range(ITERS):
        model.require_backward_grad_sync = True
        _, loss = model(x, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        norms.append(float(opt.last_grad_norm))
    return losses, norms
