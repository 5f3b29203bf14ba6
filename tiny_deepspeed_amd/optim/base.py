"""From-scratch optimizer base over an OrderedDict of named parameters.

Parity with ``/root/reference/tiny_deepspeed/core/optim/base.py:7-26``
(step() loops one_step(name, param) then clears grads), with two additions
the reference lacks: state_dict/load_state_dict for checkpointing
 and a pre_step/post_step hook pair the distributed
optimizers use to order communication around the update.

Gradient clipping by global norm (``max_grad_norm``) lives here, between
pre_step() and the update, because that is the only point where the reduced
gradients can be read: the squares of this rank's gradients are summed in one
launch, _reduce_sumsq() makes the sum global (a hook the sharded optimizers
override), and the clip coefficient stays on the device as the gradient scale
of the fused update, so a clipped step costs one extra read of the gradients
and no host synchronisation.
"""

from collections import OrderedDict

import torch

from .. import ops
from ..utils.profiling import trace_range


class Optimizer:
    def __init__(self, parameters, lr, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        # accepts an iterator of (name, param) like model.named_parameters()
        self.params = OrderedDict(parameters)
        for name, p in self.params.items():
            if not isinstance(p, torch.nn.Parameter):
                raise TypeError(f"{name} is not an nn.Parameter")
        self.lr = lr
        self.t = 0  # global step count (advances once per step(), not per
        # parameter — the reference advances it per tensor, a bias-correction
        # bug we do not replicate: SURVEY.md 2.11.1 / adamw.py:59)
        # clip the global gradient norm to this value (None: no clipping);
        # a hyper-parameter like lr's siblings, not part of the state dict
        self.max_grad_norm = max_grad_norm
        # pre-clip global norm of the last step: 0-dim fp32 tensor on the
        # gradients' device; None without clipping or before the first step
        self.last_grad_norm = None
        self._grad_scale = None  # clip coefficient of the step in flight

    # --- hooks for distributed subclasses --------------------------------
    def pre_step(self):
        pass

    def post_step(self):
        pass

    def _should_update(self, name, param):
        return param.grad is not None

    @torch.no_grad()
    def step(self):
        self.t += 1
        with trace_range("tdsa:optimizer.step"):
            self._run_step()

    @torch.no_grad()
    def _run_step(self):
        self.pre_step()
        items = [(n, p) for n, p in self.params.items()
                 if self._should_update(n, p)]
        self._clip(items)
        self._apply_updates(items)
        self.post_step()
        for param in self.params.values():
            param.grad = None

    def _clip(self, items):
        """Sets last_grad_norm and the gradient scale of this step's update
        from the gradients of `items` (after pre_step(): they are final)."""
        if self.max_grad_norm is None:
            return
        sumsq = ops.grad_sumsq([p.grad for _, p in items],
                               device=self._norm_device())
        # every rank gets here every step, also with nothing to update
        sumsq = self._reduce_sumsq(sumsq)
        self.last_grad_norm, self._grad_scale = ops.clip_coef(
            sumsq, self.max_grad_norm)

    def _norm_device(self):
        """Where the norm of an empty gradient list lives."""
        for p in self.params.values():
            return p.device
        return None

    def _reduce_sumsq(self, sumsq):
        """Local sum of squares -> global one. Identity here and under DDP,
        whose gradients are replicated; the sharded optimizers all-reduce."""
        return sumsq

    def _apply_updates(self, items):
        """Default: per-parameter updates. AdamW overrides this with one
        fused multi-tensor kernel launch on GPU (csrc/kernels/optim.hip)."""
        for name, param in items:
            self.one_step(name, param)

    @torch.no_grad()
    def zero_grad(self):
        for param in self.params.values():
            param.grad = None

    def one_step(self, name, param):
        raise NotImplementedError

    # --- checkpointing ----------------------------------------------------
    def _state_tensors(self):
        """Subclasses return {key: {name: tensor}} of optimizer state."""
        return {}

    def state_dict(self):
        sd = {"t": self.t, "lr": self.lr, "state": {}}
        for key, per_param in self._state_tensors().items():
            sd["state"][key] = {n: t for n, t in per_param.items() if t is not None}
        return sd

    def load_state_dict(self, sd):
        self.t = sd["t"]
        self.lr = sd["lr"]
        own = self._state_tensors()
        for key, per_param in sd["state"].items():
            if key not in own:
                continue
            for n, t in per_param.items():
                if n in own[key] and own[key][n] is not None:
                    own[key][n].copy_(t.to(own[key][n].device))
