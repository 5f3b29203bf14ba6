"""The autotuner must actually gate dispatch: ops route through
``tuner.choose`` over a real candidate list, the measured winner is cached,
and a faster non-default candidate replaces the default (the reference
routes every op through a candidate list —
/root/reference/tiny_deepspeed/core/module/ops/linear.py:9-17).

CPU strategy: monkeypatch the op module's `_ext` seam so the "HIP" candidate
exists on CPU but is made artificially slow — the tuner must switch away
from it (candidate[0]) to the torch candidate. That proves the choice is
measured, not hardcoded.
"""

import importlib
import time

import pytest
import torch
import torch.nn.functional as F

from tiny_deepspeed_amd import ops
from tiny_deepspeed_amd.ops import linear as linear_ops
from tiny_deepspeed_amd.ops import layernorm as ln_ops
from tiny_deepspeed_amd.ops.autotuner import RuntimeAutoTuner, default_tuner

# the ops package re-exports functions named like these modules
ce_ops = importlib.import_module("tiny_deepspeed_amd.ops.cross_entropy")
emb_ops = importlib.import_module("tiny_deepspeed_amd.ops.embedding")
gelu_ops = importlib.import_module("tiny_deepspeed_amd.ops.gelu")


class _SlowFakeExt:
    """Pretends to be the HIP extension; correct numerics, penalized speed."""

    def column_sum(self, dy2):
        time.sleep(0.002)
        return dy2.sum(dim=0)

    def layernorm_fwd(self, x, w, b, eps, res=None):
        time.sleep(0.002)
        assert res is None
        return ln_ops.ln_fwd_torch(x, w, b, eps)


@pytest.fixture
def fake_ext(monkeypatch):
    ext = _SlowFakeExt()
    for mod in (linear_ops, ln_ops):
        monkeypatch.setattr(mod._ext, "use_native", lambda *t: True)
        monkeypatch.setattr(mod._ext, "get_ext", lambda: ext)
    return ext


def test_bias_grad_switches_to_faster_candidate(fake_ext):
    tuner = RuntimeAutoTuner(warmup=1, iters=3)
    dy = torch.randn(64, 32)
    out = linear_ops.linear_bias_grad(dy, tuner=tuner)
    torch.testing.assert_close(out, dy.sum(dim=0))
    choices = tuner.choices()
    assert len(choices) == 1
    # candidate[0] is db_hip (the fake, slowed); the tuner must have
    # measured and switched to db_torch
    assert list(choices.values())[0] == "db_torch"


def test_layernorm_fwd_switches_and_caches(fake_ext):
    tuner = RuntimeAutoTuner(warmup=1, iters=3)
    x = torch.randn(8, 64)
    w = torch.ones(64)
    b = torch.zeros(64)
    y, mean, rstd = ln_ops.layernorm_fwd(x, w, b, tuner=tuner)
    ref_y, ref_mean, ref_rstd = ln_ops.ln_fwd_torch(x, w, b, 1e-5)
    torch.testing.assert_close(y, ref_y)
    assert list(tuner.choices().values())[0] == "ln_fwd_torch"
    # cached: second call must dispatch straight to the stored winner
    calls = []
    orig = ln_ops.ln_fwd_torch
    key = next(iter(tuner._best))
    tuner._best[key] = lambda *a: (calls.append(1), orig(*a[:3], a[3]))[1]
    ln_ops.layernorm_fwd(x, w, b, tuner=tuner)
    assert calls == [1]


def test_same_op_different_shapes_tuned_separately(fake_ext):
    tuner = RuntimeAutoTuner(warmup=1, iters=2)
    linear_ops.linear_bias_grad(torch.randn(64, 32), tuner=tuner)
    linear_ops.linear_bias_grad(torch.randn(128, 16), tuner=tuner)
    assert len(tuner.choices()) == 2


def test_final_tune_freezes_unseen_keys_to_default(fake_ext):
    tuner = RuntimeAutoTuner(warmup=1, iters=2)
    tuner.final_tune()
    dy = torch.randn(32, 8)
    out = linear_ops.linear_bias_grad(dy, tuner=tuner)
    torch.testing.assert_close(out, dy.sum(dim=0))
    assert tuner.choices() == {}  # no tuning after freeze; default ran


def test_tuner_cache_roundtrip(fake_ext, tmp_path):
    """save_cache/load_cache: a second tuner adopts the first one's winners
    without re-measuring (used for tuning-noise-free rocprof captures)."""
    path = str(tmp_path / "tuner.json")
    t1 = RuntimeAutoTuner(warmup=1, iters=3)
    dy = torch.randn(64, 32)
    linear_ops.linear_bias_grad(dy, tuner=t1)
    assert list(t1.choices().values()) == ["db_torch"]
    t1.save_cache(path)

    t2 = RuntimeAutoTuner(warmup=1, iters=3)
    t2.load_cache(path)
    calls = []
    orig_time = t2._time_one
    t2._time_one = lambda *a, **k: (calls.append(1), orig_time(*a, **k))[1]
    out = linear_ops.linear_bias_grad(dy, tuner=t2)
    torch.testing.assert_close(out, dy.sum(dim=0))
    assert calls == []  # no measurement ran
    assert list(t2.choices().values()) == ["db_torch"]


def test_default_tuner_disabled_by_env(monkeypatch):
    import tiny_deepspeed_amd.ops.autotuner as at
    monkeypatch.setenv("TDSA_AUTOTUNE", "0")
    assert default_tuner() is None
    monkeypatch.delenv("TDSA_AUTOTUNE")
    # CPU container: no GPU -> nothing to tune either way
    if not torch.cuda.is_available():
        assert default_tuner() is None


def test_ops_fall_back_cleanly_without_tuner():
    # tuner=None on CPU: single torch candidate, no tuner machinery touched
    dy = torch.randn(16, 4)
    torch.testing.assert_close(ops.linear_bias_grad(dy), dy.sum(dim=0))


# ---- what every tuned op hands to the tuner -------------------------------
class _TorchBackedExt:
    """Stands in for the extension on CPU: every entry point the op modules
    call, computed by the op's own torch candidate."""

    def gelu_fwd(self, x):
        return gelu_ops.gelu_fwd_torch(x)

    def gelu_bwd(self, dy, x):
        return gelu_ops.gelu_bwd_torch(dy, x)

    def cross_entropy_fwd(self, logits, targets, ignore_index):
        return ce_ops.ce_fwd_torch(logits, targets, ignore_index)

    def cross_entropy_bwd(self, logits, targets, lse, dloss, n_valid,
                          ignore_index, out=None):
        return ce_ops.ce_bwd_torch(dloss, logits, targets, lse, n_valid,
                                   ignore_index, out)

    def embedding_fwd(self, weight, idx):
        return emb_ops.emb_fwd_torch(weight, idx)

    def embedding_bwd(self, dy, idx, num_embeddings, padding_idx):
        return emb_ops.emb_bwd_torch(idx, dy.float(), num_embeddings,
                                     None if padding_idx == -1 else padding_idx)

    def layernorm_fwd(self, x, w, b, eps, res=None):
        if res is None:
            return ln_ops.ln_fwd_torch(x, w, b, eps)
        h, y, mean, rstd = ln_ops.ln_fwd_res_torch(x, res, w, b, eps)
        return y, mean, rstd, h

    def layernorm_bwd_dx(self, dy, x, w, mean, rstd, dh=None):
        dx, ws = ln_ops.ln_dx_torch(dy, x, w, mean, rstd, dh)
        dw, db = ln_ops.layernorm_dwdb(ws)
        return dx, dw.unsqueeze(0), db.unsqueeze(0)

    def column_sum(self, dy2):
        return dy2.sum(dim=0)


class _RecordingTuner:
    def __init__(self):
        self.calls = []

    def choose(self, op, candidates, *args):
        self.calls.append((op, [c.__name__ for c in candidates], args))
        return candidates[0](*args)


@pytest.fixture
def kernel_path_on_cpu(monkeypatch):
    """The op modules take their kernel path on CPU tensors: the `_ext` seam
    reports a native extension whose entry points are the torch candidates."""
    ext = _TorchBackedExt()
    monkeypatch.setattr(ln_ops._ext, "use_native", lambda *t: True)
    monkeypatch.setattr(ln_ops._ext, "get_ext", lambda: ext)
    return _RecordingTuner()


def _kinds(args):
    return [(tuple(a.shape), a.dtype) if isinstance(a, torch.Tensor) else a
            for a in args]


def test_tuned_ops_candidates_and_argument_order(kernel_path_on_cpu):
    """What the tuner cache file stores for every op outside attention: the
    op name, the candidates' names with HIP first, and the order and kinds
    of the arguments given to choose (the tensor ones make the shape key)."""
    tuner = kernel_path_on_cpu
    g = torch.Generator().manual_seed(0)
    f32, i64 = torch.float32, torch.int64
    x = torch.randn(2, 3, 8, generator=g)
    dy = torch.randn(2, 3, 8, generator=g)
    w, b = torch.randn(8, generator=g), torch.randn(8, generator=g)

    torch.testing.assert_close(gelu_ops.gelu_fwd(x, tuner=tuner),
                               gelu_ops.gelu_fwd_torch(x))
    torch.testing.assert_close(gelu_ops.gelu_bwd(dy, x, tuner=tuner),
                               gelu_ops.gelu_bwd_torch(dy, x))

    logits = torch.randn(6, 8, generator=g)
    targets = torch.tensor([0, 7, 3, -100, 1, 2])
    loss_sum, lse, n_valid = ce_ops.cross_entropy_fwd(logits, targets, -100,
                                                      tuner=tuner)
    ref = F.cross_entropy(logits, targets, ignore_index=-100, reduction="sum")
    torch.testing.assert_close(loss_sum, ref)
    dloss = torch.tensor(1.0)
    ce_ops.cross_entropy_bwd(dloss, logits, targets, lse, n_valid, -100,
                             tuner=tuner)

    table = torch.randn(10, 4, generator=g)
    idx = torch.tensor([[1, 9, 1], [0, 3, 1]])
    out = emb_ops.embedding_forward(table, idx, None, tuner=tuner)
    torch.testing.assert_close(out, table[idx])
    demb = torch.randn(2, 3, 4, generator=g)
    emb_ops.embedding_weight_grad(idx, demb, 10, None, tuner=tuner)

    y, mean, rstd = ln_ops.layernorm_fwd(x, w, b, tuner=tuner)
    torch.testing.assert_close(y, F.layer_norm(x, (8,), w, b))
    ln_ops.layernorm_fwd_res(x, dy, w, b, tuner=tuner)
    ln_ops.layernorm_dx(dy, x, w, mean, rstd, None, tuner=tuner)

    torch.testing.assert_close(linear_ops.linear_bias_grad(dy, tuner=tuner),
                               dy.reshape(-1, 8).sum(0))
    n_before = len(tuner.calls)
    dw = linear_ops.linear_weight_grad(dy, x, tuner=tuner)
    torch.testing.assert_close(dw, dy.reshape(-1, 8).t() @ x.reshape(-1, 8))
    # linear_dw on CPU tensors: the single candidate dw_library runs; with
    # one candidate there is nothing to choose and the tuner is not asked
    assert tuner.calls[n_before:] == []
    assert not linear_ops._dw_hip_supported(dy.reshape(-1, 8), x.reshape(-1, 8))

    assert [(op, names) for op, names, _ in tuner.calls] == [
        ("gelu_fwd", ["gelu_fwd_hip", "gelu_fwd_torch"]),
        ("gelu_bwd", ["gelu_bwd_hip", "gelu_bwd_torch"]),
        ("ce_fwd", ["ce_fwd_hip", "ce_fwd_torch"]),
        ("ce_bwd", ["ce_bwd_hip", "ce_bwd_torch"]),
        ("emb_fwd", ["emb_fwd_hip", "emb_fwd_torch"]),
        ("emb_bwd", ["emb_bwd_hip", "emb_bwd_torch"]),
        ("ln_fwd", ["ln_fwd_hip", "ln_fwd_torch"]),
        ("ln_fwd_res", ["ln_fwd_res_hip", "ln_fwd_res_torch"]),
        ("ln_dx", ["ln_dx_hip", "ln_dx_torch"]),
        ("linear_db", ["db_hip", "db_torch"]),
    ]
    t3, vec, rows = ((2, 3, 8), f32), ((8,), f32), ((2, 3), f32)
    assert [_kinds(args) for _, _, args in tuner.calls] == [
        [t3],                                                  # gelu_fwd
        [t3, t3],                                              # gelu_bwd
        [((6, 8), f32), ((6,), i64), -100],                    # ce_fwd
        [((), f32), ((6, 8), f32), ((6,), i64), ((6,), f32), ((), i64),
         -100, None],                                          # ce_bwd
        [((10, 4), f32), ((2, 3), i64), None],                 # emb_fwd
        [((6,), i64), ((6, 4), f32), 10, None],                # emb_bwd
        [t3, vec, vec, 1e-5],                                  # ln_fwd
        [t3, t3, vec, vec, 1e-5],                              # ln_fwd_res
        [t3, t3, vec, rows, rows, None],                       # ln_dx
        [((6, 8), f32)],                                       # linear_db
    ]
    # the tensors themselves are handed on, not copies
    assert tuner.calls[0][2][0] is x
    assert tuner.calls[3][2][1] is logits


@pytest.mark.parametrize("dtype,V", [(torch.float32, 6), (torch.bfloat16, 12)])
def test_cross_entropy_off_width_vocab_never_reaches_tuner(
        kernel_path_on_cpu, dtype, V):
    """V % W != 0 (W = 4 fp32, 8 bf16): the kernels cannot take the rows, so
    the composite runs directly and the tuner never sees the shape."""
    tuner = kernel_path_on_cpu
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(5, V, generator=g).to(dtype)
    targets = torch.tensor([0, 1, -100, V - 1, 2])
    loss_sum, lse, n_valid = ce_ops.cross_entropy_fwd(logits, targets, -100,
                                                      tuner=tuner)
    ref = F.cross_entropy(logits.float(), targets, ignore_index=-100,
                          reduction="sum")
    torch.testing.assert_close(loss_sum, ref)
    dlogits = ce_ops.cross_entropy_bwd(1.0, logits, targets, lse, n_valid,
                                       -100, tuner=tuner)
    assert dlogits.shape == logits.shape and dlogits.dtype == dtype
    assert tuner.calls == []
