"""Runtime autotuner: picks the fastest candidate implementation of an op.

Same capability as the reference's RuntimeAutoTuner
(``/root/reference/tiny_deepspeed/core/autotuner/runtime_tuner.py:7-39``),
re-designed for MI355X: timing uses hipEvents (torch.cuda.Event) instead of
host wall-clock so the measurement covers device time only, and candidates
are keyed per input-shape/dtype so one module can serve several shapes.

Candidates are callables taking identical args. The default (index 0) is the
hand-written HIP kernel; later entries are library/torch fallbacks.
"""

import os
import time

import torch

from . import _ext


class RuntimeAutoTuner:
    def __init__(self, enabled: bool = True, warmup: int = 5, iters: int = 20):
        self.enabled = enabled
        self.warmup = warmup
        self.iters = iters
        self._best = {}  # (op_name, key) -> callable
        self._preloaded = {}  # repr(key) -> winner __name__ (cache file)
        self.finalized = False

    @staticmethod
    def _key(args):
        parts = []
        for a in args:
            if isinstance(a, torch.Tensor):
                parts.append((tuple(a.shape), str(a.dtype)))
        return tuple(parts)

    def choose(self, op_name, candidates, *args, **kwargs):
        """Run the best candidate (tuning on first sight of a new key)."""
        if not self.enabled or len(candidates) == 1:
            return candidates[0](*args, **kwargs)
        key = (op_name, self._key(args))
        fn = self._best.get(key)
        if fn is not None:
            return fn(*args, **kwargs)
        if self._preloaded:
            name = self._preloaded.get(repr(key))
            for c in candidates:
                if c.__name__ == name:
                    self._best[key] = c
                    return c(*args, **kwargs)
        if self.finalized:
            # after final_tune(), unseen keys use the default candidate
            return candidates[0](*args, **kwargs)
        fn, out = self._tune(candidates, args, kwargs)
        self._best[key] = fn
        return out

    def _time_one(self, fn, args, kwargs):
        on_gpu = any(isinstance(a, torch.Tensor) and a.is_cuda for a in args)
        if on_gpu:
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            for _ in range(self.warmup):
                fn(*args, **kwargs)
            start.record()
            for _ in range(self.iters):
                fn(*args, **kwargs)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / self.iters
        for _ in range(self.warmup):
            fn(*args, **kwargs)
        t0 = time.perf_counter()
        for _ in range(self.iters):
            fn(*args, **kwargs)
        return (time.perf_counter() - t0) * 1e3 / self.iters

    def _tune(self, candidates, args, kwargs):
        best_fn, best_ms = None, float("inf")
        for fn in candidates:
            try:
                ms = self._time_one(fn, args, kwargs)
            except Exception:
                continue
            if ms < best_ms:
                best_fn, best_ms = fn, ms
        if best_fn is None:
            best_fn = candidates[0]
        return best_fn, best_fn(*args, **kwargs)

    def final_tune(self):
        """Freeze the choices made so far (reference parity: ``final_tune``)."""
        self.finalized = True

    def choices(self):
        """{(op_name, shape_key): chosen callable __name__} — introspection
        for tests and for logging which implementation won per shape."""
        return {k: fn.__name__ for k, fn in self._best.items()}

    # --- cache file (like TunableOp's): lets a second process skip the
    # measurement phase entirely — used to capture rocprof traces free of
    # candidate-timing noise, and to pin choices for reproducibility -----
    def save_cache(self, path):
        import json

        with open(path, "w") as f:
            json.dump({repr(k): fn.__name__ for k, fn in self._best.items()},
                      f, indent=1, sort_keys=True)

    def load_cache(self, path):
        import json

        with open(path) as f:
            self._preloaded = json.load(f)


_DEFAULT_TUNER = None


def default_tuner():
    """Process-wide tuner used by the op layer when the module didn't pass
    one. Live on GPU by default — every op with >1 candidate implementation
    dispatches through measured choice (the reference routes every op
    through a candidate list, /root/reference/tiny_deepspeed/core/module/
    ops/linear.py:9-17). ``TDSA_AUTOTUNE=0`` disables (candidate[0], the
    hand-written kernel, runs unconditionally); on CPU there is nothing to
    tune (single torch candidate) so None is returned."""
    global _DEFAULT_TUNER
    if os.environ.get("TDSA_AUTOTUNE", "1") == "0":
        return None
    if not torch.cuda.is_available():
        return None
    if _DEFAULT_TUNER is None:
        _DEFAULT_TUNER = RuntimeAutoTuner()
        cache = os.environ.get("TDSA_TUNER_CACHE")
        if cache:
            if os.path.exists(cache):
                _DEFAULT_TUNER.load_cache(cache)
            else:
                import atexit

                def _save():
                    try:
                        if _DEFAULT_TUNER is not None:
                            _DEFAULT_TUNER.save_cache(cache)
                    except OSError:
                        pass  # cache is an optimization; never fail exit

                atexit.register(_save)
    return _DEFAULT_TUNER


def dispatch(op_name, candidates, args, on, tuner=None, supported=True):
    """The one choice every tuned {HIP kernel, torch} op makes. candidates is
    [hip, torch]; `on` is the tensor whose device decides; `supported` is the
    op's own "the kernel takes this shape" test. Without a native extension
    for `on`, or with an unsupported shape, the torch candidate runs and the
    tuner never sees the call. Otherwise the tuner (the given one, else the
    process default) picks; without a tuner the HIP kernel runs."""
    hip, composite = candidates
    if not (_ext.use_native(on) and supported):
        return composite(*args)
    tuner = tuner if tuner is not None else default_tuner()
    if tuner is not None:
        return tuner.choose(op_name, candidates, *args)
    return hip(*args)
