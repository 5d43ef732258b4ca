"""The torch side of a call into libmzsearch.so, stated once: which device, which stream, what a kernel reads in
place, how an argument struct is launched, how a loop of such calls is captured into a graph, the weight struct of the
default MLP trio, and the base of the per-model objects that keep one (`FusedCall`).  (`_lib` itself stays free of
torch.)"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc

import torch

from . import _lib


def device_index(device) -> int:
    """The ordinal of a torch GPU device; one without an index (`cuda`) is the current device."""
    return device.index if device.index is not None else torch.cuda.current_device()


# torch's current stream of a device, raw: the stream a capture records on while one runs.  (torch.cuda.current_stream()
# builds a Stream object, ~6 us per call: only where the raw getter is missing.)
_raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
if _raw is not None:
    def raw_stream(dev_index: int) -> C.c_void_p:
        return C.c_void_p(_raw(dev_index))
else:
    def raw_stream(dev_index: int) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(dev_index).cuda_stream)


def as_device(x, dtype, device) -> torch.Tensor:
    """`x` as a contiguous tensor of `dtype` on `device`; one that already is all of that passes through untouched (the
    kernel reads the caller's own storage)."""
    if isinstance(x, torch.Tensor) and x.dtype == dtype and x.device == device and x.is_contiguous():
        return x
    return torch.as_tensor(x, device=device).to(dtype).contiguous()


def launch(entry: str, cls, device, *extra, handle=None, **fields):
    """entry(&args, *extra, stream) on `device`'s current stream: `args` a `cls` struct of `fields` with `device` set.
    A status other than MZS_OK raises (`_lib.check`).  The caller keeps the tensors behind the pointers alive."""
    dev = device_index(device)
    a = _lib.args(cls, device=dev, **fields)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), entry)(C.byref(a), *extra, raw_stream(dev)), handle)


@contextlib.contextmanager
def capture(graph):
    """`torch.cuda.graph(graph)` with Python's cyclic collector held off: dead cycles are collected before the capture
    begins, none during it.

    Why: torch.cuda.graph collects garbage on entry only under torch.compiler.config.force_cudagraph_gc (it used to do
    so always), so a collection can start at any allocation of the captured Python code.  With the call sites of nn.py
    going through `launch` and `_memo` (more short-lived tuples and dicts per call than the hand-written preambles), the
    whole suite in one process aborted (SIGABRT) in test_resnet_plugin_nets_drive_the_stepwise_search: faulthandler
    showed the collector starting ("Garbage-collecting") at the signature tuple of nn._memo, inside the captured loop of
    MuZeroSearch._run_loop, with no Python finaliser frame -- a C-level destructor.  Supposed, not traced: the
    CUDAGraph of an earlier test's unreachable model (models and their handles live on in reference cycles), whose
    destructor synchronises the device on ROCm, which a capture forbids.  With this guard the same run passes.  The
    hazard was there before, at whichever allocation crossed the collector's threshold."""
    gc.collect()
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if enabled:
            gc.enable()


class MlpWeights:
    """The MzsMlpWeights struct of the default trio's 18 parameter tensors (`params`, in MLP_WEIGHT_NAMES order), kept
    and rebuilt only when a tensor moved (optimisers update in place) or is not contiguous.  The callers set the scalar
    fields (obs_dim, support_size, discount) themselves.  `cls`, `names`: another weight struct of the same kind and its
    pointer members in the order of `params` (the stochastic family's 34: MzsStochasticTrainWeights)."""

    def __init__(self, params, cls=_lib.MzsMlpWeights, names=_lib.MLP_WEIGHT_NAMES):
        self.params, self._cls, self._names = params, cls, names
        self._w = self._keep = self._ptrs = None

    def get(self):
        """(struct, the tensors its pointers refer to: to be kept alive until the launch has run)"""
        ptrs = tuple(x.data_ptr() for x in self.params)
        if ptrs != self._ptrs or not all(x.is_contiguous() for x in self.params):
            keep = [x.detach().contiguous() for x in self.params]
            self._w = _lib.args(self._cls, **{n: x.data_ptr() for n, x in zip(self._names, keep)})
            self._keep = keep
            # a contiguous copy is not cached: it would go stale under an in-place update of its original
            self._ptrs = ptrs if all(k.data_ptr() == q for k, q in zip(keep, ptrs)) else None
        return self._w, self._keep


class FusedCall:
    """What the per-model objects that put one C entry on the current stream share (the fused training steps of loss.py,
    the value unrolls of unroll.py): the model, the library, `params` in the C ABI's order (`names`), the device they lie
    on -- a GPU, or the constructor refuses --, the support size, and the kept weight struct (`MlpWeights`)."""

    def __init__(self, muzero_instance, params, names, weight_struct):
        self.m = muzero_instance
        self.params = [params[n] for n in names]
        self.dev = self.params[0].device
        if self.dev.type != "cuda":
            raise RuntimeError("muax_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self._L = _lib.load()
        self.S = muzero_instance._support_size
        self._weights = MlpWeights(self.params, weight_struct, names)
