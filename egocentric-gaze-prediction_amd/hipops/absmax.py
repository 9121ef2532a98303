"""Abs-max scalars of activations and gradients (the scale of their f16 split), and hipGraph capture."""
from __future__ import annotations

import sys

import torch

from .._lib import check
from ._core import LIB, _req, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


class _AbsmaxArena:
    """Zero-filled abs-max buffers (egz_common.h: the producers fold their maxima in with atomic max, so a buffer must start at
    zero).  Buffers are cut from chunks that ONE fill zeroes (a chunk serves ~250 buffers = about one SP step); a chunk is
    filled on the stream that was current when it was created and every other stream that takes a buffer from it waits for
    that fill once.  A hipGraph capture gets ONE chunk of its own (CAPTURE_CHUNK buffers), created by ``capture()`` below on
    the capture's origin stream before any side stream forks: the captured fill re-zeroes it on every replay, buffers handed
    out before / after the capture are never touched by it, and a capture that needs more buffers than the chunk holds raises
    (a second chunk created mid-capture on a forked stream would not be ordered before the other streams' atomic maxima --
    ADVICE r4).  Captures must go through ``capture()``: take() inside a capture that did not raises."""
    CHUNK = 256
    CAPTURE_CHUNK = 1024

    def __init__(self):
        self.elems = 0
        self.chunk = None
        self.size = 0
        self.used = 0
        self.tag = None
        self.event = None
        self.waited = set()
        self.capture_seq = 0
        self.in_capture = False

    def capture_begin(self, device, eager: bool = True):
        """First statement inside a hipGraph capture (``capture()``): the capture's buffers come from a chunk of its own whose
        fill is captured HERE, on the capture's origin stream, before any side stream forks.  ``eager=False``: a capture that
        stays on one stream and may not take a buffer at all (the AT per-sample step: its replay would zero the chunk for
        nothing, one launch per sample) -- the chunk is then created by the first take() inside the capture."""
        self.capture_seq += 1
        self.chunk = None
        self.in_capture = True
        if eager:
            self.take(device)

    def capture_end(self):
        self.in_capture = False
        self.chunk = None                 # the next eager take() starts a chunk of its own

    def take(self, device) -> torch.Tensor:
        if not self.elems:
            self.elems = int(LIB.egz_absmax_elems())
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and not self.in_capture:
            raise RuntimeError("abs-max arena: a hipGraph capture that did not go through hipops.capture() asked for a buffer "
                               "(it would share the previous capture's chunk)")
        tag = (capturing, self.capture_seq if capturing else 0, str(device))
        if self.chunk is None or self.used == self.size or tag != self.tag:
            if capturing and self.chunk is not None and tag == self.tag:
                raise RuntimeError(f"abs-max arena: the capture needs more than {self.size} abs-max buffers "
                                   "(raise _AbsmaxArena.CAPTURE_CHUNK)")
            self.size = self.CAPTURE_CHUNK if capturing else self.CHUNK
            self.chunk = torch.zeros(self.size * self.elems, dtype=torch.int32, device=device)
            self.used, self.tag = 0, tag
            if capturing:
                self.event = None                    # inside a capture the forked streams are ordered by the capture graph itself
            else:
                self.event = torch.cuda.Event()
                self.event.record()
            self.waited = {_stream()}
        elif self.event is not None:
            raw = _stream()                           # (the raw handle: ~0.3 us; a Stream object only when this stream has to wait)
            if raw not in self.waited:
                torch.cuda.current_stream().wait_event(self.event)
                self.waited.add(raw)
        buf = self.chunk[self.used * self.elems:(self.used + 1) * self.elems]
        self.used += 1
        return buf




class capture:
    """``with hipops.capture(graph[, eager_arena=False]): ...`` = ``torch.cuda.graph(graph)`` plus what this package's launches
    need inside a capture: the abs-max arena's per-capture chunk (see _AbsmaxArena).  Every capture site of the package goes
    through here (graphs.GraphedModule / GraphedTrainStep; AT._GraphedSampleStep, training and validation).
    After the block ``written`` holds the tensors the captured launches were declared to write (hipops.touch_params: the fused
    optimizer's parameters, BatchNorm running means) and ``rebuilt`` the keys of the packings they rebuild: hipops.note_replay."""

    def __init__(self, graph, eager_arena: bool = True, **kw):
        self.ctx = torch.cuda.graph(graph, **kw)
        self.eager_arena = eager_arena
        self.written, self.rebuilt = [], []

    def __enter__(self):
        # the persistent LSTM launches keep their hand-off scratch per (device, stream), zeroed ONCE when it is allocated (its
        # sticky error words must survive replays): a buffer allocated inside the capture would come from the graph's pool and
        # be re-zeroed by nothing / by every replay -- so the capture stream's scratch is created here, eagerly, before the
        # capture begins (torch.cuda.graph synchronises the device on entry: the zero fill has landed by then)
        st = getattr(self.ctx, "capture_stream", None)
        if st is not None and _H.LSTM_PERSIST:
            _H._persist_sync(torch.device("cuda", torch.cuda.current_device()), st.cuda_stream)
        self.ctx.__enter__()
        try:
            _H.ABSMAX_ARENA.capture_begin(torch.device("cuda", torch.cuda.current_device()), eager=self.eager_arena)
        except BaseException:
            _H.ABSMAX_ARENA.capture_end()
            self.ctx.__exit__(None, None, None)
            raise
        _H._CAPTURE_LOG[0] = ([], [])
        return self

    def __exit__(self, *exc):
        # what the captured launches write behind torch's back, and the packings they rebuild after it: the host side of those
        # declarations ran once, here; the owner of the graph repeats it after every replay (hipops.note_replay)
        log, _H._CAPTURE_LOG[0] = _H._CAPTURE_LOG[0], None
        if log is not None:
            self.written = list({id(t): t for t in log[0]}.values())
            self.rebuilt = list(dict.fromkeys(log[1]))
        _H.ABSMAX_ARENA.capture_end()
        return self.ctx.__exit__(*exc)


def _new_absmax(device) -> torch.Tensor:
    """A zero-filled abs-max buffer (32 slots, one per 128-byte line; see egz_common.h and _AbsmaxArena)."""
    return _H.ABSMAX_ARENA.take(device)


def absmax_value(am: torch.Tensor) -> torch.Tensor:
    """max |x| held by an abs-max buffer, as a 1-element float32 tensor (the maximum over its slots)."""
    return am.view(32, -1)[:, 0].max().reshape(1).view(torch.float32)


def _want_absmax() -> bool:
    return _H.PRECISION == "split" and _H.GRAD_SPLIT == "f16"


# Forward activations get the same treatment as gradients: the pass that WRITES a post-ReLU activation (BN apply + ReLU
# [+ pool], the bias + ReLU epilogue of a decoder conv) also emits max |a|, and the consuming convolution (forward operand)
# and weight gradient (x operand) multiply by the matching power of two before the f16 split -- without it the pair's 22 bits
# only hold for max |a| in [2^-3, 65504] (lo goes subnormal below, hi saturates above).
# (hipops.FWD_SCALE; test_forward_scaling_off_loses_the_small_range turns it off.)
ABSMAX_STATS = {"standalone": 0}         # standalone egz_absmax passes (an operand arrived without its producer's abs-max)


def _want_fwd_absmax() -> bool:
    return _H.PRECISION == "split" and _H.FWD_SCALE


def carry_absmax(dst: torch.Tensor, src) -> torch.Tensor:
    """Hand the abs-max scalar of ``src`` (a tensor or the scalar buffer itself) on to ``dst`` -- a view / re-layout of the same
    values (permutes and detaches create new tensor objects, which drop Python attributes)."""
    am = getattr(src, "_egz_absmax", None) if isinstance(src, torch.Tensor) and src.dtype != torch.int32 else src
    if am is not None:
        dst._egz_absmax = am
    if isinstance(src, torch.Tensor) and getattr(src, "_egz_presplit", False):
        dst._egz_presplit = True          # (the tensor holds f16 pairs, not fp32 values: see PRESPLIT)
    return dst


def absmax_of(x: torch.Tensor) -> torch.Tensor:
    """The abs-max scalar of a gradient tensor: the one its producer kernel attached (bn_relu_pool_bwd, relu_bwd_bias,
    pairmax_bwd compute it in their own pass), else a standalone reduction (egz_absmax)."""
    am = getattr(x, "_egz_absmax", None)
    if am is None:
        _req(x, "x")
        am = _new_absmax(x.device)
        ABSMAX_STATS["standalone"] += 1
        check(LIB.egz_absmax(x.data_ptr(), x.numel(), am.data_ptr(), _stream()), "egz_absmax")
        x._egz_absmax = am
    return am
