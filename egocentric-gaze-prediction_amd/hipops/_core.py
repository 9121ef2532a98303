"""What every family shares: the profiler, the one library proxy, stream / pointer helpers, the workspace, the launch status
word."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from .._lib import LIB as _RAW_LIB


EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_STATS = 0, 1, 2


class _Profiler:
    """Optional per-entry-point timing with HIP events recorded on the launch stream (the stream every
    C-ABI call is issued on is torch's current stream, so torch.cuda.Event brackets exactly those kernels).
    Used by bench.py's roofline leg; off by default (zero overhead beyond one attribute test)."""

    def __init__(self):
        self.enabled = False
        self.events = {}
        self.flops = {}

    def start(self):
        self.events, self.flops, self.enabled = {}, {}, True

    def stop(self):
        """-> {entry point: {'calls', 'ms', 'flops'}}"""
        self.enabled = False
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.events.items():
            out[name] = {"calls": len(evs), "ms": sum(a.elapsed_time(b) for a, b in evs),
                         "flops": self.flops.get(name, 0.0)}
        for name, v in self.flops.items():      # FLOPs noted under a family name none of whose own launches ran in this step
            out.setdefault(name, {"calls": 0, "ms": 0.0, "flops": v})
        return out

    def note_flops(self, name, v):
        if self.enabled:
            self.flops[name] = self.flops.get(name, 0.0) + v


PROF = _Profiler()


class _LibProxy:
    def __init__(self, raw):
        self._raw = raw

    def __getattr__(self, name):
        fn = getattr(self._raw, name)

        def call(*a):
            if not PROF.enabled or name.endswith(("_bytes", "_rows", "_elems", "_ok", "_splits")):   # host-side queries launch nothing
                return fn(*a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            PROF.events.setdefault(name, []).append((e0, e1))
            return rc
        setattr(self, name, call)
        return call


LIB = _LibProxy(_RAW_LIB)


# Every C-ABI launch asks for the current stream: torch.cuda.current_stream() builds a Stream object through several Python
# layers (~10 us per call, measured: 7 calls = 67 us of a 436 us AT sample step); the raw-handle accessor costs ~0.3 us.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous buffer, got strides {t.stride()} for {tuple(t.shape)}")
    return t


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _out(out: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """A kernel output: a fresh tensor, or the caller's destination (e.g. a gradient sink) viewed with that shape."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    n = 1
    for d in shape:
        n *= d
    if out.numel() != n or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"output buffer {tuple(out.shape)} / {out.dtype} does not fit {tuple(shape)} fp32 contiguous")
    return out.view(shape)


# ----------------------------------------------------------------------------- workspace
_WS = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Stream-ordered scratch (one buffer per device AND stream, grown on demand; the C-ABI never allocates).
    Keyed by stream because kernels on different HIP streams run concurrently (streams.py)."""
    key = (torch.device(device).index or 0, _stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _ptr_table(tensors):
    """Host array of device pointers (None -> NULL) for the C-ABI entry points that take a parameter table."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


# ----------------------------------------------------------------------------- the launch status word
class LaunchStatus(NamedTuple):
    """The status word of one launch on its way to the host: ``host`` a one-word pinned tensor the device word is being
    copied into, ``event`` recorded behind that copy.  A plain tuple to its readers: ``host, event = pending``."""
    host: torch.Tensor
    event: object

    def wait(self) -> int:
        """Waits for the launch -> its status word."""
        self.event.synchronize()
        return int(self.host[0])


def finish_launch(status: torch.Tensor, status_to: Optional[dict], key: str, judge) -> None:
    """The tail of every op that ends in a status word: the device word ``status`` is copied to pinned memory behind the
    launch (non-blocking) and an event recorded.  With ``status_to`` (a dict) the LaunchStatus is left there under ``key``
    for the caller to wait on later; without, this waits and hands the word to ``judge`` (int -> None: raises or warns)."""
    host = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(status, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    if status_to is not None:
        status_to[key] = LaunchStatus(host, done)
    else:
        judge(LaunchStatus(host, done).wait())


def drain_status(chunks, key: str, wait, judge, judge_resident) -> None:
    """Judges the status words of ``chunks`` = [(who, status_to dict)], every dict holding the word of a gather
    ('_resident_status') and of a store (``key``), all queued on ONE stream in this order.  The words were copied on that
    stream in order, so when the last one has landed all have: ``wait`` (the store's ``*_status`` function) is called once,
    on the last word, and the rest are read as they lie.  Per chunk ``judge_resident(word)`` comes before
    ``judge(word, who)``; ``who`` names the chunk in the store's errors."""
    if chunks:
        wait(chunks[-1][1][key])
    for who, status in chunks:
        judge_resident(int(LaunchStatus(*status['_resident_status']).host[0]))      # (a plain pair will do, as everywhere)
        judge(int(LaunchStatus(*status[key]).host[0]), who)
