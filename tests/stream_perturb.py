"""Schedule perturbation for the stream-ordering tests (tests/test_hip_stream_order.py).

The package orders its HIP streams with stream waits only (streams.py and the hand-written sites listed in DESIGN.md, "Stream
concurrency").  At test sizes every kernel is over before the next one on another stream is issued, so a missing wait gives the right
numbers anyway.  This module makes a missing edge visible:

  serial()                  the oracle: ``streams.ENABLED = False``, every launch on the one current stream, no delays;
  perturb(mode, delay_ms)   bounded spin kernels (``torch.cuda._sleep``) in front of the work somebody else has to wait for;
  poison(h)                 0xFF bytes in every hipops workspace and in a spread of freed allocator blocks, so that a read that
                            comes too early returns NaN / garbage, never last step's identical values.

The hooks wrap Python functions and methods of torch and of the package from the test process; the product code has no seam for
them.  Nothing here touches environment variables or runtime settings, and a hook that finds its stream inside a hipGraph capture
raises (a spin kernel must not be captured).

Modes:
  "late_helper"  the helper stream is late: a delay on the side stream after ``side.wait_stream(cur)`` in ``streams.fork.__enter__``
                 and on entry to every ``torch.cuda.stream(...)`` region opened by package code (the h2d stream of
                 STdatas.staged_batches, AT's copy stream, dp's comm stream, graphs.py's warm-up stream, model_SP's
                 ``with torch.cuda.stream(f.side)``).  A consumer that does not join, or an input freed without record_stream, reads early.
  "late_waiter"  after every ``Stream.wait_stream`` / ``Stream.wait_event`` issued from package code, the stream that waited is delayed.
  "late_owner"   the CURRENT stream is delayed right before work other streams depend on through bespoke logic: before
                 ``_AbsmaxArena.take`` creates a chunk (so before its zero fill), before every weight-pack launch (packed_weight,
                 refresh_packings, repack_stale all end in one of the ``egz_pack_w3x3_*`` launches), before the launches of
                 ``prepare_network_input`` and before ``resident_gather``'s launch.
  "none"         no delay (the plain multi-stream run).

Hardware queues.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES (4) hardware queues, and streams that share a queue run
FIFO: a spin kernel on one of them holds the other back, and the race between the two stays hidden.  Which streams share is
fixed when they are created, so in a long test process it depends on every test that ran before (measured: in a fresh process the
abs-max scenario of the self-check is seen in 10 of 10 runs, behind the rest of the suite in 0 of 10).  ``perturb`` therefore
gives the package's helper streams of the current stream -- the shared ``wgrad`` stream, ``encoder_t`` and ``h2d`` -- streams of
torch's pool that were MEASURED (``shares_queue``) to sit on hardware queues of their own, apart from the current stream and
from each other: the layout the package has in a fresh process (main + encoder_t + wgrad + one more, streams.py), whatever ran
before.  The entries of ``streams._SIDE`` are put back on exit.
"""
import contextlib
import sys
import time

import torch

DEV = "cuda:0"
MODES = ("none", "late_helper", "late_waiter", "late_owner")
MAX_DELAY_MS = 20.0
PKG = "egaze_amd"
PACK_LAUNCHES = ("egz_pack_w3x3_fwd", "egz_pack_w3x3_dgrad", "egz_pack_w3x3_ups_fwd", "egz_pack_w3x3_ups_dgrad",
                 "egz_pack_w3x3_split", "egz_pack_w3x3_split_frag", "egz_pack_w3x3_frag_batch")

_CYCLES_PER_MS = [None]
_ORIG_STREAM_CTX = torch.cuda.stream            # the un-hooked context manager, for the hooks' own use
STATS = {"delays": 0}


def cycles_per_ms() -> float:
    """Spin cycles of ``torch.cuda._sleep`` per millisecond, measured once per session with two timing events."""
    if _CYCLES_PER_MS[0] is None:
        probe = 1_000_000
        torch.cuda.synchronize()
        torch.cuda._sleep(probe)                 # (first launch: module load)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        _CYCLES_PER_MS[0] = probe / max(e0.elapsed_time(e1), 1e-3)
    return _CYCLES_PER_MS[0]


def _from_package(depth: int = 2) -> bool:
    """The function ``depth`` frames up (the caller of the hooked function) belongs to the package."""
    name = sys._getframe(depth).f_globals.get("__name__", "")
    return name == PKG or name.startswith(PKG + ".")


def shares_queue(a, b, ms: float = 2.0) -> bool:
    """Measured: work on stream ``b`` is held back by a spin kernel of ``ms`` on stream ``a`` (they share a hardware queue)."""
    cycles = int(ms * cycles_per_ms())
    if _TICK[0] is None:
        _TICK[0] = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with _ORIG_STREAM_CTX(a):
        torch.cuda._sleep(cycles)
    with _ORIG_STREAM_CTX(b):
        _TICK[0].add_(1.0)                       # (a real launch: a marker alone need not travel through the queue)
        ev.record()
    t0 = time.perf_counter()
    ev.synchronize()
    held = time.perf_counter() - t0 > 0.5e-3 * ms
    torch.cuda.synchronize()
    return held


_TICK = [None]
_HELPERS = [None]
HELPER_KINDS = ("wgrad", "encoder_t", "h2d")


def helper_streams():
    """Up to three streams of torch's pool on hardware queues of their own: apart from the current stream and from each other
    (measured once per session; torch hands its 32 pool streams out round-robin)."""
    if _HELPERS[0] is None:
        cur = torch.cuda.current_stream()
        found = []
        for _ in range(40):
            if len(found) == len(HELPER_KINDS):
                break
            st = torch.cuda.Stream()
            others = [cur] + found
            if any(st.cuda_stream == o.cuda_stream for o in others) or any(shares_queue(o, st) for o in others):
                continue
            found.append(st)
        _HELPERS[0] = found
    return _HELPERS[0]


@contextlib.contextmanager
def spread_helpers():
    """The package's helper streams of the current stream on hardware queues of their own (see the module docstring)."""
    from egaze_amd import streams
    cur = streams.current()
    dev = cur.device.index
    keys = [(dev, 0 if kind in streams._SHARED else cur.cuda_stream, kind) for kind in HELPER_KINDS]
    missing = object()
    keep = {k: streams._SIDE.get(k, missing) for k in keys}
    torch.cuda.synchronize()
    for k, st in zip(keys, helper_streams()):
        streams._SIDE[k] = st
    try:
        yield
    finally:
        torch.cuda.synchronize()
        for k, st in keep.items():
            if st is missing:
                streams._SIDE.pop(k, None)
            else:
                streams._SIDE[k] = st


class _Delay:
    def __init__(self, delay_ms: float):
        if not 0 < delay_ms <= MAX_DELAY_MS:
            raise ValueError(f"delay of {delay_ms} ms: delays are bounded by {MAX_DELAY_MS} ms")
        self.cycles = int(delay_ms * cycles_per_ms())

    def current(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("stream_perturb: a delay inside a hipGraph capture (perturb() is for eager steps only)")
        torch.cuda._sleep(self.cycles)
        STATS["delays"] += 1

    def on(self, stream):
        with _ORIG_STREAM_CTX(stream):
            self.current()


@contextlib.contextmanager
def _patched(obj, name, make):
    """``obj.name = make(original)`` for the duration of the block."""
    orig = getattr(obj, name)
    setattr(obj, name, make(orig))
    try:
        yield
    finally:
        setattr(obj, name, orig)


@contextlib.contextmanager
def serial():
    """The oracle run: HIP-stream concurrency switched off (everything on the current stream), no delays."""
    from egaze_amd import streams
    keep = streams.ENABLED
    streams.ENABLED = False
    try:
        yield
    finally:
        streams.ENABLED = keep


def _late_helper(stack, d):
    from egaze_amd import streams

    def fork_enter(orig):
        def enter(self):
            res = orig(self)
            if self.enabled:
                d.current()                      # the current stream is the side stream now
            return res
        return enter
    stack.enter_context(_patched(streams.fork, "__enter__", fork_enter))

    def stream_ctx(orig):
        class region:
            def __init__(self, ctx, hooked):
                self.ctx, self.hooked = ctx, hooked

            def __enter__(self):
                res = self.ctx.__enter__()
                if self.hooked:
                    d.current()
                return res

            def __exit__(self, *exc):
                return self.ctx.__exit__(*exc)

        def stream(st):
            return region(orig(st), st is not None and _from_package())
        return stream
    stack.enter_context(_patched(torch.cuda, "stream", stream_ctx))


def _late_waiter(stack, d):
    def waiter(orig):
        def wait(self, other):
            res = orig(self, other)
            if _from_package():
                d.on(self)
            return res
        return wait
    # (Stream.wait_stream calls self.wait_event from torch's own module: one delay per package-level wait)
    stack.enter_context(_patched(torch.cuda.Stream, "wait_stream", waiter))
    stack.enter_context(_patched(torch.cuda.Stream, "wait_event", waiter))


def _late_owner(stack, d):
    import egaze_amd.hipops as H

    def take(orig):
        def wrapped(self, device):
            capturing = torch.cuda.is_current_stream_capturing()
            tag = (capturing, self.capture_seq if capturing else 0, str(device))
            if self.chunk is None or self.used == self.size or tag != self.tag:        # take() is about to create a chunk
                d.current()
            return orig(self, device)
        return wrapped
    stack.enter_context(_patched(H._AbsmaxArena, "take", take))

    def launch(orig):
        def wrapped(*a):
            d.current()
            return orig(*a)
        return wrapped
    for name in PACK_LAUNCHES:
        getattr(H.LIB, name)                      # (the proxy caches its launcher as an instance attribute on first use)
        stack.enter_context(_patched(H.LIB, name, launch))

    def prepare(orig):
        def wrapped(x, *a, **kw):
            if isinstance(x, torch.Tensor) and x.is_cuda and getattr(x, "_egz_prepared", None) is None:
                d.current()
            return orig(x, *a, **kw)
        return wrapped
    stack.enter_context(_patched(H, "prepare_network_input", prepare))

    def gather(orig):
        def wrapped(*a, **kw):
            d.current()
            return orig(*a, **kw)
        return wrapped
    stack.enter_context(_patched(H, "resident_gather", gather))


_INSTALL = {"late_helper": _late_helper, "late_waiter": _late_waiter, "late_owner": _late_owner}


@contextlib.contextmanager
def perturb(mode: str, delay_ms: float):
    """Install the delays of ``mode`` (see the module docstring) for the duration of the block, with the package's helper streams
    on hardware queues of their own; every hook is removed on exit and the device is drained, so no spin kernel outlives the
    block."""
    if mode not in MODES:
        raise ValueError(f"perturb: mode {mode!r} is none of {MODES}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("perturb() inside a hipGraph capture")
    with contextlib.ExitStack() as stack:
        stack.enter_context(spread_helpers())
        if mode != "none":
            _INSTALL[mode](stack, _Delay(delay_ms))
        try:
            yield
        finally:
            torch.cuda.synchronize()


def poison(h):
    """Fill every hipops workspace and a spread of freed caching-allocator blocks with 0xFF bytes (NaN in fp32 and fp64), so that
    a row / tile a kernel forgets to write reads back as NaN rather than as a lucky zero."""
    torch.cuda.synchronize()
    for ws in h._WS.values():
        ws.fill_(255)
    junk = [torch.empty(256 << 20, dtype=torch.uint8, device=DEV)]
    junk += [torch.empty(n, dtype=torch.uint8, device=DEV) for n in [1 << 20] * 8 + [64 << 10] * 16 + [4096] * 64 + [512] * 64]
    for t in junk:
        t.fill_(255)
    torch.cuda.synchronize()
    del junk
