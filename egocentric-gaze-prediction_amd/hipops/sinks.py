"""Gradient sinks: backward kernels write a fused optimizer's flat gradient buffer directly."""
from __future__ import annotations

import sys
from typing import Optional

import torch

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- gradient sinks
class GradSink:
    """Where a parameter's gradient lands when the parameter lives in a fused optimizer's flat buffers (optim.FusedAdam):
    the backward kernels write ``p.grad`` (a view of the flat gradient buffer) DIRECTLY and the autograd node returns
    ``None`` for that input, so no stock ``AccumulateGrad`` add (one launch + 3 HBM passes per parameter, reference
    SP.py:136-138) runs in the step.  torch's accumulation semantics are kept: only the FIRST gradient of a
    ``zero_grad()`` generation is written in place; a second backward without ``zero_grad`` (or a weight used twice in one
    graph) finds the sink taken and goes through autograd's ordinary accumulation.  ``hooks`` fire after the in-place
    write (dp.GradReducer counts its buckets down there, as its post-accumulate-grad hook does on the autograd route)."""
    __slots__ = ("buf", "owner", "gen_written", "hooks")

    def __init__(self, buf, owner):
        self.buf, self.owner, self.gen_written, self.hooks = buf, owner, -1, []


def grad_sink(param, wanted: bool = True) -> Optional[torch.Tensor]:
    """The in-place gradient destination of ``param`` for this backward pass, or None (-> return the gradient to autograd).
    Taking the sink marks it used for the current zero_grad generation."""
    if not wanted:
        return None
    sk = getattr(param, "_egz_sink", None)
    if sk is None or not _H.DIRECT_GRADS:
        return None
    gen = sk.owner.zero_gen
    if sk.gen_written == gen:
        return None
    sk.gen_written = gen
    return sk.buf


# hipops.DIRECT_GRADS = False: every gradient goes back through autograd's AccumulateGrad (AT._GraphedSampleStep honours it).
PENDING_PRODUCER = [None]       # helper stream a detached weight-gradient fork just left running (functions._close_fork)


def grad_done(param):
    """Run the sink hooks of ``param``: its gradient is final on the current stream -- or on the helper stream a detached
    weight-gradient fork left running (the hooks get that stream as their second argument)."""
    st, PENDING_PRODUCER[0] = PENDING_PRODUCER[0], None
    sk = getattr(param, "_egz_sink", None)
    if sk is not None:
        for h in sk.hooks:
            h(param, st)
