"""The 1x1 sigmoid head, the losses and the Adam step."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, _out, _p, _req, _stream
from .absmax import _new_absmax
from .conv import MASK_FUSE_STATS

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- head + losses
def conv1x1_sigmoid_fwd(x: torch.Tensor, w: torch.Tensor, bias, want_logits: bool = False):
    _req(x, "x"); _req(w, "weight")
    C = x.shape[-1]
    M = x.numel() // C
    out = torch.empty(tuple(x.shape[:-1]), dtype=torch.float32, device=x.device)
    logits = torch.empty_like(out) if want_logits else None
    check(LIB.egz_conv1x1_sigmoid_fwd(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), _p(logits), M, C,
                                      _stream()), "egz_conv1x1_sigmoid_fwd")
    return out, logits


def conv1x1_sigmoid_bwd(x, w, out, dout, need_dx: bool = True, out_dw=None, out_db=None):
    _req(x, "x"); _req(out, "out"); _req(dout, "dout")
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x) if need_dx else None
    dw = _out(out_dw, (1, C, 1, 1), x.device)
    db = _out(out_db, (1,), x.device)
    ws = _H.workspace(LIB.egz_conv1x1_sigmoid_bwd_ws_bytes(C), x.device)
    check(LIB.egz_conv1x1_sigmoid_bwd(x.data_ptr(), w.data_ptr(), out.data_ptr(), dout.data_ptr(), _p(dx),
                                      dw.data_ptr(), db.data_ptr(), M, C, ws.data_ptr(), ws.numel(), _stream()),
          "egz_conv1x1_sigmoid_bwd")
    return dx, dw, db


def conv1x1_sigmoid_bwd_masked(x, w, out, dout, out_dw=None, out_db=None):
    """Head backward with the ReLU backward of the conv block below folded in (x = that block's post-ReLU output):
    -> (dx masked, dw, db, stat rows (rows, C) fp64 whose column sums are the block's bias gradient, abs-max buffer of dx) --
    the ``_egz_premasked`` hand-over of conv3x3_dgrad_masked (functions.ConvReLU.backward)."""
    _req(x, "x"); _req(out, "out"); _req(dout, "dout")
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    dw = _out(out_dw, (1, C, 1, 1), x.device)
    db = _out(out_db, (1,), x.device)
    ws = _H.workspace(LIB.egz_conv1x1_sigmoid_bwd_ws_bytes(C), x.device)
    stat = torch.empty((int(LIB.egz_conv1x1_sigmoid_bwd_rows(M, C)), C), dtype=torch.float64, device=x.device)
    amo = _new_absmax(x.device)
    check(LIB.egz_conv1x1_sigmoid_bwd_masked(x.data_ptr(), w.data_ptr(), out.data_ptr(), dout.data_ptr(), dx.data_ptr(),
                                             dw.data_ptr(), db.data_ptr(), stat.data_ptr(), amo.data_ptr(), M, C,
                                             ws.data_ptr(), ws.numel(), _stream()), "egz_conv1x1_sigmoid_bwd_masked")
    MASK_FUSE_STATS["produced"] += 1
    return dx, dw, db, stat, amo


def floss_fwd(inp: torch.Tensor, target: torch.Tensor, weighted: bool = True):
    """Returns (loss 0-dim tensor, weights or None).  inp/target: (B,1,H,W) or (B,H,W)."""
    _req(inp, "input"); _req(target, "target")
    B, H, W = inp.shape[0], inp.shape[-2], inp.shape[-1]
    loss = torch.empty((), dtype=torch.float32, device=inp.device)
    weights = torch.empty(inp.numel(), dtype=torch.float32, device=inp.device) if weighted else None
    ws = _H.workspace(LIB.egz_loss_ws_bytes(B), inp.device)
    check(LIB.egz_floss_fwd(inp.data_ptr(), target.data_ptr(), _p(weights), loss.data_ptr(), B, H, W, int(weighted),
                            ws.data_ptr(), ws.numel(), _stream()), "egz_floss_fwd")
    return loss, weights


def floss_bwd(inp, target, weights, grad_out: Optional[torch.Tensor]) -> torch.Tensor:
    dinp = torch.empty_like(inp)
    check(LIB.egz_floss_bwd(inp.data_ptr(), target.data_ptr(), _p(weights), _p(grad_out), dinp.data_ptr(),
                            inp.numel(), _stream()), "egz_floss_bwd")
    return dinp


def mse_fwd(a: torch.Tensor, b: torch.Tensor, tanh_target: bool = False) -> torch.Tensor:
    """mean((a - b)^2), or mean((a - tanh(b))^2) with ``tanh_target`` (AT.py:138 in one pass)."""
    _req(a, "a"); _req(b, "b")
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    ws = _H.workspace(1024 * 8, a.device)
    check(LIB.egz_mse_fwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), a.numel(), ws.data_ptr(), ws.numel(),
                          int(tanh_target), _stream()), "egz_mse_fwd")
    return loss


def mse_fwd_grad(a: torch.Tensor, b: torch.Tensor, tanh_target: bool = False, ring: Optional[torch.Tensor] = None,
                 counter: Optional[torch.Tensor] = None):
    """(loss, d loss / d a) of nn.MSELoss in one launch (n <= 4096; the AT per-sample step).  ``ring`` / ``counter``: the loss is
    also parked in ring[counter[0] % len(ring)] (counter: a device int32 tensor, e.g. FusedAdam.step_dev)."""
    _req(a, "a"); _req(b, "b")
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    da = torch.empty_like(a)
    check(LIB.egz_mse_fwd_grad(a.data_ptr(), b.data_ptr(), loss.data_ptr(), da.data_ptr(), a.numel(), int(tanh_target),
                               _p(ring), 0 if ring is None else ring.numel(), _p(counter), _stream()), "egz_mse_fwd_grad")
    return loss, da


def mse_bwd(a, b, grad_out, tanh_target: bool = False) -> torch.Tensor:
    da = torch.empty_like(a)
    check(LIB.egz_mse_bwd(a.data_ptr(), b.data_ptr(), _p(grad_out), da.data_ptr(), a.numel(), int(tanh_target), _stream()),
          "egz_mse_bwd")
    return da


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, lo: int = 0, hi: Optional[int] = None, nonfinite=None):
    """One Adam step over the flat buffers, or over their slice [lo, hi) (element offsets, multiples of 4).  ``nonfinite``: int32
    device word that gets bit 0 set when the step skipped an element because its gradient was NaN / inf (csrc/adam.hip)."""
    hi = p.numel() if hi is None else hi
    if hi <= lo:
        return
    o = 4 * lo
    check(LIB.egz_adam_step(p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o, hi - lo, lr, beta1, beta2,
                            eps, int(step), grad_scale, _p(nonfinite), _stream()), "egz_adam_step")


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, step_dev, grad_scale=1.0, nonfinite=None):
    """Adam step whose counter of completed steps lives on the device (int32 tensor): usable inside a captured hipGraph."""
    check(LIB.egz_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, beta1, beta2, eps,
                                step_dev.data_ptr(), grad_scale, _p(nonfinite), _stream()), "egz_adam_step_dev")
