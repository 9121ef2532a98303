"""Layout and elementwise passes: stacks, ReLU backward, column sums, NCHW <-> NHWC, input preparation."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, _out, _p, _req, _stream
from .absmax import _new_absmax, _want_absmax, _want_fwd_absmax

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


def stack2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(B, ...) + (B, ...) -> (2B, ...): the depth-2 stack of the fusion block folded into the batch dim, for callers
    whose two maps do not already share one buffer (two stream-ordered device copies, no torch.cat kernel)."""
    _req(a, "a"); _req(b, "b")
    out = torch.empty((2 * a.shape[0],) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
    n = a.numel()
    check(LIB.egz_copy(a.data_ptr(), out.data_ptr(), n, _stream()), "egz_copy")
    check(LIB.egz_copy(b.data_ptr(), out.data_ptr() + 4 * n, n, _stream()), "egz_copy")
    return out


def cat2_planes(f: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """torch.cat((f, g), dim=1) of two (B, 1, H, W) maps in one kernel (models/late_fusion.py:19)."""
    _req(f, "f"); _req(g, "g")
    B, _, Hh, Ww = f.shape
    out = torch.empty((B, 2, Hh, Ww), dtype=torch.float32, device=f.device)
    check(LIB.egz_cat2_planes(f.data_ptr(), g.data_ptr(), out.data_ptr(), B, Hh * Ww, _stream()), "egz_cat2_planes")
    return out


def fill_zero(t: torch.Tensor):
    """hipMemsetAsync on the current stream (zero_grad of the flat gradient buffer)."""
    check(LIB.egz_fill_zero(t.data_ptr(), t.numel() * t.element_size(), _stream()), "egz_fill_zero")


def channel_stats(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    K = x.shape[-1]
    rows = x.numel() // K
    stat = torch.empty((LIB.egz_channel_stats_rows(), 2, K), dtype=torch.float64, device=x.device)
    check(LIB.egz_channel_stats(x.data_ptr(), rows, K, stat.data_ptr(), _stream()), "egz_channel_stats")
    return stat


def relu_bwd(out: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    _req(out, "out"); _req(dout, "dout")
    dy = torch.empty_like(dout)
    check(LIB.egz_relu_bwd(out.data_ptr(), dout.data_ptr(), dy.data_ptr(), out.numel(), _stream()), "egz_relu_bwd")
    return dy


def relu_bwd_bias(out: torch.Tensor, dout: torch.Tensor, out_db: Optional[torch.Tensor] = None):
    """ReLU backward fused with the producing conv's bias gradient: (dy, db)."""
    _req(out, "out"); _req(dout, "dout")
    K = out.shape[-1]
    rows = out.numel() // K
    dy = torch.empty_like(dout)
    db = _out(out_db, (K,), out.device)
    ws = _H.workspace(LIB.egz_relu_bwd_bias_ws_bytes(K), out.device)
    am = _new_absmax(out.device) if _want_absmax() else None
    check(LIB.egz_relu_bwd_bias(out.data_ptr(), dout.data_ptr(), dy.data_ptr(), db.data_ptr(), rows, K,
                                ws.data_ptr(), ws.numel(), _p(am), _stream()), "egz_relu_bwd_bias")
    if am is not None:
        dy._egz_absmax = am
    return dy, db


def upsample2x_bwd(dxu: torch.Tensor) -> torch.Tensor:
    _req(dxu, "dxu")
    B, H2, W2, C = dxu.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, C), dtype=torch.float32, device=dxu.device)
    check(LIB.egz_upsample2x_bwd(dxu.data_ptr(), dx.data_ptr(), B, H2 // 2, W2 // 2, C, _stream()),
          "egz_upsample2x_bwd")
    return dx


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum over all leading dims of an NHWC tensor -> (K,) (conv bias gradient)."""
    _req(x, "x")
    K = x.shape[-1]
    rows = x.numel() // K
    out = _out(out, (K,), x.device)
    ws = _H.workspace(64 * K * 8, x.device)
    check(LIB.egz_colsum(x.data_ptr(), rows, K, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "egz_colsum")
    return out


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    check(LIB.egz_nchw_to_nhwc(x.data_ptr(), out.data_ptr(), B, C, H, W, _stream()), "egz_nchw_to_nhwc")
    return out


def nchw_to_nhwc_pad(x: torch.Tensor, Cp: int) -> torch.Tensor:
    """(B, C, H, W) -> (B, H, W, Cp) with zero channels C .. Cp-1."""
    _req(x, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, Cp), dtype=torch.float32, device=x.device)
    check(LIB.egz_nchw_to_nhwc_pad(x.data_ptr(), out.data_ptr(), B, C, H, W, Cp, _stream()), "egz_nchw_to_nhwc_pad")
    return out


def prepare_network_input(x: torch.Tensor, Cp: int = 32):
    """Input-side work of the NEXT forward pass, issued NOW on the current stream (a copy / helper stream): the re-layout of a
    16 ... 32-channel NCHW network input (the 20-channel flow stack, SP.py:128) into the zero-padded NHWC-32 form its first
    convolution reads, and the abs-max of the result (the scale of its f16 split).  Neither depends on the weights, so a driver
    that has batch k + 1 on the device while step k computes (data.STdatas.staged_batches, bench.py) moves these two HBM passes
    (~0.14 ms at batch 32) out of the serial head of the forward pass and under the MFMA-bound kernels of the step before.  The
    prepared tensor rides on ``x`` and is consumed ONCE by functions.ConvBNReLUPool (the tensor's version and shape are
    checked; anything else falls back to the in-step conversion)."""
    prep = getattr(x, "_egz_prepared", None)
    if prep is not None and prep[1] == x._version and prep[0].shape[3] == Cp:
        return prep[0]                     # the producer of x wrote it already (resident_gather)
    if not (x.is_cuda and x.dim() == 4 and 16 <= x.shape[1] <= Cp and _H.PRECISION == "split" and x.is_contiguous()):
        return None
    xin = _H.nchw_to_nhwc_pad(x.detach(), Cp)
    if _want_fwd_absmax():
        _H.absmax_of(xin)
    ev = torch.cuda.Event()
    ev.record()
    x._egz_prepared = (xin, x._version, ev)
    return xin


def take_prepared_input(x: torch.Tensor, Cp: int = 32):
    """The tensor prepare_network_input left on ``x`` (or None), handed over to the current stream; one-shot."""
    prep = getattr(x, "_egz_prepared", None)
    if prep is None:
        return None
    del x._egz_prepared
    xin, version, ev = prep
    if version != x._version or xin.shape[0] != x.shape[0] or xin.shape[3] != Cp or tuple(xin.shape[1:3]) != tuple(x.shape[2:]):
        return None
    cur = torch.cuda.current_stream()
    cur.wait_event(ev)
    xin.record_stream(cur)
    return xin


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    B, H, W, C = x.shape
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    check(LIB.egz_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), B, C, H, W, _stream()), "egz_nhwc_to_nchw")
    return out
