"""BatchNorm (train, deferred, eval fold) with ReLU and pool, and the fusion block's pair-max."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, _out, _p, _req, _stream
from .packing import _tag
from .absmax import _new_absmax, _want_absmax, _want_fwd_absmax
from .conv import BNSUMS_STATS, PRESPLIT_STATS

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- BN / ReLU / pool
def bn_finalize(stat: torch.Tensor, count: float, gamma, beta, running_mean, running_var, momentum: float,
                eps: float, num_batches_tracked: Optional[torch.Tensor] = None, mm: Optional[torch.Tensor] = None):
    """``num_batches_tracked``: the BatchNorm's int64 counter on the device, incremented by the same launch.
    ``mm``: the per-channel max / min buffer of the conv output (conv3x3_fwd(want_bound=True)) -> returns (coef, abs-max buffer
    holding the EXACT max of relu(y * scale + shift)) instead of coef alone."""
    rows, _, K = stat.shape
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        raise RuntimeError("num_batches_tracked: expected an int64 HIP tensor")
    dev = stat.device
    coef = torch.empty((4, K), dtype=torch.float32, device=dev)      # mean, invstd, scale, shift
    ws = _H.workspace(LIB.egz_bn_ws_bytes(K), dev)
    if running_mean is not None:        # written behind torch's back: invalidate what is cached on it (bn_eval_coeffs)
        _H.touch_params((running_mean,))
    args = (stat.data_ptr(), rows, K, float(count), _p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum, eps,
            coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), _p(num_batches_tracked),
            ws.data_ptr(), ws.numel())
    if mm is not None:
        am = _new_absmax(dev)
        check(LIB.egz_bn_finalize_bound(*args, mm.data_ptr(), am.data_ptr(), _stream()), "egz_bn_finalize_bound")
        return coef, am
    check(LIB.egz_bn_finalize(*args, _stream()), "egz_bn_finalize")
    return coef


# Deferred BatchNorm (late-fusion stack, training): the [BN -> ReLU] of a narrow block is applied by the NEXT block's conv and
# weight-gradient kernels while they stage its pre-BN output, so the normalised tensor (205 MB at B = 32, 224 x 224 x 32) is
# neither written nor read.  BN_DEFER = False materialises it as before (test_deferred_batchnorm_matches_materialised compares the two).
BN_DEFER_STATS = {"deferred": 0}


def bn_defer_ok(B: int, H: int, W: int, K: int, K_next: int, first_direct: bool) -> bool:
    """Can the [BN -> ReLU] of a block with K output channels at (B, H, W) be left to a next 3x3 conv with K_next filters?
    Needs the split-half policy, the persistent narrow conv kernel and the narrow weight-gradient kernel for K -> K_next, and
    a producer that emits per-channel max / min rows (the narrow conv kernel itself, or the direct first-layer kernel)."""
    if not (_H.BN_DEFER and _H.BNSUMS_FUSE and _H.PRECISION == "split" and _H.GRAD_SPLIT == "f16" and _H.FWD_SCALE):
        return False
    if not (K in (16, 32) and K_next <= 32 and K_next % 4 == 0 and H % 16 == 0 and W % 16 == 0):
        return False
    if 4 * B * H * W * max(K, K_next) >= 2 ** 32:
        return False
    return bool(LIB.egz_conv3x3_streamed_ok(B, H, W, K, K_next, 0) and LIB.egz_conv3x3_streamed_ok(B, H, W, K_next, K, 0)
                and LIB.egz_conv3x3_wgrad_narrow_ok(B, H, W, K, K_next))


def bn_finalize_deferred(stat: torch.Tensor, minmax: torch.Tensor, count: float, gamma, beta, running_mean, running_var,
                         momentum: float, eps: float, num_batches_tracked: Optional[torch.Tensor] = None):
    """bn_finalize for a BatchNorm whose output is never materialised -> (coef (4, K), abs-max buffer holding the exact max of
    relu(y * scale + shift), derived from y's per-channel max / min rows)."""
    rows, _, K = stat.shape
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        raise RuntimeError("num_batches_tracked: expected an int64 HIP tensor")
    dev = stat.device
    coef = torch.empty((4, K), dtype=torch.float32, device=dev)
    am = _new_absmax(dev)
    if running_mean is not None:
        _H.touch_params((running_mean,))
    check(LIB.egz_bn_finalize_deferred(stat.data_ptr(), rows, K, float(count), _p(gamma), _p(beta), _p(running_mean),
                                       _p(running_var), momentum, eps, coef[0].data_ptr(), coef[1].data_ptr(),
                                       coef[2].data_ptr(), coef[3].data_ptr(), _p(num_batches_tracked), minmax.data_ptr(),
                                       minmax.shape[0], am.data_ptr(), _stream()), "egz_bn_finalize_deferred")
    BN_DEFER_STATS["deferred"] += 1
    return coef, am


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps: float):
    """Eval-mode (scale, shift) rows of a BatchNorm.  Pass the module's own parameter / buffer objects: the result is cached
    on ``running_mean`` and reused until any of the four tensors changed (torch version counters for in-place torch
    writes such as load_state_dict or a broadcast, the per-tensor epoch for writes behind torch's back: bn_finalize's
    running-statistics update, the fused optimizer's step) -- at batch 1 the two launches per layer were a quarter of the
    device time of a captured forward."""
    key = (_tag(running_mean), _tag(running_var), None if gamma is None else _tag(gamma), None if beta is None else _tag(beta),
           float(eps), _stream_device(running_mean))
    hit = getattr(running_mean, "_egz_evalcoef", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    K = running_mean.numel()
    coef = torch.zeros((4, K), dtype=torch.float32, device=running_mean.device)
    g = None if gamma is None else gamma.detach()
    b = None if beta is None else beta.detach()
    check(LIB.egz_bn_eval_coeffs(K, _p(g), _p(b), running_mean.data_ptr(), running_var.data_ptr(), eps,
                                 coef[2].data_ptr(), coef[3].data_ptr(), _stream()), "egz_bn_eval_coeffs")
    # the cached rows are read by later launches on whatever stream is current then: make them safe to read from any
    # stream by finishing the two small launches first (once per weight change, not per forward)
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream().synchronize()
        running_mean._egz_evalcoef = (key, coef)
    return coef


def _stream_device(t):
    return t.device.index or 0


# Inference: a [Conv2d 3x3 -> BatchNorm2d (eval) -> ReLU] block without a pool runs as ONE launch -- the BatchNorm's eval-mode
# affine map is folded into the convolution (w' = w * scale[k], b' = b * scale[k] + shift[k], the bias + ReLU epilogue), so the
# normalise pass (one read + one write of the layer's output, 8 of the 13 blocks of a VGG16-BN encoder) disappears.  The folded
# tensors are cached on the weight and rebuilt when the weight, the bias or the BatchNorm's coefficients change.  Rounding: the
# product w * scale is rounded once per weight (relative 6e-8) -- eval outputs move by ~1e-7 relative.
# (hipops.EVAL_FOLD; test_eval_batchnorm_folded_into_conv compares the two.  hipops.INFER_CALL is set by utils.conv_bn_relu_pool
# right before ConvBNReLUPool.apply: the block runs under torch.no_grad().)
EVAL_FOLD_STATS = {"folded": 0}


def bn_fold_key(weight, bias, gamma, beta, running_mean, running_var, eps: float):
    return (_tag(weight), None if bias is None else _tag(bias), _tag(running_mean), _tag(running_var),
            None if gamma is None else _tag(gamma), None if beta is None else _tag(beta), float(eps))


def bn_fold_is_warm(weight, bias, gamma, beta, running_mean, running_var, eps: float) -> bool:
    """True when the folded tensors cached on ``weight`` match the current parameters / statistics (so that
    bn_folded_conv launches nothing): what a hipGraph capture needs -- a cold OR stale cache takes the unfolded path."""
    hit = getattr(weight, "_egz_fold", None)
    return hit is not None and hit[0] == _H.bn_fold_key(weight, bias, gamma, beta, running_mean, running_var, eps)


def bn_folded_conv(weight, bias, gamma, beta, running_mean, running_var, eps: float):
    """-> (w', b') of the folded block, cached on ``weight`` (pass the module's own parameter / buffer objects).  Not to be
    called inside a hipGraph capture before the cache is warm (the fold itself is a few stock elementwise kernels, once per
    weight change)."""
    coef = _H.bn_eval_coeffs(gamma, beta, running_mean, running_var, eps)
    key = _H.bn_fold_key(weight, bias, gamma, beta, running_mean, running_var, eps)
    hit = getattr(weight, "_egz_fold", None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("bn_folded_conv: cold or stale cache inside a hipGraph capture (callers check bn_fold_is_warm)")
    with torch.no_grad():
        K = weight.shape[0]
        wf = hit[1] if hit is not None else torch.empty_like(weight.detach())
        bf = hit[2] if hit is not None else torch.empty((K,), dtype=torch.float32, device=weight.device)
        torch.mul(weight.detach(), coef[2].view(K, 1, 1, 1), out=wf)
        if bias is not None:
            torch.addcmul(coef[3], bias.detach(), coef[2], out=bf)
        else:
            bf.copy_(coef[3])
    _H.touch_params([wf])                       # its packings are stale
    torch.cuda.current_stream().synchronize()
    weight._egz_fold = (key, wf, bf)
    return wf, bf


def bn_relu_pool_fwd(y: torch.Tensor, coef: torch.Tensor, pool: bool, out: Optional[torch.Tensor] = None,
                     presplit_am: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``presplit_am``: the exact abs-max of the output (bn_finalize(..., mm=...)): the output is then stored PRE-SPLIT (f16
    hi / lo pairs in the fp32 footprint, see PRESPLIT) and tagged ``_egz_presplit``; only conv3x3_fwd(pre_in=True) and
    conv3x3_wgrad(x_pre=True) can read it."""
    _req(y, "y")
    B, H, W, K = y.shape
    out = _out(out, (B, H // 2, W // 2, K) if pool else (B, H, W, K), y.device)
    args = (y.data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), out.data_ptr(), B, H, W, K, int(pool))
    if presplit_am is not None:
        check(LIB.egz_bn_relu_pool_fwd_presplit(*args, presplit_am.data_ptr(), _stream()), "egz_bn_relu_pool_fwd_presplit")
        out._egz_absmax = presplit_am
        out._egz_presplit = True
        PRESPLIT_STATS["produced"] += 1
        return out
    am = _new_absmax(y.device) if _want_fwd_absmax() else None
    check(LIB.egz_bn_relu_pool_fwd(*args, _p(am), _stream()), "egz_bn_relu_pool_fwd")
    if am is not None:
        out._egz_absmax = am      # max |out|, folded into the same pass: scales the f16 split of the consuming convolution
    return out


def bn_relu_pool_bwd(y: torch.Tensor, dout: torch.Tensor, coef: torch.Tensor, pool: bool,
                     out_dgamma: Optional[torch.Tensor] = None, out_dbeta: Optional[torch.Tensor] = None,
                     sums: Optional[torch.Tensor] = None, presplit=None):
    """Returns (dy, dgamma, dbeta); ``out_dgamma`` / ``out_dbeta``: K-float destinations (gradient sinks).
    ``sums``: (rows, 2, K) fp64 partial rows from conv3x3_dgrad_bnsums (the producer of ``dout``): no reduce pass.
    ``presplit`` = (abs-max buffer of dout, max / min buffer of y): dy is stored as pre-split pairs scaled by a bound of its
    maximum (see PRESPLIT_GRAD), tagged ``_egz_presplit`` and carrying that bound as ``_egz_absmax``."""
    _req(y, "y"); _req(dout, "dout")
    B, H, W, K = y.shape
    dy = torch.empty_like(y)
    dg, db = _out(out_dgamma, (K,), y.device), _out(out_dbeta, (K,), y.device)
    ws = _H.workspace(LIB.egz_bn_relu_pool_bwd_ws_bytes(K), y.device)
    am = _new_absmax(y.device) if presplit is not None or _want_absmax() else None
    args = (y.data_ptr(), dout.data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(),
            dy.data_ptr(), dg.data_ptr(), db.data_ptr(), B, H, W, K, int(pool), ws.data_ptr(), ws.numel(), _p(am), _p(sums),
            0 if sums is None else sums.shape[0])
    if presplit is not None:
        dout_am, y_mm = presplit
        check(LIB.egz_bn_relu_pool_bwd_presplit(*args, y_mm.data_ptr(), dout_am.data_ptr(), _stream()),
              "egz_bn_relu_pool_bwd_presplit")
        dy._egz_presplit = True
        PRESPLIT_STATS["grad_produced"] += 1
    else:
        check(LIB.egz_bn_relu_pool_bwd(*args, _stream()), "egz_bn_relu_pool_bwd")
    if sums is not None:
        BNSUMS_STATS["consumed"] += 1
    if am is not None:
        dy._egz_absmax = am      # max |dy|, folded into the same pass: scales the f16 split of the conv backward
    return dy, dg, db


def bn_bwd_first_wgrad_ok(C: int, K: int, pool: bool) -> bool:
    """First block of a narrow stack: BatchNorm backward + weight gradient in one pass."""
    return bool(K in (32, 64) and 1 <= C <= 3 and not pool)


def bn_bwd_first_wgrad(y: torch.Tensor, dout: torch.Tensor, coef: torch.Tensor, x_nchw: torch.Tensor,
                       out_dgamma: Optional[torch.Tensor] = None, out_dbeta: Optional[torch.Tensor] = None,
                       out_dw: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None):
    """Backward of a first [Conv2d(C <= 3 -> 32 | 64) -> BN(train) -> ReLU] block (the late-fusion stack; the RGB encoder) in one
    pass over (y, dout): returns (dw (K, C, 3, 3), dgamma, dbeta); the gradient w.r.t. the conv output is never materialised."""
    _req(y, "y"); _req(dout, "dout"); _req(x_nchw, "x")
    B, H, W, K = y.shape
    C = x_nchw.shape[1]
    if tuple(x_nchw.shape) != (B, C, H, W) or tuple(dout.shape) != tuple(y.shape):
        raise RuntimeError(f"x {tuple(x_nchw.shape)} / dout {tuple(dout.shape)} do not match y {tuple(y.shape)}")
    dg, db = _out(out_dgamma, (K,), y.device), _out(out_dbeta, (K,), y.device)
    dw = _out(out_dw, (K, C, 3, 3), y.device)
    nb = LIB.egz_bn_bwd_first_wgrad_ws_bytes(C, K)
    ws = _H.workspace(nb, y.device)
    check(LIB.egz_bn_bwd_first_wgrad(y.data_ptr(), dout.data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), coef[0].data_ptr(),
                                     coef[1].data_ptr(), x_nchw.data_ptr(), dw.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                     B, H, W, C, K, ws.data_ptr(), ws.numel(), _p(sums), 0 if sums is None else sums.shape[0],
                                     _stream()), "egz_bn_bwd_first_wgrad")
    if sums is not None:
        BNSUMS_STATS["consumed"] += 1
    return dw, dg, db


def pairmax_fwd(y2: torch.Tensor) -> torch.Tensor:
    """y2: (2B, H, W, K) = stream s rows then stream t rows -> (B, H, W, K) element-wise max (s wins ties)."""
    _req(y2, "y2")
    B2 = y2.shape[0]
    z = torch.empty((B2 // 2,) + tuple(y2.shape[1:]), dtype=torch.float32, device=y2.device)
    check(LIB.egz_pairmax_fwd(y2.data_ptr(), z.data_ptr(), z.numel(), _stream()), "egz_pairmax_fwd")
    return z


def pairmax_bwd(y2: torch.Tensor, dz: torch.Tensor) -> torch.Tensor:
    _req(y2, "y2"); _req(dz, "dz")
    dy2 = torch.empty_like(y2)
    am = _new_absmax(y2.device) if _want_absmax() else None
    check(LIB.egz_pairmax_bwd(y2.data_ptr(), dz.data_ptr(), dy2.data_ptr(), dz.numel(), _p(am), _stream()),
          "egz_pairmax_bwd")
    if am is not None:
        dy2._egz_absmax = am
    return dy2
