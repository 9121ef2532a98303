"""TV-L1 optical flow (csrc/flow_tvl1.hip)."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- TV-L1 optical flow (data/extract_flow.py)
# csrc/flow_tvl1.hip; DESIGN.md "TV-L1 optical flow" is the definition, tests/flow_ref.py its numpy restatement.
FLOW_PRESMOOTH_SIGMA = 0.8
FLOW_FUSED = (1, 2, 3, 4, 6, 8)          # inner iterations per solver launch that are built (1: the streaming form)
FLOW_MAX_LEVELS = 16                      # pyramid levels at most, whatever nscales asks for
_FLOW_TAPS = {}
_FLOW_WS = {}


def _flow_taps(device, sigma: float):
    """scipy.ndimage's 1-D Gaussian taps for ``sigma`` (fp64 on the host), as a float32 table on the device -> (taps, R)."""
    key = (torch.device(device).index or 0, float(sigma))
    hit = _FLOW_TAPS.get(key)
    if hit is None:
        import numpy as np
        radius = int(4.0 * sigma + 0.5)
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        hit = (torch.from_numpy((phi / phi.sum()).astype(np.float32)).to(device), radius)
        _FLOW_TAPS[key] = hit
    return hit


def flow_pyramid_sigma(zfactor: float) -> float:
    return 0.6 * (zfactor ** -2 - 1.0) ** 0.5


def flow_level_sizes(H: int, W: int, nscales: int, zfactor: float):
    """[(H, W), ...] of the pyramid, fine to coarse: nscales is clamped so that the coarsest level keeps 16 pixels per side,
    and to FLOW_MAX_LEVELS levels (MAX_LEVELS of the .hip file)."""
    sizes = [(int(H), int(W))]
    while len(sizes) < min(nscales, FLOW_MAX_LEVELS):
        h, w = int(sizes[-1][0] * zfactor + 0.5), int(sizes[-1][1] * zfactor + 0.5)
        if h < 16 or w < 16:
            break
        sizes.append((h, w))
    return sizes


def _flow_dev(t, name, what, dtype, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name}: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if t.dim() not in dims:
        raise ValueError(f"{what}: {name} must have {' or '.join(str(d) for d in dims)} dimensions, got {tuple(t.shape)}")
    return t.contiguous()


def _flow_hw(t, name, what):
    H, W = (int(v) for v in t.shape[-2:])
    if not (16 <= H <= 2048 and 16 <= W <= 2048):
        raise ValueError(f"{what}: {name} of {H} x {W}: height and width must be 16 .. 2048")
    return H, W


def _flow_params(what, **kw):
    for name, v in kw.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
            raise ValueError(f"{what}: {name} must be positive, got {v!r}")


def _flow_k(what, fused):
    if fused is None:
        return 0
    if isinstance(fused, bool) or not isinstance(fused, int) or fused not in FLOW_FUSED:
        raise ValueError(f"{what}: fused must be None (the default, {LIB.egz_tvl1_default_k()}), 1 (one launch per iteration) "
                         f"or 2, 3, 4, 6, 8 iterations per tiled launch, got {fused!r}")
    return fused


def bgr_to_gray_u8(frames: torch.Tensor) -> torch.Tensor:
    """cv2.cvtColor(BGR2GRAY) on 8-bit images (egz_bgr_to_gray_u8): (4899 R + 9617 G + 1868 B + 8192) >> 14, exact.
    frames: uint8 on the GPU, interleaved (N, H, W, 3) or planar (N, 3, H, W) -- the last axis decides when both are 3.
    -> (N, H, W) uint8."""
    what = "bgr_to_gray_u8"
    x = _flow_dev(frames, "frames", what, torch.uint8, (4,))
    if x.shape[3] == 3:
        N, H, W, planar = x.shape[0], x.shape[1], x.shape[2], 0
    elif x.shape[1] == 3:
        N, H, W, planar = x.shape[0], x.shape[2], x.shape[3], 1
    else:
        raise ValueError(f"{what}: frames must be (N, H, W, 3) or (N, 3, H, W), got {tuple(x.shape)}")
    if min(N, H, W) < 1:
        raise ValueError(f"{what}: frames is empty: {tuple(x.shape)}")
    out = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
    check(LIB.egz_bgr_to_gray_u8(x.data_ptr(), N, H, W, planar, out.data_ptr(), _stream()), "egz_bgr_to_gray_u8")
    return out


def flow_to_u8(u: torch.Tensor, bound: float = 20.0) -> torch.Tensor:
    """A flow component as the 8-bit image the temporal stream reads (egz_flow_to_u8): u > bound -> 255, u < -bound -> 0,
    else rint(255 (u + bound) / (2 bound)) in fp64, half to even.  u: float32 on the GPU -> uint8 of the same shape."""
    what = "flow_to_u8"
    if not isinstance(u, torch.Tensor) or not u.is_cuda:
        raise RuntimeError(f"{what}: u: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if u.dtype != torch.float32:
        raise ValueError(f"{what}: u must be float32, got {u.dtype}")
    if u.numel() == 0:
        raise ValueError(f"{what}: u is empty: {tuple(u.shape)}")
    _flow_params(what, bound=bound)
    x = u.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(LIB.egz_flow_to_u8(x.data_ptr(), x.numel(), float(bound), out.data_ptr(), _stream()), "egz_flow_to_u8")
    return out


def tvl1_flow(frames_gray_u8: torch.Tensor, *, tau: float = 0.25, lam: float = 0.15, theta: float = 0.3, nscales: int = 5,
              zfactor: float = 0.5, warps: int = 5, iterations: int = 30, fused: Optional[int] = None):
    """Dual TV-L1 optical flow between consecutive frames of a run (egz_tvl1_flow; DESIGN.md "TV-L1 optical flow").

    frames_gray_u8: (F, H, W) uint8 on the GPU, F >= 2, 16 <= H, W <= 2048.  -> (u1, u2), each (F - 1, H, W) float32:
    frame[i + 1](x + u[i]) ~ frame[i](x), u1 along x, u2 along y.  ``iterations`` inner iterations per warp, a fixed count;
    nscales is clamped so that the coarsest level keeps 16 pixels per side, and to 16 levels.  fused: inner iterations per solver launch --
    None = the measured default, 1 = one streaming launch per iteration, 2 / 3 / 4 / 6 / 8 = overlapped tiles; every choice gives the
    same bits.  The workspace is cached per (device, stream, F, H, W)."""
    what = "tvl1_flow"
    x = _flow_dev(frames_gray_u8, "frames_gray_u8", what, torch.uint8, (3,))
    F = int(x.shape[0])
    if F < 2:
        raise ValueError(f"{what}: frames_gray_u8 holds {F} frame(s): a flow needs at least 2")
    if F > 65536:
        raise ValueError(f"{what}: frames_gray_u8 holds {F} frames: 65536 per call at most")
    H, W = _flow_hw(x, "frames_gray_u8", what)
    _flow_params(what, tau=tau, lam=lam, theta=theta, nscales=nscales, zfactor=zfactor, warps=warps, iterations=iterations)
    for name, v in (("nscales", nscales), ("warps", warps), ("iterations", iterations)):
        if not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if not zfactor < 1:
        raise ValueError(f"{what}: zfactor must lie in (0, 1), got {zfactor!r}")
    k = _flow_k(what, fused)
    dev = x.device
    g0, r0 = _flow_taps(dev, FLOW_PRESMOOTH_SIGMA)
    g1, r1 = _flow_taps(dev, _H.flow_pyramid_sigma(float(zfactor)))
    if r1 > 16:
        raise ValueError(f"{what}: zfactor {zfactor!r} needs a pyramid filter of radius {r1}: 16 taps per side at most")
    nb = LIB.egz_tvl1_flow_ws_bytes(F, H, W, nscales, float(zfactor))
    key = (dev.index or 0, _stream(), F, H, W)
    ws = _FLOW_WS.get(key)
    if ws is None or ws.numel() < nb:
        _FLOW_WS.pop(key, None)
        while len(_FLOW_WS) >= 4:                                   # a folder's chunks have two sizes: keep a few, not all
            _FLOW_WS.pop(next(iter(_FLOW_WS)))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        _FLOW_WS[key] = ws
    u1 = torch.empty((F - 1, H, W), dtype=torch.float32, device=dev)
    u2 = torch.empty_like(u1)
    check(LIB.egz_tvl1_flow(x.data_ptr(), F, H, W, g0.data_ptr(), r0, g1.data_ptr(), r1, float(tau), float(lam), float(theta),
                            nscales, float(zfactor), warps, iterations, k, ws.data_ptr(), ws.numel(), u1.data_ptr(),
                            u2.data_ptr(), _stream()), "egz_tvl1_flow")
    return u1, u2


# The stages of tvl1_flow one by one (tests, tools/bench_flow.py); planes are (P, H, W).
def flow_gauss(src: torch.Tensor, sigma: float) -> torch.Tensor:
    """Separable Gaussian with a replicated border of uint8 or float32 planes (P, H, W) -> float32."""
    what = "flow_gauss"
    if isinstance(src, torch.Tensor) and src.dtype == torch.uint8:
        x = _flow_dev(src, "src", what, torch.uint8, (3,))
    else:
        x = _flow_dev(src, "src", what, torch.float32, (3,))
    H, W = _flow_hw(x, "src", what)
    _flow_params(what, sigma=sigma)
    gw, R = _flow_taps(x.device, float(sigma))
    tmp = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dst = torch.empty_like(tmp)
    check(LIB.egz_flow_gauss(x.data_ptr(), int(x.dtype == torch.uint8), x.shape[0], H, W, gw.data_ptr(), R, tmp.data_ptr(),
                             dst.data_ptr(), _stream()), "egz_flow_gauss")
    return dst


def flow_resample(src: torch.Tensor, out_hw, scale: float = 1.0) -> torch.Tensor:
    """Keys' bicubic resampling (a = -0.5) of float32 planes (P, h, w) to out_hw, times ``scale``."""
    what = "flow_resample"
    x = _flow_dev(src, "src", what, torch.float32, (3,))
    hs, ws = _flow_hw(x, "src", what)
    hd, wd = (int(v) for v in out_hw)
    if not (16 <= hd <= 2048 and 16 <= wd <= 2048):
        raise ValueError(f"{what}: out_hw {(hd, wd)}: height and width must be 16 .. 2048")
    dst = torch.empty((x.shape[0], hd, wd), dtype=torch.float32, device=x.device)
    check(LIB.egz_flow_resample(x.data_ptr(), x.shape[0], hs, ws, dst.data_ptr(), hd, wd, float(scale), _stream()),
          "egz_flow_resample")
    return dst


def flow_grad(img: torch.Tensor):
    """Central differences with a replicated border of float32 planes (P, H, W) -> (d/dx, d/dy)."""
    what = "flow_grad"
    x = _flow_dev(img, "img", what, torch.float32, (3,))
    H, W = _flow_hw(x, "img", what)
    gx, gy = torch.empty_like(x), torch.empty_like(x)
    check(LIB.egz_flow_grad(x.data_ptr(), x.shape[0], H, W, gx.data_ptr(), gy.data_ptr(), _stream()), "egz_flow_grad")
    return gx, gy


def tvl1_warp(img: torch.Tensor, i1x: torch.Tensor, i1y: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """img: (N + 1, H, W) frames of one level; i1x, i1y: (N, H, W) gradient of frames 1 .. N; u: (2, N, H, W) flow
    -> (4, N, H, W): gx, gy, gx^2 + gy^2 and the constant part of the residual, I1 and its gradient sampled at x + u."""
    what = "tvl1_warp"
    x = _flow_dev(img, "img", what, torch.float32, (3,))
    H, W = _flow_hw(x, "img", what)
    N = int(x.shape[0]) - 1
    gx = _flow_dev(i1x, "i1x", what, torch.float32, (3,))
    gy = _flow_dev(i1y, "i1y", what, torch.float32, (3,))
    uu = _flow_dev(u, "u", what, torch.float32, (4,))
    if N < 1 or tuple(gx.shape) != (N, H, W) or tuple(gy.shape) != (N, H, W) or tuple(uu.shape) != (2, N, H, W):
        raise ValueError(f"{what}: img {tuple(x.shape)} needs i1x, i1y of {(N, H, W)} and u of {(2, N, H, W)}, got "
                         f"{tuple(gx.shape)}, {tuple(gy.shape)}, {tuple(uu.shape)}")
    consts = torch.empty((4, N, H, W), dtype=torch.float32, device=x.device)
    check(LIB.egz_tvl1_warp(x.data_ptr(), gx.data_ptr(), gy.data_ptr(), uu.data_ptr(), consts.data_ptr(), N, H, W, _stream()),
          "egz_tvl1_warp")
    return consts


def tvl1_iterate(state: torch.Tensor, consts: torch.Tensor, iterations: int, *, tau: float = 0.25, lam: float = 0.15,
                 theta: float = 0.3, fused: Optional[int] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``iterations`` inner iterations of the solver (egz_tvl1_iterate).  state: (6, N, H, W) float32 = u1 u2 p11 p12 p21 p22
    (left unchanged); consts: (4, N, H, W) from tvl1_warp.  -> the new state.  scratch: a (6, N, H, W) buffer to ping-pong
    with (overwritten; the result may be it)."""
    what = "tvl1_iterate"
    s = _flow_dev(state, "state", what, torch.float32, (4,))
    c = _flow_dev(consts, "consts", what, torch.float32, (4,))
    H, W = _flow_hw(s, "state", what)
    N = int(s.shape[1])
    if s.shape[0] != 6 or N < 1 or tuple(c.shape) != (4, N, H, W):
        raise ValueError(f"{what}: state must be (6, N, H, W) and consts (4, N, H, W), got {tuple(s.shape)} and "
                         f"{tuple(c.shape)}")
    _flow_params(what, iterations=iterations, tau=tau, lam=lam, theta=theta)
    if not isinstance(iterations, int):
        raise ValueError(f"{what}: iterations must be an integer, got {iterations!r}")
    k = _flow_k(what, fused)
    a = s.clone()
    if scratch is None:
        b = torch.empty_like(a)
    else:
        b = _flow_dev(scratch, "scratch", what, torch.float32, (4,))
        if tuple(b.shape) != tuple(a.shape) or b.data_ptr() != scratch.data_ptr():
            raise ValueError(f"{what}: scratch must be a contiguous {tuple(a.shape)} buffer, got {tuple(scratch.shape)}")
    check(LIB.egz_tvl1_iterate(a.data_ptr(), b.data_ptr(), c.data_ptr(), N, H, W, iterations, k, float(tau), float(lam),
                               float(theta), _stream()), "egz_tvl1_iterate")
    launches = -(-iterations // (k or LIB.egz_tvl1_default_k()))
    return a if launches % 2 == 0 else b
