"""Feature visualisation: INTER_LINEAR resize, JET heatmap overlays."""
from __future__ import annotations

import sys

import torch

from .._lib import check
from ._core import LIB, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- feature visualisation (vis_features.py)
def linear_table(ssize: int, dsize: int, axis: str = "x"):
    """OpenCV's INTER_LINEAR table for one axis of an 8-bit resize (resizeGeneric_ in imgproc/resize.cpp, restated here: cv2
    is not a dependency of this package), in OpenCV's own float arithmetic.  -> (ofs int32 [dsize], alpha int16 [2 dsize]):
    per output index d, f = (float)((d + 0.5) * scale - 0.5) with scale = 1.0 / ((double)dsize / ssize), s = floor(f),
    f -= s, alpha = (cvRound((1.f - f) * 2048), cvRound(f * 2048)).  axis 'x' turns s < 0 into (s = 0, f = 0) and
    s >= ssize - 1 into (s = ssize - 1, f = 0); axis 'y' leaves s and f as computed (the kernel clamps the two source rows)."""
    import numpy as np
    ssize, dsize = int(ssize), int(dsize)
    if ssize <= 0 or dsize <= 0:
        raise ValueError(f"linear_table: sizes must be positive (got {ssize} -> {dsize})")
    if axis not in ("x", "y"):
        raise ValueError(f"linear_table: axis must be 'x' or 'y', got {axis!r}")
    scale = 1.0 / (dsize / ssize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    if axis == "x":
        lo, hi = s < 0, s >= ssize - 1
        s = np.where(lo, 0, np.where(hi, ssize - 1, s))
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048))
    a1 = np.rint(f * np.float32(2048))
    return s.astype(np.int32), np.stack((a0, a1), 1).reshape(-1).astype(np.int16)


_LINEAR_T = {}


def _linear_tables(device, src_hw, out_hw, what):
    (sh, sw), (dh, dw) = (tuple(int(v) for v in src_hw), tuple(int(v) for v in out_hw))
    if sh == 2 * dh and sw == 2 * dw:
        raise ValueError(f"{what}: {(sh, sw)} -> {(dh, dw)} is an exact 2x decimation, which cv2.resize hands from "
                         f"INTER_LINEAR to its INTER_AREA code; that path is not provided here")
    key = (torch.device(device).index or 0, (sh, sw), (dh, dw))
    hit = _LINEAR_T.get(key)
    if hit is None:
        hit = tuple(torch.from_numpy(a).to(device) for a in _H.linear_table(sw, dw, "x") + _H.linear_table(sh, dh, "y"))
        _LINEAR_T[key] = hit
    return hit          # (x ofs, x alpha, y ofs, y alpha)


def _u8_dev(t, name, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: {name} must be uint8, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a HIP ('cuda') tensor -- this package has no CPU path")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous, got strides {t.stride()} for {tuple(t.shape)}")
    return t


def resize_linear_u8(src: torch.Tensor, out_hw, layout: str = "chw") -> torch.Tensor:
    """cv2.resize(img, (W', H')) with INTER_LINEAR on 8-bit images, bit for bit (egz_resize_linear_u8), N images per launch.

    src: uint8, contiguous, on the GPU.  layout 'chw' (planar): (H, W), (N, H, W) or (N, C, H, W); layout 'hwc' (interleaved,
    cv2's own): (H, W, C) or (N, H, W, C); C = 1 or 3.  out_hw = (H', W').  -> the same layout at H' x W'.  An exact 2x
    decimation on both axes, which cv2.resize hands to its INTER_AREA code, raises ValueError (area_table / gaze_gt_maps
    restate INTER_AREA)."""
    what = "resize_linear_u8"
    _u8_dev(src, "src", what)
    if layout not in ("chw", "hwc"):
        raise ValueError(f"{what}: layout must be 'chw' or 'hwc', got {layout!r}")
    dh, dw = (int(v) for v in out_hw)
    if dh <= 0 or dw <= 0:
        raise ValueError(f"{what}: out_hw {(dh, dw)} must be positive")
    shape = tuple(src.shape)
    if layout == "chw" and src.dim() in (2, 3, 4):
        N, C, sh, sw = ((1, 1) if src.dim() == 2 else (shape[0], 1) if src.dim() == 3 else shape[:2]) + shape[-2:]
        oshape = shape[:-2] + (dh, dw)
    elif layout == "hwc" and src.dim() in (3, 4):
        N, sh, sw, C = (1,) * (4 - src.dim()) + shape
        oshape = shape[:-3] + (dh, dw, C)
    else:
        raise ValueError(f"{what}: a {src.dim()}-D source {shape} does not fit layout {layout!r}")
    if C not in (1, 3):
        raise ValueError(f"{what}: {C} channels in {shape} (layout {layout!r}); 1 or 3 are supported")
    if min(N, sh, sw) <= 0:
        raise ValueError(f"{what}: empty source {shape}")
    xo, xa, yo, ya = _linear_tables(src.device, (sh, sw), (dh, dw), what)
    dst = torch.empty(oshape, dtype=torch.uint8, device=src.device)
    check(LIB.egz_resize_linear_u8(src.data_ptr(), N, C, sh, sw, dh, dw, int(layout == "hwc"), xo.data_ptr(), xa.data_ptr(),
                                   yo.data_ptr(), ya.data_ptr(), dst.data_ptr(), _stream()), "egz_resize_linear_u8")
    return dst


def heatmap_overlay(maps: torch.Tensor, frames: torch.Tensor, frame_index, lut: torch.Tensor) -> torch.Tensor:
    """vis_features' resize -> applyColorMap -> heatmap * 0.3 + img * 0.5 -> imwrite chain for M overlays in one launch
    (egz_heatmap_overlay).

    maps: (M, h, w) uint8; frames: (F, 3, H, W) uint8 BGR planes (the raw_u8 loader's 'image'); frame_index: M frame numbers in
    [0, F) (a list or an integer tensor); lut: (256, 3) uint8 BGR colormap (jet_lut).  All on one GPU.  -> (M, H, W, 3) uint8
    BGR, what cv2.imwrite would receive: the map resized with INTER_LINEAR (resize_linear_u8's arithmetic), looked up, and
    blended as rint(fl64(h * 0.3) + fl64(i * 0.5)) (numpy float64, then convertTo(CV_8U): half to even, saturated)."""
    what = "heatmap_overlay"
    _u8_dev(maps, "maps", what)
    _u8_dev(frames, "frames", what)
    _u8_dev(lut, "lut", what)
    if maps.dim() != 3 or min(maps.shape) == 0:
        raise ValueError(f"{what}: maps must be a non-empty (M, h, w), got {tuple(maps.shape)}")
    if frames.dim() != 4 or frames.shape[1] != 3 or min(frames.shape) == 0:
        raise ValueError(f"{what}: frames must be a non-empty (F, 3, H, W), got {tuple(frames.shape)}")
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"{what}: lut must be (256, 3), got {tuple(lut.shape)}")
    if len({maps.device, frames.device, lut.device}) != 1:
        raise ValueError(f"{what}: maps, frames and lut must be on one device")
    M, h, w = maps.shape
    F, _, Hh, Ww = frames.shape
    if isinstance(frame_index, torch.Tensor):
        if frame_index.dtype.is_floating_point or frame_index.dtype.is_complex or frame_index.dtype == torch.bool:
            raise ValueError(f"{what}: frame_index must hold integers, got {frame_index.dtype}")
        fi_host = frame_index.detach().cpu().reshape(-1).to(torch.int64)
    else:
        fi_host = torch.as_tensor(list(frame_index), dtype=torch.int64).reshape(-1)
    if fi_host.numel() != M:
        raise ValueError(f"{what}: {M} maps but {fi_host.numel()} frame indices")
    if bool(((fi_host < 0) | (fi_host >= F)).any()):
        raise ValueError(f"{what}: frame indices must lie in [0, {F})")
    xo, xa, yo, ya = _linear_tables(maps.device, (h, w), (Hh, Ww), what)
    fi = fi_host.to(torch.int32).to(maps.device, non_blocking=True)
    out = torch.empty((M, Hh, Ww, 3), dtype=torch.uint8, device=maps.device)
    check(LIB.egz_heatmap_overlay(maps.data_ptr(), M, h, w, fi.data_ptr(), frames.data_ptr(), F, Hh, Ww, lut.data_ptr(),
                                  xo.data_ptr(), xa.data_ptr(), yo.data_ptr(), ya.data_ptr(), out.data_ptr(), _stream()),
          "egz_heatmap_overlay")
    return out


def cell_argmax_u8(gt: torch.Tensor, cell: int = 16) -> torch.Tensor:
    """argmax(AvgPool2d(cell)(gt)) of the reference's vis_features, from exact integer cell sums (egz_cell_argmax_u8).

    gt: (N, H, W) or (N, 1, H, W) uint8 on the GPU.  -> (N,) int32 on the GPU: the row-major index of the first maximal cell of
    the (H // cell) x (W // cell) grid (numpy's tie rule; trailing rows / columns are dropped as AvgPool2d drops them)."""
    what = "cell_argmax_u8"
    _u8_dev(gt, "gt", what)
    if gt.dim() == 4 and gt.shape[1] == 1:
        gt = gt.view(gt.shape[0], gt.shape[2], gt.shape[3])
    if gt.dim() != 3 or gt.shape[0] == 0:
        raise ValueError(f"{what}: gt must be (N, H, W) or (N, 1, H, W), got {tuple(gt.shape)}")
    cell = int(cell)
    N, Hh, Ww = gt.shape
    if cell <= 0 or Hh < cell or Ww < cell:
        raise ValueError(f"{what}: cell {cell} does not fit a {Hh} x {Ww} map")
    out = torch.empty(N, dtype=torch.int32, device=gt.device)
    check(LIB.egz_cell_argmax_u8(gt.data_ptr(), N, Hh, Ww, cell, out.data_ptr(), _stream()), "egz_cell_argmax_u8")
    return out


def jet_table_restated():
    """OpenCV's COLORMAP_JET table restated (colormap.cpp: Jet::init, linear_colormap, linspace, interp1_) as a (256, 3) uint8
    BGR numpy array: base tables clip(1.5 - |4 i / 255 - c|, 0, 1) for c = 3 (R), 2 (G), 1 (B) at X = linspace(0, 1, 256) in
    float32, interpolated at the same points in float32, then convertTo(CV_8U, 255.) with cvRound.  Entries sit on .5 ties, so
    one float32 step that differs from cv2's flips an entry by 1: this table has NOT been checked against cv2 (see jet_lut)."""
    import numpy as np
    n = 256
    i = np.arange(n, dtype=np.float64)
    step = np.float32(np.float32(1) / np.float32(n - 1))
    X = (np.float32(0) + np.arange(n, dtype=np.float32) * step).astype(np.float32)
    planes = []
    for c in (1, 2, 3):                                   # B, G, R
        Y = np.clip(1.5 - np.abs(4.0 * i / 255.0 - c), 0.0, 1.0).astype(np.float32)
        yi = np.empty(n, np.float32)
        for k in range(n):
            xi = X[k]
            low, high = 0, n - 1
            if xi < X[low]:
                high = 1
            if xi > X[high]:
                low = high - 1
            while high - low > 1:
                m = low + ((high - low) >> 1)
                if xi > X[m]:
                    low = m
                else:
                    high = m
            t = np.float32(np.float32(xi - X[low]) * np.float32(Y[high] - Y[low])) / np.float32(X[high] - X[low])
            yi[k] = np.float32(0) + np.float32(Y[low] + np.float32(t))
        planes.append(yi)
    lut = np.stack(planes, 1).astype(np.float32)
    return np.clip(np.rint(lut * np.float32(255)), 0, 255).astype(np.uint8)


_JET = {}
_JET_WARNED = [False]


def jet_lut(device) -> torch.Tensor:
    """The (256, 3) uint8 BGR COLORMAP_JET table on ``device``: cv2's own table when cv2 imports (read once, by
    cv2.applyColorMap of a 0 .. 255 ramp), else jet_table_restated() -- unverified against cv2, with a warning the first time."""
    key = str(torch.device(device))
    hit = _JET.get(key)
    if hit is None:
        import numpy as np
        try:
            import cv2
            tab = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET).reshape(256, 3)
        except ImportError:
            if not _JET_WARNED[0]:
                import warnings
                warnings.warn("cv2 is not importable: using a restatement of OpenCV's COLORMAP_JET table that has not been "
                              "checked against cv2 (an entry may differ by 1); pass lut= for an exact table", stacklevel=2)
                _JET_WARNED[0] = True
            tab = _H.jet_table_restated()
        hit = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.uint8)).to(device)
        _JET[key] = hit
    return hit
