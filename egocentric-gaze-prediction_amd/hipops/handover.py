"""The AT -> LF hand-over on the device (late_input: predict.py's; late_store: AT.extract_late(into=...)'s, straight into a
resident late-fusion pool), the SP -> AT hand-over (lstm_store: extractLSTMw.extractw(into=...)'s, straight into a resident
LSTM vector pool) and the gaze marker of an overlay (draw_ring)."""
from __future__ import annotations

import functools
import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, LaunchStatus, _p, _stream, finish_launch

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time

LATE_INPUT_STATUS = {1: "a NaN was quantised to 0", 2: "a value outside [0, 1] was clamped",
                     3: "a NaN was quantised to 0 and a value outside [0, 1] was clamped"}


# ----------------------------------------------------------------------------- the operand checks of the three ops
def _operand(t, name, what, dtypes, dim, form, dev=None, on="", shape=None, refuse=None):
    """One device operand of a hand-over op: a tensor on ``dev`` (None: on any GPU), non-empty, of one of ``dtypes`` with
    ``dim`` dimensions (of exactly ``shape`` where given; ``form`` spells the shape in the message), not refused by
    ``refuse(t)`` (-> the rest of a message, or None) and contiguous.  ``on`` is the op's wording of "must be ... ``dev``".
    -> t"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if dev is None and not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a HIP ('cuda') tensor -- this package has no CPU path")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: {name} must be {on} {dev}, got {t.device}")
    if t.dtype not in dtypes or t.dim() != dim or min(t.shape) == 0 or (shape is not None and tuple(t.shape) != shape):
        kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what}: {name} must be a non-empty {kinds} {form}, got {t.dtype} {tuple(t.shape)}")
    why = refuse(t) if refuse is not None else None
    if why is not None:
        raise ValueError(f"{what}: {name} {why}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous, got strides {t.stride()} for {tuple(t.shape)}")
    return t


def _map_dev(t, name, what):
    return _operand(t, name, what, (torch.float32, torch.uint8), 3, "(B, H, W)")


def _map_pair(sp, at, what):
    """The SP and AT maps of late_input / late_store -> (samples, H, W, h, w)."""
    _map_dev(sp, "sp", what)
    _map_dev(at, "at", what)
    if sp.device != at.device:
        raise ValueError(f"{what}: sp and at must be on one device ({sp.device} vs {at.device})")
    if sp.shape[0] != at.shape[0]:
        raise ValueError(f"{what}: {sp.shape[0]} SP maps but {at.shape[0]} AT maps")
    if sp.shape[0] > 65535:
        raise ValueError(f"{what}: {sp.shape[0]} samples in one launch (65535 at most)")
    return tuple(int(v) for v in sp.shape) + (int(at.shape[1]), int(at.shape[2]))


def check_rows(dst, shape, dev, what, noun, cols=None):
    """The host half of _rows_dev: ``dst`` is a contiguous int64 tensor of ``shape`` on ``dev`` or on the host, and outside
    -1 no number is named twice in it (in its columns ``cols`` where given: the others are not written through).  Two
    writers of one ``noun`` ('plane', 'row') have no defined order, so a repeat is refused, naming the first.  A device
    ``dst`` is read back for this (a wait)."""
    if not (isinstance(dst, torch.Tensor) and dst.dtype == torch.int64 and tuple(dst.shape) == tuple(shape)
            and dst.is_contiguous() and (dst.device == dev or dst.device.type == 'cpu')):
        got = f"{dst.dtype} {tuple(dst.shape)} on {dst.device}" if isinstance(dst, torch.Tensor) else type(dst).__name__
        raise ValueError(f"{what}: dst must be a contiguous int64 {tuple(shape)} tensor on {dev} or on the host, got {got}")
    named = (dst if cols is None else dst[:, :cols]).cpu().numpy().ravel()
    named = named[named != -1].tolist()
    if len(set(named)) != len(named):
        seen = set()
        twice = next(int(v) for v in named if v in seen or seen.add(v))
        raise ValueError(f"{what}: dst names {noun} {twice} twice in one call")


def _rows_dev(dst, shape, dev, what, noun, cols=None):
    """The destination numbers of a store, checked (check_rows) -> on ``dev``: a host ``dst`` is uploaded from pinned memory
    without waiting for the device."""
    check_rows(dst, shape, dev, what, noun, cols)
    if dst.device.type == 'cpu':
        pinned = torch.empty(tuple(shape), dtype=torch.int64, pin_memory=True)
        pinned.copy_(dst)
        dst = pinned.to(dev, non_blocking=True)
    return dst


# ----------------------------------------------------------------------------- AT -> LF
def late_input(sp: torch.Tensor, at: torch.Tensor, want_u8: bool = False, status_to: Optional[dict] = None):
    """late_fusion's input from the SP map and the AT map of a batch, as AT.extract_late's files and data.lateDataset would
    hand it over, in one launch (egz_late_input).

    sp: (B, H, W) fp32 SP map, or uint8 (already quantised); at: (B, h, w) fp32 AT map (weighted_minmax's output), or uint8;
    contiguous, on one GPU.  fp32 values are quantised as ``(255 * x).to(torch.uint8)`` (truncation), the AT plane at h x w and
    then resized to H x W with resize_linear_u8's arithmetic (cv2.resize, INTER_LINEAR).  -> fused (B, 2, H, W) fp32, channel 0
    the AT plane / 255 and channel 1 the SP plane / 255 -- LF.trainLate's order, bit-identical with late_gather of the same
    planes; with ``want_u8`` also planes (B, 2, H, W) uint8 in the same order.  NaN or x < 0 gives 0, 255 x >= 256 gives 255 (a
    NaN AT map is legitimate: weighted_minmax of a constant map is 0 / 0).  The launch's status word (bit 0: NaN, bit 1: out
    of range) is handled as late_gather's: read here (a wait for this launch; a non-zero word warns, the outputs are defined), or,
    with ``status_to`` (a dict), left there as ``(pinned host word, event)`` under '_late_input_status' for late_input_status."""
    what = "late_input"
    B, Hh, Ww, h, w = _map_pair(sp, at, what)
    if B * 2 * Hh * Ww * 4 >= 1 << 32:
        raise ValueError(f"{what}: a fused output of {B * 2 * Hh * Ww * 4} bytes; below 4 GiB per launch")
    dev = sp.device
    tabs = (None,) * 4 if (h, w) == (Hh, Ww) else _H._linear_tables(dev, (h, w), (Hh, Ww), what)
    fused = torch.empty((B, 2, Hh, Ww), dtype=torch.float32, device=dev)
    planes = torch.empty((B, 2, Hh, Ww), dtype=torch.uint8, device=dev) if want_u8 else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.egz_late_input(sp.data_ptr(), int(sp.dtype == torch.uint8), at.data_ptr(), int(at.dtype == torch.uint8), B, Hh, Ww,
                             h, w, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), fused.data_ptr(), _p(planes),
                             status.data_ptr(), _stream()), "egz_late_input")
    # (bit 2 cannot come up here, so the rule is late_store's; the warning points at this function's caller)
    finish_launch(status, status_to, '_late_input_status', functools.partial(_H.check_late_store_status, who=what, stacklevel=4))
    return (fused, planes) if want_u8 else fused


def late_input_status(pending) -> int:
    """Waits for the late_input launch that ``pending = (host status word, event)`` belongs to -> its status word (0: every
    value was inside [0, 1]; LATE_INPUT_STATUS names the bits).  Nothing was skipped: the outputs are defined either way."""
    return LaunchStatus(*pending).wait()


LATE_STORE_STATUS = {**LATE_INPUT_STATUS, 4: "a plane number outside its pool (that sample wrote nothing)"}


def late_store(sp: torch.Tensor, at: torch.Tensor, late_pool: torch.Tensor, dst: torch.Tensor,
               gt_pool: Optional[torch.Tensor] = None, gt_src: Optional[torch.Tensor] = None, status_to: Optional[dict] = None):
    """late_input's two planes of a chunk written straight into a late-fusion pool (data.late_resident), and the ground-truth
    plane of every sample copied beside them, in one launch (egz_late_store).  No fp32 tensor is produced.

    sp (n, H, W) and at (n, h, w): as late_input takes them.  late_pool: uint8 (P, H, W), contiguous, on the same GPU.  dst:
    int64 (n, 3), the planes of late_pool that take the SP plane, the AT plane and the ground truth of each sample, in
    ResidentLateDataset's column order; -1 skips a plane.  gt_pool: uint8 (Q, H, W) on the same GPU with gt_src: int64 (n,) on
    that GPU, the plane of gt_pool each sample's ground truth is copied from; without them the third column is skipped.
    A plane named twice in ``dst`` is refused (two writers of one plane have no defined order).  ``dst`` may be a host tensor:
    it is checked there and uploaded from pinned memory without waiting for the device; a device ``dst`` is read back for the
    check (a wait).  A number outside [-1, P) in ``dst`` or outside [0, Q) in ``gt_src`` is never dereferenced: that sample
    writes nothing and bit 2 of the status word goes up; bits 0 / 1 are late_input's, for the maps that were stored.  The word
    is read here (a wait; bits 0 / 1 warn, bit 2 raises), or, with ``status_to`` (a dict), left there as ``(pinned host word,
    event)`` under '_late_store_status' for late_store_status.  -> late_pool."""
    what = "late_store"
    n, Hh, Ww, h, w = _map_pair(sp, at, what)
    dev = sp.device

    on = "a HIP ('cuda') tensor on the maps' device"

    def other_planes(t):
        return None if tuple(t.shape[1:]) == (Hh, Ww) else f"holds planes of {tuple(t.shape[1:])}, sp has {(Hh, Ww)}"
    _operand(late_pool, "late_pool", what, (torch.uint8,), 3, "(P, H, W)", dev, on, refuse=other_planes)
    if (gt_pool is None) != (gt_src is None):
        raise ValueError(f"{what}: gt_pool and gt_src go together")
    if gt_pool is not None:
        _operand(gt_pool, "gt_pool", what, (torch.uint8,), 3, "(P, H, W)", dev, on, refuse=other_planes)
        _operand(gt_src, "gt_src", what, (torch.int64,), 1, f"({n},)", dev, on, shape=(n,))
        lo, hi = late_pool.data_ptr(), late_pool.data_ptr() + late_pool.numel()
        if gt_pool.data_ptr() < hi and lo < gt_pool.data_ptr() + gt_pool.numel():
            raise ValueError(f"{what}: gt_pool overlaps late_pool")
    dst = _rows_dev(dst, (n, 3), dev, what, "plane", cols=None if gt_pool is not None else 2)
    tabs = (None,) * 4 if (h, w) == (Hh, Ww) else _H._linear_tables(dev, (h, w), (Hh, Ww), what)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.egz_late_store(sp.data_ptr(), int(sp.dtype == torch.uint8), at.data_ptr(), int(at.dtype == torch.uint8), n, Hh, Ww,
                             h, w, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]), late_pool.data_ptr(),
                             late_pool.shape[0], dst.data_ptr(), _p(gt_pool), 0 if gt_pool is None else gt_pool.shape[0],
                             _p(gt_src), status.data_ptr(), _stream()), "egz_late_store")
    finish_launch(status, status_to, '_late_store_status', functools.partial(_H.check_late_store_status, stacklevel=4))
    return late_pool


def late_store_status(pending) -> int:
    """Waits for the late_store launch that ``pending = (host status word, event)`` belongs to -> its status word
    (LATE_STORE_STATUS names the bits)."""
    return LaunchStatus(*pending).wait()


def check_late_store_status(st: int, who: str = "late_store", stacklevel: int = 2):
    """The rule for a late_store status word: bit 2 (a plane number outside its pool: samples were skipped) raises, bits 0 / 1
    (defined values were stored) warn as late_input does."""
    if st & 4:
        raise RuntimeError(f"{who}: {LATE_STORE_STATUS[4]}")
    if st:
        import warnings
        warnings.warn(f"{who}: {LATE_STORE_STATUS.get(st, st)}", RuntimeWarning, stacklevel=stacklevel)


# ----------------------------------------------------------------------------- SP -> AT
LSTM_STORE_STATUS = {1: "a ground-truth plane number or a pool row outside its pool (that sample wrote nothing)"}


def lstm_store(feat_nhwc: torch.Tensor, gt_pool: torch.Tensor, gt_src: torch.Tensor, pool: torch.Tensor, dst: torch.Tensor,
               size: int, cell: int = 16, want_cells: bool = False, status_to: Optional[dict] = None):
    """The LSTM vectors of a chunk written straight into a resident vector pool (data.lstm_resident), in one launch
    (egz_lstm_store): what extractLSTMw.channel_weight(feat, gt, size, align=False) computes per sample and extractw writes to
    fix_<name>.pth.tar, bit for bit, without the ground truth leaving the device.

    feat_nhwc: fp32 (B, H, W, C) channels-last, H == W (the reference clips both window coordinates with H).  gt_pool: uint8
    (Q, H cell, W cell) with gt_src: int64 (B,), the plane of gt_pool that is each sample's ground truth.  pool: fp32 (rows, C)
    with dst: int64 (B,), the row that takes each sample's vector; -1 skips the sample.  All contiguous and on one GPU, but
    ``dst`` may be a host tensor: it is checked there and uploaded from pinned memory without waiting for the device; a device
    ``dst`` is read back for the check (a wait).  A row named twice is refused.  The gaze cell is the first arg-max of
    avg_pool2d(gt / 255, cell) in ATen's CPU summation order, the window extractLSTMw.var_window(cell, size), the mean
    window_mean's.  A number outside [-1, rows) in ``dst`` or outside [0, Q) in ``gt_src`` is never dereferenced: that sample
    writes nothing and bit 0 of the status word goes up.  The word is read here (a wait; bit 0 raises), or, with ``status_to``
    (a dict), left there as ``(pinned host word, event)`` under '_lstm_store_status' for lstm_store_status.
    -> pool, or (pool, cells) with ``want_cells``: cells int32 (B,), the flat gaze cell of every stored sample (-1: skipped)."""
    what, on = "lstm_store", "on the features' device"
    for name, t in (("feat_nhwc", feat_nhwc), ("gt_pool", gt_pool), ("gt_src", gt_src), ("pool", pool), ("dst", dst)):
        if not isinstance(t, torch.Tensor):           # all five before anything else is judged
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    _operand(feat_nhwc, "feat_nhwc", what, (torch.float32,), 4, "(B, H, W, C)")
    dev = feat_nhwc.device
    B, Hh, Ww, C = (int(v) for v in feat_nhwc.shape)
    if Hh != Ww:
        raise ValueError(f"{what}: a {Hh} x {Ww} map: H == W is needed (the reference clips both window coordinates with H)")
    if B > 65535:
        raise ValueError(f"{what}: {B} samples in one launch (65535 at most)")
    for name, v, lo, hi in (("cell", cell, 1, 256), ("size", size, 1, Hh)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}, got {v!r}")
    planes = (Hh * cell, Ww * cell)
    _operand(gt_pool, "gt_pool", what, (torch.uint8,), 3, "(Q, H, W)", dev, on,
             refuse=lambda t: None if tuple(t.shape[1:]) == planes else
             f"holds planes of {tuple(t.shape[1:])}, a {Hh} x {Ww} map with cell {cell} needs {planes}")
    _operand(pool, "pool", what, (torch.float32,), 2, "(rows, C)", dev, on,
             refuse=lambda t: None if t.shape[1] == C else f"rows hold {t.shape[1]} values, feat_nhwc has C = {C} channels")
    _operand(gt_src, "gt_src", what, (torch.int64,), 1, f"({B},)", dev, on, shape=(B,))
    dst = _rows_dev(dst, (B,), dev, what, "row")
    cells = torch.full((B,), -1, dtype=torch.int32, device=dev) if want_cells else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.egz_lstm_store(feat_nhwc.data_ptr(), B, Hh, Ww, C, gt_pool.data_ptr(), gt_pool.shape[0], gt_src.data_ptr(), cell,
                             size, pool.data_ptr(), pool.shape[0], dst.data_ptr(), _p(cells), status.data_ptr(), _stream()),
          "egz_lstm_store")
    finish_launch(status, status_to, '_lstm_store_status', _H.check_lstm_store_status)
    return (pool, cells) if want_cells else pool


def lstm_store_status(pending) -> int:
    """Waits for the lstm_store launch that ``pending = (host status word, event)`` belongs to -> its status word
    (LSTM_STORE_STATUS names the bit)."""
    return LaunchStatus(*pending).wait()


def check_lstm_store_status(st: int, who: str = "lstm_store"):
    """The rule for an lstm_store status word: bit 0 (samples were skipped) raises."""
    if st & 1:
        raise RuntimeError(f"{who}: {LSTM_STORE_STATUS[1]}")


def draw_ring(images: torch.Tensor, centers: torch.Tensor, r_in: int, r_out: int, colour=(255, 255, 255)) -> torch.Tensor:
    """A ring (r_in = 0: a disc) drawn into M images in place, one launch (egz_draw_ring).

    images: (M, H, W, 3) uint8, contiguous, on the GPU (BGR as everywhere here); centers: (M, 2) int32 (row, col) on the same
    GPU, inside the image or not (the ring is clipped); 0 <= r_in <= r_out integers; colour: three bytes in the images' channel
    order.  Pixel (y, x) takes the colour iff r_in^2 <= (y - cy)^2 + (x - cx)^2 <= r_out^2, in integers.  -> images."""
    what = "draw_ring"
    if not isinstance(images, torch.Tensor) or not isinstance(centers, torch.Tensor):
        raise ValueError(f"{what}: images and centers must be tensors")
    if not images.is_cuda or not centers.is_cuda or images.device != centers.device:
        raise ValueError(f"{what}: images and centers must be HIP ('cuda') tensors on one device -- this package has no CPU path")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or min(images.shape) == 0:
        raise ValueError(f"{what}: images must be a non-empty uint8 (M, H, W, 3), got {images.dtype} {tuple(images.shape)}")
    if centers.dtype != torch.int32 or tuple(centers.shape) != (images.shape[0], 2):
        raise ValueError(f"{what}: centers must be int32 ({images.shape[0]}, 2), got {centers.dtype} {tuple(centers.shape)}")
    if not images.is_contiguous() or not centers.is_contiguous():
        raise ValueError(f"{what}: images and centers must be contiguous")
    for name, v in (("r_in", r_in), ("r_out", r_out)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if not 0 <= r_in <= r_out < 1 << 30:
        raise ValueError(f"{what}: radii {r_in} .. {r_out}: 0 <= r_in <= r_out is needed")
    col = tuple(int(c) for c in colour)
    if len(col) != 3 or any(not 0 <= c <= 255 for c in col):
        raise ValueError(f"{what}: colour {colour!r} must be three values in 0 .. 255")
    M, Hh, Ww = (int(v) for v in images.shape[:3])
    if M > 65535:
        raise ValueError(f"{what}: {M} images in one launch (65535 at most)")
    check(LIB.egz_draw_ring(images.data_ptr(), M, Hh, Ww, centers.data_ptr(), r_in, r_out, col[0], col[1], col[2], _stream()),
          "egz_draw_ring")
    return images
