"""Dataset preparation and input pipeline: gaze maps, u8 normalise, the resident gathers (SP / AT, with and without augmentation, and late fusion), AT glue."""
from __future__ import annotations

import dataclasses
import math
import struct
import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, LaunchStatus, _p, _req, _stream, finish_launch
from .absmax import _new_absmax, _want_fwd_absmax
from .metrics import _gauss_weights

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- dataset preparation (ground-truth gaze maps)
def area_table(ssize: int, dsize: int):
    """OpenCV's INTER_AREA decimation table for one axis, non-integer scale (computeResizeAreaTab in imgproc/resize.cpp,
    restated here: cv2 is not a dependency of this package).  -> (ofs int32 [dsize + 1], si int32 [K], alpha float32 [K]):
    the entries of output index d are [ofs[d], ofs[d + 1]), in OpenCV's order."""
    import math
    import numpy as np
    if not (0 < dsize <= ssize):
        raise ValueError(f"area_table: INTER_AREA decimation needs 0 < dsize <= ssize (got {ssize} -> {dsize})")
    scale = 1.0 / (dsize / ssize)
    ofs, si, alpha = [0], [], []
    for d in range(dsize):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, ssize - fs1)
        s1, s2 = math.ceil(fs1), math.floor(fs2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        if s1 - fs1 > 1e-3:
            si.append(s1 - 1); alpha.append((s1 - fs1) / cell)
        for s in range(s1, s2):
            si.append(s); alpha.append(1.0 / cell)
        if fs2 - s2 > 1e-3:
            si.append(s2); alpha.append(min(min(fs2 - s2, 1.0), cell) / cell)
        ofs.append(len(si))
    return np.array(ofs, np.int32), np.array(si, np.int32), np.array(alpha, np.float32)


_AREA_T = {}


def _area_tables(device, src_hw, out_hw):
    key = (torch.device(device).index or 0, tuple(src_hw), tuple(out_hw))
    hit = _AREA_T.get(key)
    if hit is None:
        hit = tuple(tuple(torch.from_numpy(a).to(device) for a in _H.area_table(s, d)) for s, d in zip(src_hw, out_hw))
        _AREA_T[key] = hit
    return hit          # ((y ofs, si, alpha), (x ofs, si, alpha))


def gaze_gt_maps(rows: torch.Tensor, cols: torch.Tensor, src_hw, sigma: float, out_hw=(224, 224), mode: int = 0,
                 want_f64: bool = False, want_fullres: bool = False):
    """Ground-truth gaze maps of the reference's dataset preparation, N frames in one launch (egz_gaze_gt_maps).

    rows, cols: (N,) integer tensors on the GPU, the impulse position of each frame in [0, H) x [0, W) (negative indices
    already wrapped).  Each map is scipy.ndimage.gaussian_filter(impulse, sigma) over src_hw = (H, W), min-max normalised,
    times 255 and area-resized to out_hw: mode 0 resizes the float64 map and rounds (data/dataset_preprocessing.py, GTEA
    Gaze+, cv2.imwrite of a float64 image), mode 1 truncates to uint8 first and resizes with float accumulation
    (misc/gazedataset_gt.py, GTEA Gaze).  -> (u8 (N, oh, ow), f64 (N, oh, ow) or None, fullres (N, H, W) float64 or None),
    all on the GPU; the full-resolution maps cost 8 H W bytes each (tests)."""
    for t, name in ((rows, "rows"), (cols, "cols")):
        if not t.is_cuda:
            raise RuntimeError(f"gaze_gt_maps: {name}: expected a HIP ('cuda') tensor -- this package has no CPU path")
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool or t.dim() != 1:
            raise ValueError(f"gaze_gt_maps: {name} must be a 1-D integer tensor, got {t.dtype} {tuple(t.shape)}")
    if rows.numel() != cols.numel() or rows.numel() == 0 or rows.device != cols.device:
        raise ValueError(f"gaze_gt_maps: rows / cols must be non-empty, of one length and on one device "
                         f"({rows.numel()} vs {cols.numel()})")
    H, W = (int(v) for v in src_hw)
    oh, ow = (int(v) for v in out_hw)
    if mode not in (0, 1):
        raise ValueError(f"gaze_gt_maps: mode {mode} is neither 0 (GTEA Gaze+) nor 1 (GTEA Gaze)")
    if not (0 < oh <= H and 0 < ow <= W):
        raise ValueError(f"gaze_gt_maps: INTER_AREA decimation needs 0 < out <= src (got {(H, W)} -> {(oh, ow)})")
    if not sigma > 0:
        raise ValueError(f"gaze_gt_maps: sigma must be positive, got {sigma}")
    dev = rows.device
    gw, radius = _gauss_weights(dev, float(sigma))
    if radius >= min(H, W):
        raise ValueError(f"gaze_gt_maps: kernel radius {radius} (sigma {sigma}) must be below min(H, W) = {min(H, W)}")
    pos = torch.stack((rows.to(torch.int64), cols.to(dev, torch.int64)), 1)
    bad = ((pos[:, 0] < 0) | (pos[:, 0] >= H) | (pos[:, 1] < 0) | (pos[:, 1] >= W)).any()
    if bool(bad):
        raise ValueError(f"gaze_gt_maps: impulse positions must lie in [0, {H}) x [0, {W})")
    pos = pos.to(torch.int32).contiguous()
    (yo, ys, ya), (xo, xs, xa) = _area_tables(dev, (H, W), (oh, ow))
    N = pos.shape[0]
    u8 = torch.empty((N, oh, ow), dtype=torch.uint8, device=dev)
    f64 = torch.empty((N, oh, ow), dtype=torch.float64, device=dev) if want_f64 else None
    full = torch.empty((N, H, W), dtype=torch.float64, device=dev) if want_fullres else None
    check(LIB.egz_gaze_gt_maps(pos.data_ptr(), N, H, W, gw.data_ptr(), radius, xo.data_ptr(), xs.data_ptr(), xa.data_ptr(),
                               xs.numel(), yo.data_ptr(), ys.data_ptr(), ya.data_ptr(), ys.numel(), mode, oh, ow,
                               u8.data_ptr(), f64.data_ptr() if f64 is not None else None,
                               full.data_ptr() if full is not None else None, _stream()), "egz_gaze_gt_maps")
    return u8, f64, full


# ----------------------------------------------------------------------------- input pipeline / AT glue
_NORM_CONST = {}


def u8_normalize(src: torch.Tensor, mean, std) -> torch.Tensor:
    """src: uint8 (..., C, H, W) on the GPU -> fp32 (u8 / 255 - mean[c]) / std[c] (bit-exact with the torch expression)."""
    if src.dtype != torch.uint8 or not src.is_cuda or not src.is_contiguous():
        raise ValueError("u8_normalize: contiguous CUDA uint8 tensor expected")
    C, plane = src.shape[-3], src.shape[-2] * src.shape[-1]
    key = (src.device.index or 0, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    hit = _NORM_CONST.get(key)
    if hit is None:
        hit = (torch.tensor(key[1], dtype=torch.float32, device=src.device),
               torch.tensor(key[2], dtype=torch.float32, device=src.device))
        _NORM_CONST[key] = hit
    if hit[0].numel() != C:
        raise ValueError(f"u8_normalize: {C} channels but {hit[0].numel()} mean / std values")
    dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    check(LIB.egz_u8_normalize(src.data_ptr(), dst.data_ptr(), src.numel(), plane, C, hit[0].data_ptr(),
                               hit[1].data_ptr(), _stream()), "egz_u8_normalize")
    return dst


# ----------------------------------------------------------------------------- resident dataset (data/resident.py, --gpu_resident)
RESIDENT_STATUS = {1: "a sample number (idx) outside the table", 2: "a plane-table entry outside the pool",
                   3: "a sample number outside the table and a plane-table entry outside the pool"}
_RESIDENT_FIELDS = {'image': 1, 'flow': 2, 'gt': 4}


def judge_resident_status(st: int) -> None:
    """The rule for the status word of a gather (resident_gather, resident_gather_aug, late_gather): any bit raises."""
    if st:
        what = RESIDENT_STATUS.get(st) or AFFINE_STATUS.get(st, st)
        raise RuntimeError(f"resident_gather: {what}: the sample was skipped, its outputs are undefined")


def check_resident_status(pending) -> None:
    """Waits for the gather that ``pending = (host status word, event)`` belongs to and raises if it skipped a sample."""
    judge_resident_status(LaunchStatus(*pending).wait())


def _gather_operands(name, pool, table, idx, cols):
    """The operand checks of the gathers (``name`` the public function, ``cols`` the table's width) -> (device, P, H, W, B)."""
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda and pool.dtype == torch.uint8 and pool.dim() == 3
            and pool.is_contiguous()):
        raise ValueError(f"{name}: pool must be a contiguous uint8 (P, H, W) tensor on the GPU")
    dev = pool.device
    if not (table.device == dev and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == cols
            and table.is_contiguous()):
        raise ValueError(f"{name}: table must be a contiguous int64 (N, {cols}) tensor on the pool's device")
    if not (idx.device == dev and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous()):
        raise ValueError(f"{name}: idx must be a contiguous int64 (B,) tensor on the pool's device")
    return (dev, *pool.shape, idx.numel())


def _resident_fields(name, fields):
    fields = tuple(fields)
    if not fields or any(f not in _RESIDENT_FIELDS for f in fields):
        raise ValueError(f"{name}: fields {fields!r} must name some of 'image', 'flow', 'gt'")
    return fields


def _resident_consts(dev):
    """Mean and std of the 24 planes of the SP / AT layout (image 3, flow 20, ground truth 0 / 1) on ``dev``, made once."""
    from ..data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    key = ('resident', dev.index or 0)
    const = _NORM_CONST.get(key)
    if const is None:
        const = (torch.tensor(IMAGE_MEAN + FLOW_MEAN + (0.0,), dtype=torch.float32, device=dev),
                 torch.tensor(IMAGE_STD + FLOW_STD + (1.0,), dtype=torch.float32, device=dev))
        _NORM_CONST[key] = const
    return const


def _resident_outputs(dev, B, H, W, fields, raw, prepare):
    """The outputs of an SP / AT gather -> (image, flow, gt, xin, am, out_raw), None for what the launch does not produce: the
    bytes alone with ``raw``; the NHWC-32 flow stack and its abs-max buffer under the conditions of prepare_network_input."""
    new = lambda C: torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    image = flow = gt = xin = am = out_raw = None
    if raw:
        out_raw = torch.empty((B, 24, H, W), dtype=torch.uint8, device=dev)
    else:
        image = new(3) if 'image' in fields else None
        flow = new(20) if 'flow' in fields else None
        gt = new(1) if 'gt' in fields else None
        if flow is not None and prepare and _H.PRECISION == "split":
            xin = torch.empty((B, H, W, 32), dtype=torch.float32, device=dev)
            am = _new_absmax(dev)
    return image, flow, gt, xin, am, out_raw


def _resident_args(pool, table, idx, fields, outputs, status):
    """The 18 arguments the three SP / AT entry points begin with (_lib._RESIDENT_PREFIX)."""
    mean, std = _resident_consts(pool.device)
    P, H, W = pool.shape
    return (pool.data_ptr(), P, table.data_ptr(), table.shape[0], idx.data_ptr(), idx.numel(), H, W, mean.data_ptr(),
            std.data_ptr(), *(_p(t) for t in outputs), sum(_RESIDENT_FIELDS[f] for f in set(fields)), status.data_ptr())


def _attach_prepared(flow, xin, am):
    """Lets the NHWC-32 form that came out of the gather's launch ride on ``flow`` (``flow._egz_prepared``)."""
    if xin is None:
        return
    if _want_fwd_absmax():
        xin._egz_absmax = am
    ev = torch.cuda.Event()
    ev.record()
    flow._egz_prepared = (xin, flow._version, ev)


def resident_gather(pool: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, fields=('image', 'flow', 'gt'),
                    raw: bool = False, prepare: bool = True, status_to: Optional[dict] = None):
    """A batch of the SP / AT sample layout gathered from a pool of decoded planes on the device (egz_resident_gather).

    pool: uint8 (P, H, W); table: int64 (N, 22) plane numbers (column 0 the first of 3 BGR planes, 1 .. 20 the flow planes in
    STdatas order, 21 the ground truth); idx: int64 (B,) sample numbers; all on the GPU.  -> ``(image, flow, gt)`` fp32
    (B,3,H,W) / (B,20,H,W) / (B,1,H,W), normalised as data.STdatas.stage_batch does (bit-identical), None for a field not in
    ``fields``; with ``raw=True`` instead the uint8 (B,24,H,W) bytes (image 0:3, flow 3:23, gt 23; planes of fields not in
    ``fields`` are not written).  Under the conditions of prepare_network_input the flow stack's NHWC-32 form and its abs-max
    come out of the same launch and ride on ``flow`` (``flow._egz_prepared``).  An index out of range is never dereferenced:
    the status word is read here (a wait for this launch), or, with ``status_to`` (a dict, e.g. the collated sample), left
    there under '_resident_status' for check_resident_status at hand-over."""
    dev, P, H, W, B = _gather_operands("resident_gather", pool, table, idx, 22)
    fields = _resident_fields("resident_gather", fields)
    image, flow, gt, xin, am, out_raw = _resident_outputs(dev, B, H, W, fields, raw, prepare)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.egz_resident_gather(*_resident_args(pool, table, idx, fields, (image, flow, gt, xin, am, out_raw), status),
                                  _stream()), "egz_resident_gather")
    _attach_prepared(flow, xin, am)
    finish_launch(status, status_to, '_resident_status', judge_resident_status)
    return out_raw if raw else (image, flow, gt)


# ----------------------------------------------------------------------------- augmentation in the gather
RESIDENT_STATUS.update({
    4: "an explicit augmentation row out of range (flip not 0 / 1, |dy| or |dx| above 32767, or a non-finite gain / bias)",
    5: "a sample number outside the table and an explicit augmentation row out of range",
    6: "a plane-table entry outside the pool and an explicit augmentation row out of range",
    7: "a sample number outside the table, a plane-table entry outside the pool and an explicit augmentation row out of range"})


# Status values 8 .. 15: bit 3, an explicit row of the affine gather whose magnification or angle is out
# of range, alone and with each combination of bits 0 .. 2.  A table of its own: RESIDENT_STATUS keeps the seven values of the
# entry points without the affine step; check_resident_status reads both.
_AFFINE_ROW = "an explicit augmentation row with a magnification outside [0.5, 1.5], an angle beyond 45 degrees or either non-finite"
AFFINE_STATUS = {8: _AFFINE_ROW}
AFFINE_STATUS.update({8 + st: f"{RESIDENT_STATUS[st]}, and {_AFFINE_ROW}" for st in range(1, 8)})


@dataclasses.dataclass(frozen=True)
class AugSpec:
    """What resident_gather_aug draws per sample: ``flip`` the probability of a horizontal flip, ``shift`` the largest
    translation in pixels (dy and dx uniform in -shift .. shift), ``contrast`` / ``brightness`` the amplitudes of the colour
    frame's gain (1 +- contrast) and bias (+- brightness), ``seed`` the seed of the hash the draw comes from, ``scale`` the
    amplitude of the magnification (1 +- scale, at most 0.5) and ``rotate`` that of the rotation about the frame's centre in
    degrees (+- rotate, at most 45)."""
    flip: float = 0.0
    shift: int = 0
    contrast: float = 0.0
    brightness: float = 0.0
    seed: int = 0
    scale: float = 0.0
    rotate: float = 0.0

    def __post_init__(self):
        for name, typ in (("flip", float), ("shift", int), ("contrast", float), ("brightness", float), ("seed", int),
                          ("scale", float), ("rotate", float)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int,) if typ is int else (int, float)):
                raise ValueError(f"AugSpec: {name} = {v!r} is not {'an integer' if typ is int else 'a number'}")
            object.__setattr__(self, name, typ(v))
        if not 0.0 <= self.flip <= 1.0:
            raise ValueError(f"AugSpec: flip = {self.flip} is not a probability in [0, 1]")
        if not 0 <= self.shift <= 32767:
            raise ValueError(f"AugSpec: shift = {self.shift} outside 0 .. 32767 pixels")
        for name in ("contrast", "brightness"):
            if not 0.0 <= getattr(self, name) < 1.0:
                raise ValueError(f"AugSpec: {name} = {getattr(self, name)} outside [0, 1)")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"AugSpec: seed = {self.seed} outside 0 .. 2^64 - 1")
        if not 0.0 <= self.scale <= 0.5:
            raise ValueError(f"AugSpec: scale = {self.scale} outside [0, 0.5]")
        if not 0.0 <= self.rotate <= 45.0:
            raise ValueError(f"AugSpec: rotate = {self.rotate} outside [0, 45] degrees")

    @property
    def flip_thr(self) -> int:
        """floor(flip * 2^32): a sample is flipped when the high half of its first hash word is below it."""
        return int(math.floor(self.flip * 4294967296.0))

    @property
    def rotate_rad(self) -> float:
        """The rotation amplitude in radians as the fp32 value the device draws with: rounded once from fp64."""
        return struct.unpack("f", struct.pack("f", self.rotate * math.pi / 180.0))[0]

    @property
    def affine(self) -> bool:
        """Whether the draw magnifies or rotates: then the gather is egz_resident_gather_affine's."""
        return self.scale != 0.0 or self.rotate != 0.0

    @classmethod
    def parse(cls, text: str, seed: Optional[int] = None) -> "AugSpec":
        """'flip=0.5,shift=16,contrast=0.2,brightness=0.1,scale=0.15,rotate=10' (any subset, also 'seed=N'; a bare 'flip' means
        0.5) -> AugSpec; ``seed``, when given, replaces the text's."""
        kw = {}
        for item in str(text).split(","):
            key, eq, val = (s.strip() for s in item.partition("="))
            if key not in ("flip", "shift", "contrast", "brightness", "seed", "scale", "rotate") or key in kw:
                raise ValueError(f"AugSpec.parse: {item.strip()!r} in {text!r}: expected each of flip, shift, contrast, "
                                 f"brightness, seed, scale, rotate at most once, as name=value")
            if not eq:
                if key != "flip":
                    raise ValueError(f"AugSpec.parse: {key!r} in {text!r} needs a value (only a bare 'flip' has one: 0.5)")
                val = "0.5"
            try:
                kw[key] = int(val) if key in ("shift", "seed") else float(val)
            except ValueError:
                raise ValueError(f"AugSpec.parse: {key} = {val!r} in {text!r} is not a number") from None
        if seed is not None:
            kw["seed"] = seed
        return cls(**kw)

    def __str__(self):
        text = (f"flip={self.flip!r},shift={self.shift},contrast={self.contrast!r},brightness={self.brightness!r},"
                f"seed={self.seed}")
        for name in ("scale", "rotate"):                  # printed only when in use: a spec without them prints as it always did
            if getattr(self, name) != 0.0:
                text += f",{name}={getattr(self, name)!r}"
        return text


def resident_gather_aug(pool: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, spec: AugSpec, epoch: int,
                        fields=('image', 'flow', 'gt'), raw: bool = False, prepare: bool = True,
                        status_to: Optional[dict] = None, params: Optional[torch.Tensor] = None, want_params: bool = False):
    """resident_gather with augmentation in the same launch (egz_resident_gather_aug): per sample a horizontal flip and an
    integer translation applied alike to the colour frame, the flow planes (x-flow negated under a flip) and the ground truth,
    and a gain / bias on the colour frame.  The parameters are drawn on the device from a hash of (spec.seed, epoch, sample
    number) -- no host RNG is touched, and a sample's draw does not depend on its batch -- or taken from ``params``, an int32
    (B, 5) tensor on the pool's device with rows flip, dy, dx, float bits of gain, float bits of bias.  Needs W % 4 == 0.
    Everything else -- arguments, ``flow._egz_prepared``, the status word -- is resident_gather's; ``raw=True`` gives the bytes
    after the geometric step.  -> resident_gather's result, or ``(result, parameters used (B, 5) int32)`` with
    ``want_params``.

    A spec with ``scale`` or ``rotate``, or ``params`` of (B, 7) rows -- the five, then float bits of the magnification g and
    of the angle theta in radians -- goes through egz_resident_gather_affine: the picture is magnified
    and turned about its centre, sampled bilinearly, and the flow vectors turn and scale with it; the parameters used are then
    (B, 7) rows.  Without either the launch and its results are the ones described above."""
    if not isinstance(spec, AugSpec):
        raise ValueError(f"resident_gather_aug: spec must be an AugSpec, got {type(spec).__name__}")
    epoch = int(epoch)
    if not 0 <= epoch < 1 << 64:
        raise ValueError(f"resident_gather_aug: epoch = {epoch} outside 0 .. 2^64 - 1")
    dev, P, H, W, B = _gather_operands("resident_gather_aug", pool, table, idx, 22)
    fields = _resident_fields("resident_gather_aug", fields)
    if params is not None and not (isinstance(params, torch.Tensor) and params.device == dev and params.dtype == torch.int32
                                   and tuple(params.shape) in ((B, 5), (B, 7)) and params.is_contiguous()):
        raise ValueError(f"resident_gather_aug: params must be a contiguous int32 ({B}, 5) tensor on the pool's device"
                         f" (({B}, 7) with a magnification and an angle)")
    affine = spec.affine or (params is not None and params.shape[1] == 7)
    if affine and params is not None and params.shape[1] != 7:
        raise ValueError(f"resident_gather_aug: a spec with scale / rotate takes params of ({B}, 7) rows, got ({B}, 5)")
    image, flow, gt, xin, am, out_raw = _resident_outputs(dev, B, H, W, fields, raw, prepare)
    used = torch.empty((B, 7 if affine else 5), dtype=torch.int32, device=dev) if want_params else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (*_resident_args(pool, table, idx, fields, (image, flow, gt, xin, am, out_raw), status), spec.seed, epoch,
            spec.flip_thr, spec.shift, spec.contrast, spec.brightness, _p(params), _p(used))
    if affine:
        check(LIB.egz_resident_gather_affine(*args, spec.scale, spec.rotate_rad, _stream()), "egz_resident_gather_affine")
    else:
        check(LIB.egz_resident_gather_aug(*args, _stream()), "egz_resident_gather_aug")
    _attach_prepared(flow, xin, am)
    finish_launch(status, status_to, '_resident_status', judge_resident_status)
    out = out_raw if raw else (image, flow, gt)
    return (out, used) if want_params else out


def late_gather(pool: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, raw: bool = False,
                status_to: Optional[dict] = None):
    """A late-fusion batch gathered from a pool of decoded planes on the device (egz_late_gather).

    pool: uint8 (P, H, W); table: int64 (N, 3) plane numbers (SP prediction, AT map, ground truth); idx: int64 (B,) sample
    numbers; all on the GPU.  -> ``(fused, gt)`` fp32 (B,2,H,W) / (B,1,H,W), every value u8 / 255 as data.lateDataset makes it
    (bit-identical); fused channel 0 is the AT map and channel 1 the SP prediction, the tensor late_fusion's Cat2Planes would
    build.  With ``raw=True`` instead the uint8 (B,3,H,W) bytes in table order.  The status word is handled as in
    resident_gather."""
    dev, P, H, W, B = _gather_operands("late_gather", pool, table, idx, 3)
    fused = gt = out_raw = None
    if raw:
        out_raw = torch.empty((B, 3, H, W), dtype=torch.uint8, device=dev)
    else:
        fused = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        gt = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(LIB.egz_late_gather(pool.data_ptr(), P, table.data_ptr(), table.shape[0], idx.data_ptr(), B, H, W, _p(fused),
                              _p(gt), _p(out_raw), status.data_ptr(), _stream()), "egz_late_gather")
    finish_launch(status, status_to, '_resident_status', judge_resident_status)
    return out_raw if raw else (fused, gt)


def crop_mean(feat_nhwc: torch.Tensor, gp, size: int, cell: int = 16) -> torch.Tensor:
    """feat_nhwc: (B,H,W,C) fp32; gp: B gaze points (row, col) in input pixels -> chn_weight (B, C)."""
    _req(feat_nhwc, "feature")
    B, Hh, Ww, C = feat_nhwc.shape
    if isinstance(gp, torch.Tensor) and gp.is_cuda and gp.dtype == torch.int32 and gp.is_contiguous() and gp.numel() == 2 * B:
        g = gp                           # already on the device (u8_center_of_mass): no host round trip
    else:
        g = torch.as_tensor(gp, dtype=torch.int32).reshape(B, 2).to(feat_nhwc.device)
    out = torch.empty((B, C), dtype=torch.float32, device=feat_nhwc.device)
    check(LIB.egz_crop_mean(feat_nhwc.data_ptr(), g.data_ptr(), out.data_ptr(), B, Hh, Ww, C, int(size), int(cell),
                            _stream()), "egz_crop_mean")
    return out


def window_mean(feat_nhwc: torch.Tensor, windows) -> torch.Tensor:
    """feat_nhwc: (B,H,W,C) fp32; windows: B x (y0, y1, x0, x1) half-open cell ranges -> (B, C) window means."""
    _req(feat_nhwc, "feature")
    B, Hh, Ww, C = feat_nhwc.shape
    win = [tuple(int(v) for v in w) for w in windows]
    if len(win) != B or any(not (0 <= y0 < y1 <= Hh and 0 <= x0 < x1 <= Ww) for y0, y1, x0, x1 in win):
        raise ValueError(f"window_mean: windows {win} do not fit a {Hh} x {Ww} map of batch {B}")
    g = torch.tensor(win, dtype=torch.int32).to(feat_nhwc.device)
    out = torch.empty((B, C), dtype=torch.float32, device=feat_nhwc.device)
    check(LIB.egz_window_mean(feat_nhwc.data_ptr(), g.data_ptr(), out.data_ptr(), B, Hh, Ww, C, _stream()),
          "egz_window_mean")
    return out


def pixel_weighted_sum(feat_nhwc: torch.Tensor, wmap) -> torch.Tensor:
    """feat_nhwc: (B,H,W,C); wmap: (B,H,W) per-pixel weights (host array / tensor) -> (B, C) = sum_p wmap[p] * feat[p]."""
    _req(feat_nhwc, "feature")
    B, Hh, Ww, C = feat_nhwc.shape
    wm = torch.as_tensor(wmap, dtype=torch.float32).reshape(B, Hh * Ww).contiguous().to(feat_nhwc.device)
    out = torch.empty((B, C), dtype=torch.float32, device=feat_nhwc.device)
    check(LIB.egz_pixel_weighted_sum(feat_nhwc.data_ptr(), wm.data_ptr(), out.data_ptr(), B, Hh * Ww, C, _stream()),
          "egz_pixel_weighted_sum")
    return out


def weighted_minmax(feat_nhwc: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """feat_nhwc: (B,H,W,C), w: (B,C) -> (B,H,W): channel-weighted sum, min-max normalised per image."""
    _req(feat_nhwc, "feature"); _req(w, "chn_weight")
    B, Hh, Ww, C = feat_nhwc.shape
    out = torch.empty((B, Hh, Ww), dtype=torch.float32, device=feat_nhwc.device)
    check(LIB.egz_weighted_minmax(feat_nhwc.data_ptr(), w.data_ptr(), out.data_ptr(), B, Hh * Ww, C, _stream()),
          "egz_weighted_minmax")
    return out


def u8_center_of_mass(maps: torch.Tensor, want_u8: bool = False):
    """maps: (B, H, W) fp32 in [0, 1] -> (com (B, 2) float64, gp (B, 2) int32 = floor(com)[, q (B, H, W) uint8]): the
    reference's ``ndimage.center_of_mass((map * 255).astype(np.uint8))`` (run_spatialstream.py:99-104,130-131), bit for bit."""
    _req(maps, "map")
    B, Hh, Ww = maps.shape
    com = torch.empty((B, 2), dtype=torch.float64, device=maps.device)
    gp = torch.empty((B, 2), dtype=torch.int32, device=maps.device)
    q = torch.empty((B, Hh, Ww), dtype=torch.uint8, device=maps.device) if want_u8 else None
    check(LIB.egz_u8_center_of_mass(maps.data_ptr(), B, Hh, Ww, com.data_ptr(), gp.data_ptr(), _p(q), _stream()),
          "egz_u8_center_of_mass")
    return (com, gp, q) if want_u8 else (com, gp)


def bilinear_up(src: torch.Tensor, scale: int, align_corners: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: (B, h, w) -> (B, h*scale, w*scale), ``nn.functional.interpolate(mode='bilinear')`` with either align_corners
    convention.  ``out``: a (B, H, W) destination whose samples may be strided (e.g. ``x[:, 1]`` of a (B, 2, H, W) tensor --
    channel 1 of late_fusion's input) but whose rows are dense."""
    _req(src, "src")
    B, h, w = src.shape
    Hh, Ww = h * scale, w * scale
    if out is None:
        out = torch.empty((B, Hh, Ww), dtype=torch.float32, device=src.device)
    if tuple(out.shape) != (B, Hh, Ww) or out.dtype != torch.float32 or not out.is_cuda or out.stride(2) != 1 or out.stride(1) != Ww:
        raise RuntimeError(f"bilinear_up: destination {tuple(out.shape)} / strides {out.stride()} does not fit {(B, Hh, Ww)}")
    check(LIB.egz_bilinear_up(src.data_ptr(), out.data_ptr(), B, h, w, int(scale), int(bool(align_corners)),
                              out.stride(0) if B > 1 else Hh * Ww, _stream()), "egz_bilinear_up")
    return out
