"""Baseline JPEG decode and encode, and the round trip through both without the bitstream."""
from __future__ import annotations

import sys

import torch

from .._lib import check
from ._core import LIB, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- JPEG decode (data/STdatas.py, decode='gpu')
JPEG_STATUS = {0: "ok", 1: "corrupt data", 2: "unsupported JPEG", 3: "size differs from the requested output",
               4: "unreadable JPEG (libjpeg refuses it: bad header or table, no scan)"}


def _dev_table(t, dtype, device, name):
    if isinstance(t, torch.Tensor):
        if t.dim() != 1:
            raise ValueError(f"jpeg_decode: {name} must be 1-D, got {tuple(t.shape)}")
        return t.to(device=device, dtype=dtype, non_blocking=True).contiguous()
    return torch.tensor(list(t), dtype=dtype).to(device, non_blocking=True)


def jpeg_decode(data: torch.Tensor, offsets, out_hw, channels, out: torch.Tensor = None, planes=None, n3: int = None,
                stages: int = 2):
    """Baseline JPEG decode of N streams in one call (egz_jpeg_decode), bit-identical with cv2.imread.

    data: uint8 1-D tensor on the GPU, the concatenated files; offsets: N + 1 byte offsets (stream i is data[offsets[i]:
    offsets[i + 1]]); out_hw = (H, W), the size every stream must have; channels: per stream 1 (cv2.IMREAD_GRAYSCALE: the Y
    plane of a colour file) or 3 (BGR; a grayscale file is replicated).  Tables may be lists or tensors on either device.
    -> (u8, status): u8 is ``out`` or a new (N, C, H, W) tensor, C = 3 if any stream asks for colour, else 1; status (N,)
    int32 on the GPU (JPEG_STATUS).  ``out`` (uint8, contiguous, on the GPU) is read as planes of H x W: stream i fills
    planes[i] .. planes[i] + channels[i] - 1 (default planes[i] = i * C), so a caller can decode straight into slices of a
    batch tensor.  n3: number of streams with channels 3 -- counted from ``channels`` when not given (a device sync if the
    table is on the GPU).  stages=1 stops after the entropy decode (timing only; ``out`` is not written)."""
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        raise RuntimeError("jpeg_decode: data: expected a HIP ('cuda') tensor -- this package has no CPU decode path")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError(f"jpeg_decode: data must be a contiguous 1-D uint8 tensor, got {data.dtype} {tuple(data.shape)}")
    H, W = (int(v) for v in out_hw)
    if not (0 < H <= 4096 and 0 < W <= 4096):
        raise ValueError(f"jpeg_decode: out_hw {(H, W)} outside 1 .. 4096")
    dev = data.device
    if n3 is None:
        ch = channels.cpu() if isinstance(channels, torch.Tensor) else torch.tensor(list(channels))
        if not bool(((ch == 1) | (ch == 3)).all()):
            raise ValueError("jpeg_decode: channels must be 1 or 3 per stream")
        n3 = int((ch == 3).sum())
    off = _dev_table(offsets, torch.int64, dev, "offsets")
    chn = _dev_table(channels, torch.int32, dev, "channels")
    N = chn.numel()
    if N == 0 or off.numel() != N + 1:
        raise ValueError(f"jpeg_decode: {N} streams need {N + 1} offsets, got {off.numel()}")
    if not 0 <= n3 <= N:
        raise ValueError(f"jpeg_decode: n3={n3} outside [0, {N}]")
    C = 3 if n3 else 1
    if out is None:
        if planes is not None:
            raise ValueError("jpeg_decode: planes= needs out=")
        out = torch.empty((N, C, H, W), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() % (H * W) or out.device != dev:
        raise ValueError(f"jpeg_decode: out must be a contiguous uint8 GPU tensor of whole {H} x {W} planes on {dev}")
    pl = (torch.arange(N, dtype=torch.int64) * C).to(dev, non_blocking=True) if planes is None else \
        _dev_table(planes, torch.int64, dev, "planes")
    if pl.numel() != N:
        raise ValueError(f"jpeg_decode: {N} streams but {pl.numel()} plane indices")
    status = torch.empty(N, dtype=torch.int32, device=dev)
    nb = LIB.egz_jpeg_decode_ws_bytes(N, H, W, n3)
    ws = _H.workspace(nb, dev)
    check(LIB.egz_jpeg_decode(data.data_ptr(), data.numel(), off.data_ptr(), chn.data_ptr(), pl.data_ptr(), N, H, W,
                              out.data_ptr(), out.numel() // (H * W), status.data_ptr(), ws.data_ptr(), nb, n3, stages,
                              _stream()), "egz_jpeg_decode")
    return out, status


# ----------------------------------------------------------------------------- JPEG encode (--gpu-encode / --gpu_encode)
JPEG_ENCODE_STATUS = {0: "ok", 1: "the output slot is smaller than the file (nothing of it was written)"}
_SUBSAMPLING = {"420": 420, "4:2:0": 420, 420: 420, 2: 420}


def _jpeg_encode_args(images, quality, layout, subsampling):
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError("jpeg_encode: images: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if images.dtype != torch.uint8:
        raise ValueError(f"jpeg_encode: images must be uint8, got {images.dtype}")
    if layout is None:
        layout = "bgr" if images.dim() == 4 else "gray"
    if layout not in ("gray", "bgr"):
        raise ValueError(f"jpeg_encode: layout {layout!r}: 'gray' (N, H, W) or 'bgr' (N, H, W, 3) -- RGB, planar colour, "
                         "CMYK and 12-bit input are not built")
    if (layout == "gray" and images.dim() != 3) or (layout == "bgr" and (images.dim() != 4 or images.shape[3] != 3)):
        raise ValueError(f"jpeg_encode: images of shape {tuple(images.shape)} do not match layout {layout!r}: "
                         "'gray' is (N, H, W), 'bgr' is (N, H, W, 3)")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_encode: quality {quality!r} outside 1 .. 100")
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"jpeg_encode: subsampling {subsampling!r}: only '420' is built (Pillow's and cv2's default); "
                         "'444' and '422' are not")
    N, H, W = (int(v) for v in images.shape[:3])
    if not (0 < H <= 4096 and 0 < W <= 4096):
        raise ValueError(f"jpeg_encode: images of {H} x {W}: height and width must be 1 .. 4096")
    if not 0 < N <= 65535:
        raise ValueError(f"jpeg_encode: images holds {N} images: 1 .. 65535 per call")
    return images.contiguous(), N, H, W, (3 if layout == "bgr" else 1), _SUBSAMPLING[subsampling]


def _jpeg_encode_scan(img, N, H, W, C, quality, sub, stages=4):
    """First half of the encode: -> (workspace, its size, needed lengths (N,) int64 on the GPU)."""
    nb = LIB.egz_jpeg_encode_ws_bytes(N, H, W, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=img.device)        # hundreds of MB for a large batch: not the shared scratch
    needed = torch.zeros(N, dtype=torch.int64, device=img.device)
    check(LIB.egz_jpeg_encode(img.data_ptr(), N, H, W, C, quality, sub, ws.data_ptr(), nb, needed.data_ptr(), stages,
                              _stream()), "egz_jpeg_encode")
    return ws, nb, needed


def jpeg_encode(images: torch.Tensor, quality: int = 95, layout: str = None, subsampling="420"):
    """Baseline JPEG encode of N images in one call (egz_jpeg_encode), every file byte-identical with Pillow's
    Image.save(format="JPEG", quality=quality) -- libjpeg-turbo's defaults, which cv2.imwrite runs too.

    images: uint8 on the GPU, (N, H, W) grey (layout 'gray') or (N, H, W, 3) BGR (layout 'bgr', written as YCbCr 4:2:0);
    layout defaults to the one the shape implies.  -> (data, offsets, status): data a 1-D uint8 GPU tensor of the N complete
    files one after the other, offsets N + 1 int64 on the GPU (file i is data[offsets[i]:offsets[i + 1]]), status (N,) int32
    on the GPU (JPEG_ENCODE_STATUS; all 0 here) -- what jpeg_decode takes as (data, offsets).  The N lengths are read back
    once, between the entropy coding and the final write, to allocate the exact output."""
    img, N, H, W, C, sub = _jpeg_encode_args(images, quality, layout, subsampling)
    ws, nb, needed = _jpeg_encode_scan(img, N, H, W, C, quality, sub)
    offsets = torch.zeros(N + 1, dtype=torch.int64)
    torch.cumsum(needed.cpu(), 0, out=offsets[1:])                    # the one read-back
    data = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=img.device)
    off = offsets.to(img.device)
    lengths = torch.empty(N, dtype=torch.int64, device=img.device)
    status = torch.empty(N, dtype=torch.int32, device=img.device)
    check(LIB.egz_jpeg_encode_write(ws.data_ptr(), nb, N, H, W, C, data.data_ptr(), data.numel(), off.data_ptr(),
                                    needed.data_ptr(), lengths.data_ptr(), status.data_ptr(), _stream()),
          "egz_jpeg_encode_write")
    return data, off, status


def jpeg_encode_into(images: torch.Tensor, out: torch.Tensor, slot_offsets, slot_capacity, quality: int = 95,
                     layout: str = None, subsampling="420"):
    """jpeg_encode into a buffer of the caller's, without the read-back: file i goes to out[slot_offsets[i]:] if it fits in
    slot_capacity[i] bytes (and in ``out``).  -> (lengths, status), both (N,) on the GPU: the length every file needs, and
    0, or 1 where the slot was too small -- then nothing of that file is written."""
    img, N, H, W, C, sub = _jpeg_encode_args(images, quality, layout, subsampling)
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise RuntimeError("jpeg_encode_into: out: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != img.device or not out.numel():
        raise ValueError(f"jpeg_encode_into: out must be a non-empty contiguous 1-D uint8 tensor on {img.device}")
    so = _dev_table(slot_offsets, torch.int64, img.device, "slot_offsets")
    sc = _dev_table(slot_capacity, torch.int64, img.device, "slot_capacity")
    if so.numel() != N or sc.numel() != N:
        raise ValueError(f"jpeg_encode_into: {N} images need {N} slot_offsets and {N} slot_capacity entries, got "
                         f"{so.numel()} and {sc.numel()}")
    ws, nb, _ = _jpeg_encode_scan(img, N, H, W, C, quality, sub)
    lengths = torch.empty(N, dtype=torch.int64, device=img.device)
    status = torch.empty(N, dtype=torch.int32, device=img.device)
    check(LIB.egz_jpeg_encode_write(ws.data_ptr(), nb, N, H, W, C, out.data_ptr(), out.numel(), so.data_ptr(), sc.data_ptr(),
                                    lengths.data_ptr(), status.data_ptr(), _stream()), "egz_jpeg_encode_write")
    return lengths, status


# ----------------------------------------------------------------------------- JPEG round trip (flow hand-over, predict)
JPEG_ROUNDTRIP_STATUS = {0: "ok", 1: "the plane index is outside the destination (nothing of the plane was written)"}


def jpeg_roundtrip(planes: torch.Tensor, quality: int = 95, out: torch.Tensor = None, plane_index=None):
    """The planes jpeg_decode gives for jpeg_encode(planes, quality), bit for bit, in one launch (egz_jpeg_roundtrip): per
    8x8 block FDCT, quantisation, dequantisation, IDCT.  The entropy coding between the two is lossless and is left out, so
    there is no bitstream, no workspace and no read-back.

    planes: (N, H, W) uint8 on the GPU.  -> (out, status): ``out`` is a new (N, H, W) tensor, or the caller's (uint8,
    contiguous, on the same GPU), read as whole H x W planes: plane i goes to plane plane_index[i] (default i; a list or a
    tensor on either device).  status (N,) int32 on the GPU (JPEG_ROUNDTRIP_STATUS): 1 where the index is outside ``out`` --
    that plane is not written.  ``out`` may be ``planes`` itself with the default index (in place); any other overlap of
    ``out`` with ``planes`` is refused."""
    if not isinstance(planes, torch.Tensor) or not planes.is_cuda:
        raise RuntimeError("jpeg_roundtrip: planes: expected a HIP ('cuda') tensor -- this package has no CPU path")
    if planes.dtype != torch.uint8:
        raise ValueError(f"jpeg_roundtrip: planes must be uint8, got {planes.dtype}")
    if planes.dim() != 3:
        raise ValueError(f"jpeg_roundtrip: planes of shape {tuple(planes.shape)}: expected (N, H, W) grey planes")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_roundtrip: quality {quality!r} outside 1 .. 100")
    N, H, W = (int(v) for v in planes.shape)
    if not (0 < H <= 4096 and 0 < W <= 4096):
        raise ValueError(f"jpeg_roundtrip: planes of {H} x {W}: height and width must be 1 .. 4096")
    if N < 1:
        raise ValueError("jpeg_roundtrip: planes holds no plane")
    dev = planes.device
    src = planes.contiguous()
    if out is None:
        if plane_index is not None:
            raise ValueError("jpeg_roundtrip: plane_index= needs out=")
        out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() \
            or out.numel() % (H * W) or not out.numel() or out.device != dev:
        raise ValueError(f"jpeg_roundtrip: out must be a contiguous uint8 GPU tensor of whole {H} x {W} planes on {dev}")
    pl = None
    if plane_index is not None:
        pl = _dev_table(plane_index, torch.int64, dev, "plane_index")
        if pl.numel() != N:
            raise ValueError(f"jpeg_roundtrip: {N} planes but {pl.numel()} plane indices")
    nbytes = N * H * W
    lo, hi = max(src.data_ptr(), out.data_ptr()), min(src.data_ptr() + nbytes, out.data_ptr() + out.numel())
    if lo < hi and not (pl is None and src.data_ptr() == out.data_ptr()):
        raise ValueError("jpeg_roundtrip: out overlaps planes: only out = planes itself with the default plane_index (in "
                         "place) is supported")
    status = torch.empty(N, dtype=torch.int32, device=dev)
    check(LIB.egz_jpeg_roundtrip(src.data_ptr(), N, H, W, quality, pl.data_ptr() if pl is not None else None,
                                 out.data_ptr(), out.numel() // (H * W), status.data_ptr(), _stream()),
          "egz_jpeg_roundtrip")
    return out, status
