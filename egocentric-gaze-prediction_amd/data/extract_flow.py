"""Optical-flow images of the temporal stream, computed on the GPU: the first preparation step of the reference's recipe, which
its README leaves to an external "dense flow" tool.

    python -m egaze_amd.data.extract_flow --framePath frames --flowPath gtea_imgflow [--size H W] [--bound 20]
                                          [--quality 95] [--chunk 32] [--folders a b ...] [--overwrite]

``framePath`` holds one sub-folder per video with its frames as ``img_%05d.jpg``.  For every sub-folder the sorted frames are read
in chunks of ``chunk`` pairs (chunk + 1 frames, consecutive chunks share one frame) and go through

    hipops.jpeg_decode -> resize_linear_u8 (with --size) -> bgr_to_gray_u8 -> tvl1_flow -> flow_to_u8 -> jpeg_encode (grey)

with one read-back of the encoded bytes per chunk.  ``flow_x_%05d.jpg`` / ``flow_y_%05d.jpg`` number n hold the flow from frame
n to the next frame, n being the number in the first frame's name (counted from 1): the last frame of a folder gets no flow, and
``STdatas.build_temporal_list`` reads the ten flows that end at a frame's number.  An output file that exists is kept unless
``--overwrite`` is given.  The algorithm, its parameters, ``bound`` and this numbering are defined in DESIGN.md ("TV-L1 optical
flow"); agreement with the external tool's own files is not verified.  Video decoding is out of scope: the input is frames.

``flows_into`` is the same chain without the files: it writes the flow images straight into the flow planes of resident
datasets on the device (``gaze_full --gpu_resident --flow_handover``)."""
import argparse
import os
import re

FLOW_NAMES = ('flow_x_%05d.jpg', 'flow_y_%05d.jpg')
# TV-L1 parameters of the command line, and of flows_into when it is given none
TVL1_DEFAULTS = {'tau': 0.25, 'lam': 0.15, 'theta': 0.3, 'zfactor': 0.5, 'nscales': 5, 'warps': 5, 'iterations': 30}


def list_frames(folder):
    """Sorted img_*.jpg of a folder -> [(number, file name)]; the number is the one in the name."""
    out = []
    for name in sorted(os.listdir(folder)):
        m = re.fullmatch(r'img_(\d+)\.jpe?g', name)
        if m:
            out.append((int(m.group(1)), name))
    return out


def chunk_ranges(nframes, chunk):
    """[(first, last)] frame index ranges, inclusive, of at most ``chunk`` pairs each; consecutive ranges share one frame."""
    return [(s, min(s + chunk, nframes - 1)) for s in range(0, nframes - 1, chunk)]


def decode_frames(paths, size, device):
    """Files -> (N, 3, H, W) uint8 BGR planes on the device, resized to ``size`` = (H, W) if given.  Files the GPU decoder does
    not take (progressive, arithmetic-coded, ...) are decoded on the host."""
    import torch
    from .. import hipops
    from .STdatas import sniff
    from ._io import imread
    blobs = []
    for p in paths:
        with open(p, 'rb') as fh:
            blobs.append(fh.read())
    sizes = [sniff(b) for b in blobs]
    gpu = [i for i, s in enumerate(sizes) if s is not None]
    host = {i: imread(paths[i]) for i, s in enumerate(sizes) if s is None}
    shapes = {tuple(sizes[i]) for i in gpu} | {tuple(im.shape[:2]) for im in host.values()}
    if len(shapes) != 1:
        raise SystemExit(f"{os.path.dirname(paths[0])}: frames of different sizes {sorted(shapes)}")
    H, W = shapes.pop()
    out = torch.empty((len(paths), 3, H, W), dtype=torch.uint8, device=device)
    if gpu:
        data = torch.frombuffer(bytearray(b''.join(blobs[i] for i in gpu)), dtype=torch.uint8).to(device)
        offsets = [0]
        for i in gpu:
            offsets.append(offsets[-1] + len(blobs[i]))
        _, status = hipops.jpeg_decode(data, offsets, (H, W), [3] * len(gpu), out=out, planes=[3 * i for i in gpu], n3=len(gpu))
        bad = [paths[gpu[k]] for k, s in enumerate(status.cpu().tolist()) if s]
        if bad:
            raise SystemExit(f"jpeg_decode refused {len(bad)} file(s), first: {bad[0]}")
    for i, im in host.items():
        out[i] = torch.from_numpy(im).permute(2, 0, 1).to(device)
    if size is not None and tuple(size) != (H, W):
        out = hipops.resize_linear_u8(out, tuple(size), layout='chw')
    return out


def flow_images(frames_bgr, bound, params):
    """(F, 3, H, W) BGR planes -> (2, F - 1, H, W) uint8 on the device: the x images, then the y images."""
    import torch
    from .. import hipops
    u1, u2 = hipops.tvl1_flow(hipops.bgr_to_gray_u8(frames_bgr), **params)
    return hipops.flow_to_u8(torch.stack((u1, u2)), bound)


def encode_gray(u8, quality):
    """(M, H, W) uint8 planes on the device -> list of M complete JPEG files as bytes-like objects: one encode, one read-back."""
    from .. import hipops
    data, offsets, status = hipops.jpeg_encode(u8, quality=quality)
    buf, off = data.cpu().numpy(), offsets.cpu().tolist()
    if int(status.abs().max()):
        raise RuntimeError(f"jpeg_encode: status {sorted(set(status.cpu().tolist()))}")
    return [buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def process_folder(src, dst, args, device='cuda'):
    """One video: writes the flow images of every frame pair of ``src`` into ``dst``; returns the number of files written."""
    frames = list_frames(src)
    if len(frames) < 2:
        return 0
    os.makedirs(dst, exist_ok=True)
    written = 0
    for first, last in chunk_ranges(len(frames), args.chunk):
        names = [[os.path.join(dst, fmt % frames[i][0]) for i in range(first, last)] for fmt in FLOW_NAMES]
        todo = [[args.overwrite or not os.path.exists(p) for p in row] for row in names]
        if not any(any(row) for row in todo):
            continue
        bgr = decode_frames([os.path.join(src, frames[i][1]) for i in range(first, last + 1)], args.size, device)
        u8 = flow_images(bgr, args.bound, args.params)
        files = encode_gray(u8.reshape((-1,) + tuple(u8.shape[-2:])), args.quality)
        n = last - first
        for c in range(2):
            for i in range(n):
                if todo[c][i]:
                    with open(names[c][i], 'wb') as fh:
                        fh.write(files[c * n + i])
                    written += 1
    return written


# ----------------------------------------------------------------------------- hand-over into the resident ST pool (no files)
def flow_key(path):
    """A flow path of STdatas.build_temporal_list, used as a key only -> (folder name, 0 for x / 1 for y, number)."""
    m = re.fullmatch(r'flow_([xy])_(\d+)\.jpg', os.path.basename(path))
    if not m:
        raise ValueError(f"{path}: not a flow_x_%05d.jpg / flow_y_%05d.jpg name")
    return os.path.basename(os.path.dirname(path)), 'xy'.index(m.group(1)), int(m.group(2))


def missing_frame(numbers, n):
    """The frame whose absence makes flow ``n`` unavailable from the frames ``numbers`` (a set), or None: flow n runs from
    frame n to frame n + 1."""
    return n if n not in numbers else (n + 1 if n + 1 not in numbers else None)


def wanted_ranges(frames, wanted, chunk):
    """process_folder's chunk ranges over ``frames`` (list_frames' result) that hold at least one flow number of ``wanted``:
    the ranges of the others are neither decoded nor computed, as its ``todo`` skips ranges whose files all exist."""
    return [(first, last) for first, last in chunk_ranges(len(frames), chunk)
            if any(frames[i][0] in wanted for i in range(first, last))]


def flows_into(datasets, framePath, device, size=None, bound=20.0, quality=95, chunk=32, params=None):
    """Computes the flow images the filled ``datasets`` (data.resident.ResidentSTDatasets planned with ``flow_from``) refer
    to and writes them into the planes their plans gave to the flow paths, without a file: per video folder the chunk ranges
    of process_folder, the same chain up to flow_to_u8, then ONE hipops.jpeg_roundtrip launch per chunk and pool in place of
    jpeg_encode -> file -> read -> jpeg_decode -- the same bytes (the entropy coding is lossless; the quantisation is kept).
    ``quality`` 0 stores the flow_to_u8 planes as they are.  A flow no sample refers to gets no plane, a range in which none
    is referred to is neither decoded nor computed.  ``size`` (H, W): the frames are resized to it first; default: the
    pools' plane size.  The device is waited for once, at the end, for the status words (not at all with quality 0).
    -> {'pairs': frame pairs computed, 'planes': planes written, 'files': 0}."""
    import torch
    from .. import hipops
    if chunk < 1:
        raise ValueError("flows_into: chunk must be at least 1")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 0 <= quality <= 100:
        raise ValueError(f"flows_into: quality {quality!r} outside 0 .. 100 (0: no JPEG round trip)")
    params = dict(TVL1_DEFAULTS if params is None else params)
    datasets = [ds for ds in datasets if len(ds) and getattr(ds, 'flow_keys', None)]
    for ds in datasets:
        if ds.pool is None:
            raise RuntimeError("flows_into: fill(device, flow_from=...) has not run (the pool is not on the device)")
    hws = {tuple(ds.hw) for ds in datasets}
    if len(hws) > 1:
        raise RuntimeError(f"flows_into: the pools hold planes of different sizes {sorted(hws)}")
    if size is None and hws:
        size = next(iter(hws))
    wanted = {}                             # folder -> {number -> [(dataset index, 0 x / 1 y, plane)]}
    for k, ds in enumerate(datasets):
        for path, plane in ds.flow_keys:
            folder, c, n = flow_key(path)
            wanted.setdefault(folder, {}).setdefault(n, []).append((k, c, plane))
    counts = {'pairs': 0, 'planes': 0, 'files': 0}
    statuses = []
    for folder in sorted(wanted):
        src = os.path.join(framePath, folder)
        frames = list_frames(src)
        want = wanted[folder]
        for first, last in wanted_ranges(frames, want, chunk):
            bgr = decode_frames([os.path.join(src, frames[i][1]) for i in range(first, last + 1)], size, device)
            u8 = flow_images(bgr, bound, params)
            n = last - first
            u8 = u8.reshape((2 * n,) + tuple(u8.shape[-2:]))
            counts['pairs'] += n
            per_pool = {}
            for i in range(n):
                for k, c, plane in want.get(frames[first + i][0], ()):
                    per_pool.setdefault(k, []).append((c * n + i, plane))
            for k, pairs in per_pool.items():
                pool = datasets[k].pool
                if tuple(u8.shape[-2:]) != tuple(pool.shape[-2:]):
                    raise RuntimeError(f"{src}: flow images of {tuple(u8.shape[-2:])} pixels, the pool holds planes of "
                                       f"{tuple(pool.shape[-2:])}")
                sel = [s for s, _ in pairs]
                dst = torch.tensor([p for _, p in pairs], dtype=torch.int64).to(pool.device, non_blocking=True)
                planes = u8 if sel == list(range(2 * n)) else \
                    u8.index_select(0, torch.tensor(sel, dtype=torch.int64).to(u8.device, non_blocking=True))
                if quality:
                    statuses.append(hipops.jpeg_roundtrip(planes, quality, out=pool, plane_index=dst)[1])
                else:
                    pool.index_copy_(0, dst, planes)
                counts['planes'] += len(pairs)
    if statuses:
        bad = torch.cat(statuses).cpu()     # the one wait
        if int(bad.abs().max()):
            raise RuntimeError(f"flows_into: jpeg_roundtrip status {sorted(set(bad.tolist()))}: "
                               f"{hipops.JPEG_ROUNDTRIP_STATUS[1]}")
    return counts


def build_parser():
    p = argparse.ArgumentParser(description="TV-L1 optical-flow images (flow_x_*.jpg, flow_y_*.jpg) of folders of frames, "
                                            "computed on the GPU")
    a = p.add_argument
    a('--framePath', required=True, help="folder of per-video folders holding img_%%05d.jpg frames")
    a('--flowPath', required=True, help="output folder: one folder per video with flow_x_%%05d.jpg / flow_y_%%05d.jpg")
    a('--size', type=int, nargs=2, metavar=('H', 'W'), default=None, help="resize the frames (8-bit INTER_LINEAR) first")
    a('--bound', type=float, default=20.0, help="flow of +-bound pixels maps to 255 / 0")
    a('--quality', type=int, default=95, help="JPEG quality of the flow images")
    a('--chunk', type=int, default=32, help="frame pairs per GPU batch")
    a('--folders', nargs='*', default=None, help="sub-folders to process (default: all)")
    a('--overwrite', action='store_true', help="recompute and replace output files that exist")
    a('--device', default='cuda', help="torch device")
    for name, default in TVL1_DEFAULTS.items():
        a('--' + name, type=type(default), default=default, help=f"TV-L1 parameter (default {default})")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.chunk < 1:
        parser.error("--chunk must be at least 1")
    if not 1 <= args.quality <= 100:
        parser.error("--quality must be 1 .. 100")
    if not args.bound > 0:
        parser.error("--bound must be positive")
    args.params = {k: getattr(args, k) for k in ('tau', 'lam', 'theta', 'nscales', 'zfactor', 'warps', 'iterations')}
    if args.size is not None:
        args.size = tuple(args.size)
    folders = args.folders if args.folders else sorted(
        d for d in os.listdir(args.framePath) if os.path.isdir(os.path.join(args.framePath, d)))
    total = 0
    for d in folders:
        src = os.path.join(args.framePath, d)
        if not os.path.isdir(src):
            parser.error(f"--folders: {src} is not a folder")
        n = process_folder(src, os.path.join(args.flowPath, d), args, args.device)
        print(f"{d}/ {n} files")
        total += n
    return total


if __name__ == '__main__':
    main()
