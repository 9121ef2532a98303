"""GTEA Gaze+ dataset preparation, the first step of the reference's recipe (data/dataset_preprocessing.py).

For every gaze log ``<gazePath>/<video>_gaze.txt`` it writes, with the reference's file names (data/STdatas.py and
``STdatas.build_temporal_list`` parse them):
  ``<fixsacPath>/<video>.txt``            fixation (1) / saccade (0) label of frames 1 .. n-1 (np.savetxt default format)
  ``<imagePath>/<video>_<img>``           a copy of ``<flowPath>/<video>/<img>`` for the sorted ``img`` frames 1 .. n-1
  ``<gtPath>/<video>_gt_<img>``           the 224 x 224 ground-truth gaze map of that frame

The reference's map code (kept in a string literal there, which the README points users to) filters a 960 x 1280 float64
impulse with scipy's gaussian_filter(sigma 70), min-max normalises it, multiplies by 255, area-resizes it with cv2 and writes
it with cv2.imwrite; here all maps of a video are rendered in one ``hipops.gaze_gt_maps`` launch (bit-identical arithmetic,
see csrc/gaze_gt.hip) and read back once, while a thread pool encodes the maps and copies the frames.  With ``--gpu-encode``
the maps stay on the device, ``hipops.jpeg_encode`` makes the JPEG files of a whole video in one call (byte-identical with
the quality-95 files libjpeg-turbo writes), the bytes are read back once and the pool only writes files and copies frames.

    python -m egaze_amd.data.dataset_preprocessing --gazePath gtea_gaze --flowPath gtea_imgflow \\
        --imagePath gtea_images --gtPath gtea_gts --fixsacPath fixsac

``--fixsac-only`` writes the label files only, which is all the reference's live code does.
"""
import argparse
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np

GTEA_SIZE = (960, 1280)          # (H, W) of the gaze coordinates (the reference's gtea_size)
GT_SIZE = (224, 224)


def parsetxt(filename):
    """-> (gazex, gazey, nframe, fixsac): one entry per frame from the first logged one on, exactly as the reference's
    parsetxt builds them (lines starting with '#' or 'T' skipped; columns 3 / 4 / 5 = x / y / frame, 'Fix' in column 6 =
    fixation; in range means 0 <= round(x) < 1280 and 0 <= round(y) < 960 with Python's half-to-even round):
      - an out-of-range first sample becomes frame 0 at (640, 480);
      - a gap is filled with the last gaze and the last label;
      - an out-of-range new frame repeats the last gaze and is labelled 0 (saccade);
      - a repeated frame is averaged into the last entry when in range, otherwise ignored.
    One deviation: a frame number below the first one sends the reference's gap-filling loop into an endless loop; it raises
    ValueError here."""
    gazex, gazey, nframe, fixsac = [], [], [], []
    seen = set()                 # the reference tests `frame not in nframe` with a list scan (quadratic)

    def in_range(s):
        return 0 <= int(round(float(s[3]))) < 1280 and 0 <= int(round(float(s[4]))) < 960

    def push(frame, x, y, label):
        nframe.append(frame); gazex.append(x); gazey.append(y); fixsac.append(label)
        seen.add(frame)

    with open(filename, 'r') as fh:
        for line in fh:
            if line.startswith('#') or line.startswith('T'):
                continue
            s = line.split()
            frame = int(s[5])
            label = 1 if 'Fix' in s[6] else 0
            if not nframe:
                if in_range(s):
                    push(frame, float(s[3]), float(s[4]), label)
                else:
                    push(0, 640.0, 480.0, label)
            elif frame not in seen:
                if frame < nframe[-1] + 1:
                    raise ValueError(f"{filename}: frame {frame} precedes the first frame {nframe[0]} of the log "
                                     "(the reference's gap filling never ends on it)")
                while nframe[-1] + 1 != frame:
                    push(nframe[-1] + 1, gazex[-1], gazey[-1], fixsac[-1])
                if in_range(s):
                    push(frame, float(s[3]), float(s[4]), label)
                else:
                    push(frame, gazex[-1], gazey[-1], 0)        # gaze estimation error counts as a saccade
            elif in_range(s):
                gazex[-1] = (gazex[-1] + float(s[3])) / 2
                gazey[-1] = (gazey[-1] + float(s[4])) / 2
    return gazex, gazey, nframe, fixsac


def impulse_index(v, size):
    """The reference's array index int(round(v)) - 1 reduced to [0, size): -1 is the last row / column (numpy)."""
    i = int(round(v)) - 1
    if not -size <= i < size:
        raise ValueError(f"gaze coordinate {v} is outside a map of size {size}")
    return i % size


def write_map(path, u8):
    """Write one uint8 map: cv2.imwrite where cv2 is installed (JPEG quality 95 is its default), else PIL with the same
    quality; PNG is lossless either way."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        if not cv2.imwrite(path, u8):
            raise OSError(f"cv2.imwrite failed on {path}")
        return
    from PIL import Image
    im = Image.fromarray(u8)
    if path.lower().endswith(('.jpg', '.jpeg')):
        im.save(path, quality=95)
    else:
        im.save(path)


def gt_name(video, img, gt_format):
    """<video>_gt_<img>, with the image's extension replaced by .png for lossless maps (the 3-letter extension keeps
    build_temporal_list's positional parse valid)."""
    if gt_format == 'png':
        img = os.path.splitext(img)[0] + '.png'
    return video + '_gt_' + img


def write_bytes(path, data):
    with open(path, 'wb') as fh:
        fh.write(data)


def encode_maps_gpu(u8, quality=95):
    """JPEG files of the uint8 (N, H, W) maps ``u8`` on the GPU: one hipops.jpeg_encode call, one read-back of the bytes.
    -> list of N uint8 arrays (views of one buffer), each a complete file."""
    from .. import hipops
    data, offsets, status = hipops.jpeg_encode(u8, quality=quality)
    buf, off = data.cpu().numpy(), offsets.cpu().tolist()
    if int(status.abs().max()):
        raise RuntimeError(f"jpeg_encode: status {sorted(set(status.cpu().tolist()))}")
    return [buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def render_maps(gazex, gazey, sigma=70.0, device='cuda', host=True):
    """uint8 (N, 224, 224) maps of the frames (gazex[i], gazey[i]) on the host: one launch, one read-back.  host=False
    leaves them on the device as a tensor."""
    import torch
    from .. import hipops
    H, W = GTEA_SIZE
    rows = torch.tensor([impulse_index(y, H) for y in gazey], dtype=torch.int32)
    cols = torch.tensor([impulse_index(x, W) for x in gazex], dtype=torch.int32)
    u8, _, _ = hipops.gaze_gt_maps(rows.to(device), cols.to(device), GTEA_SIZE, sigma, GT_SIZE, mode=0)
    return u8.cpu().numpy() if host else u8


def process_video(f, args, pool, device='cuda'):
    """Parse one gaze log and write its outputs; returns the futures of the queued copies and encodes."""
    video = f[:-9]
    gazex, gazey, nframe, fixsac = parsetxt(os.path.join(args.gazePath, f))
    np.savetxt(os.path.join(args.fixsacPath, video + '.txt'), fixsac[1:])
    if args.fixsac_only or len(nframe) < 2:
        return []
    ims = sorted(k for k in os.listdir(os.path.join(args.flowPath, video)) if 'img' in k)
    if len(ims) < len(nframe):
        raise SystemExit(f"{video}: {len(ims)} img frames in {os.path.join(args.flowPath, video)} but the gaze log covers "
                         f"{len(nframe)} frames")
    futs = []
    if not args.no_copy_images:
        for i in range(1, len(nframe)):
            futs.append(pool.submit(shutil.copyfile, os.path.join(args.flowPath, video, ims[i]),
                                    os.path.join(args.imagePath, video + '_' + ims[i])))
    if getattr(args, 'gpu_encode', False):
        files = encode_maps_gpu(render_maps(gazex[1:], gazey[1:], args.sigma, device, host=False))
        for i in range(1, len(nframe)):
            futs.append(pool.submit(write_bytes, os.path.join(args.gtPath, gt_name(video, ims[i], args.gt_format)),
                                    files[i - 1]))
        return futs
    maps = render_maps(gazex[1:], gazey[1:], args.sigma, device)
    for i in range(1, len(nframe)):
        futs.append(pool.submit(write_map, os.path.join(args.gtPath, gt_name(video, ims[i], args.gt_format)), maps[i - 1]))
    return futs


def build_parser():
    p = argparse.ArgumentParser(description="GTEA Gaze+ dataset preparation: fixation labels, frame copies and "
                                            "ground-truth gaze maps (rendered on the GPU)")
    a = p.add_argument
    a('--gazePath', default='gtea_gaze', help="folder of <video>_gaze.txt gaze logs")
    a('--flowPath', default='gtea_imgflow', help="folder of per-video folders holding img_* / flow_x_* / flow_y_* frames")
    a('--imagePath', default='gtea_images', help="output folder of the copied RGB frames")
    a('--gtPath', default='gtea_gts', help="output folder of the ground-truth gaze maps")
    a('--fixsacPath', default='fixsac', help="output folder of the fixation / saccade label files")
    a('--fixsac-only', action='store_true', help="write the label files only (the reference's live code)")
    a('--no-copy-images', action='store_true', help="do not copy the RGB frames")
    a('--gt-format', choices=('jpg', 'png'), default='jpg', help="jpg: the reference's names, quality 95; png: lossless")
    a('--gpu-encode', action='store_true', help="encode the JPEG maps on the GPU (hipops.jpeg_encode, quality 95); the "
                                                "workers only write files")
    a('--sigma', type=float, default=70.0, help="Gaussian sigma in pixels of the 960 x 1280 gaze frame")
    a('--workers', type=int, default=8, help="threads encoding maps and copying frames")
    a('--device', default='cuda', help="torch device the maps are rendered on")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.workers < 1:
        raise SystemExit("--workers must be at least 1")
    if args.gpu_encode and args.gt_format != 'jpg':
        parser.error("--gpu-encode writes JPEG maps: it cannot be combined with --gt-format png")
    os.makedirs(args.fixsacPath, exist_ok=True)
    if not args.fixsac_only:
        os.makedirs(args.gtPath, exist_ok=True)
        if not args.no_copy_images:
            os.makedirs(args.imagePath, exist_ok=True)
    gazefiles = sorted(os.listdir(args.gazePath))
    pending = []
    with ThreadPoolExecutor(max_workers=args.workers) as pool:
        for f in gazefiles:
            print(f[:-9] + '/')
            futs = process_video(f, args, pool, args.device)
            for fu in pending:           # the previous video's files are written while this one was parsed and rendered
                fu.result()
            pending = futs
        for fu in pending:
            fu.result()


if __name__ == '__main__':
    main()
