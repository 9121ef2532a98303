"""GTEA Gaze dataset preparation (the reference's misc/gazedataset_gt.py).

For every gaze track ``<gazePath>/<name>.txt`` (two columns x y per frame, 0 = no sample, 640 x 480 frames) it writes
``<fixationPath>/<name>_fixation.txt``, one ``str(float)`` fixation label per frame, and with ``--gt DIR`` the 224 x 224
ground-truth maps ``DIR/<name>/gt_%05d.jpg`` of every frame from 0 (sigma 35 at 480 x 640, rendered on the GPU by
``hipops.gaze_gt_maps`` in mode 1: the reference's np.uint8 cast, then cv2's uint8 area resize).

    python -m egaze_amd.misc.gazedataset_gt --gazePath gazepositions --fixationPath fixations [--gt images/GTEA_Gaze]
"""
import argparse
import operator
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

FRAME_SIZE = (480, 640)          # (H, W)
GT_SIZE = (224, 224)


def interpolate_track(gps):
    """(N, 2) samples -> (interpx, interpy): end samples that are 0 become the frame centre, each coordinate is linearly
    interpolated over its own non-zero samples (scipy interp1d, as the reference) and clipped to the frame."""
    from scipy.interpolate import interp1d
    gpx = np.array(gps[:, 0], dtype=np.float64)
    gpy = np.array(gps[:, 1], dtype=np.float64)
    if gpx[0] == 0:
        gpx[0] = 320
    if gpy[0] == 0:
        gpy[0] = 240
    if gpx[-1] == 0:
        gpx[-1] = 320
    if gpy[-1] == 0:
        gpy[-1] = 240
    x = np.arange(len(gpx))
    idx = np.nonzero(gpx)
    interpx = interp1d(x[idx], gpx[idx])(x)
    idx = np.nonzero(gpy)
    interpy = interp1d(x[idx], gpy[idx])(x)
    return interpx.clip(0, 640), interpy.clip(0, 480)


def fixation_state(interpx, interpy):
    """The reference's fixation state machine: a point within 50 px (squared distance < 2500) of the running centre of the
    current fixation is a fixation sample; the centre is the running mean in the reference's operation order; a fixation
    that ends after one sample clears the label of that sample."""
    fix_state = np.zeros((len(interpx),))
    fix_state[0] = 0
    center_pt = (interpx[0], interpy[0])
    fix_num = 0
    for pt_idx in range(1, interpx.shape[0]):
        current_pt = (interpx[pt_idx], interpy[pt_idx])
        if (center_pt[0] - current_pt[0]) ** 2 + (center_pt[1] - current_pt[1]) ** 2 < 2500.0:
            fix_state[pt_idx] = 1
            fix_num += 1
            center_pt = tuple(map(operator.mul, center_pt, (fix_num, fix_num)))
            center_pt = tuple(map(operator.add, center_pt, current_pt))
            center_pt = tuple(map(operator.truediv, center_pt, (fix_num + 1, fix_num + 1)))
        else:
            fix_state[pt_idx] = 0
            if fix_num == 1:
                fix_state[pt_idx - 1] = 0
            fix_num = 0
            center_pt = current_pt
    return fix_state


def impulse_indices(interpx, interpy):
    """The reference's impulse index int(round(v)) - 1 (numpy rounds half to even), -1 wrapping to the last row / column."""
    H, W = FRAME_SIZE
    rows = np.array([int(round(v)) - 1 for v in interpy], dtype=np.int64) % H
    cols = np.array([int(round(v)) - 1 for v in interpx], dtype=np.int64) % W
    return rows, cols


def render_maps(interpx, interpy, sigma=35.0, device='cuda', host=True):
    """uint8 (N, 224, 224) maps of a whole track: one launch, one read-back (host=False: left on the device)."""
    import torch
    from .. import hipops
    rows, cols = impulse_indices(interpx, interpy)
    u8, _, _ = hipops.gaze_gt_maps(torch.from_numpy(rows).to(device), torch.from_numpy(cols).to(device), FRAME_SIZE, sigma,
                                   GT_SIZE, mode=1)
    return u8.cpu().numpy() if host else u8


def process_track(t, args, pool):
    txtname = t[:-4]
    print('begin processing video %s' % txtname)
    gps = np.loadtxt(os.path.join(args.gazePath, t))
    interpx, interpy = interpolate_track(gps)
    fix_state = fixation_state(interpx, interpy)
    with open(os.path.join(args.fixationPath, t.strip().split('.')[0] + '_fixation.txt'), 'w') as fh:
        for v in fix_state:
            fh.write(str(v) + '\n')
    if args.gt is None:
        return []
    from ..data.dataset_preprocessing import encode_maps_gpu, write_bytes, write_map
    out = os.path.join(args.gt, txtname)
    os.makedirs(out, exist_ok=True)
    if getattr(args, 'gpu_encode', False):
        files = encode_maps_gpu(render_maps(interpx, interpy, args.sigma, args.device, host=False))
        return [pool.submit(write_bytes, os.path.join(out, 'gt_%05d.jpg' % j), files[j]) for j in range(len(files))]
    maps = render_maps(interpx, interpy, args.sigma, args.device)
    return [pool.submit(write_map, os.path.join(out, 'gt_%05d.jpg' % j), maps[j]) for j in range(len(maps))]


def build_parser():
    p = argparse.ArgumentParser(description="GTEA Gaze fixation labels and (optionally) ground-truth gaze maps")
    a = p.add_argument
    a('--gazePath', default='gazepositions', help="folder of <name>.txt gaze tracks (x y per frame)")
    a('--fixationPath', default='fixations', help="output folder of <name>_fixation.txt")
    a('--gt', default=None, metavar='DIR', help="also write DIR/<name>/gt_%%05d.jpg maps (rendered on the GPU)")
    a('--gpu-encode', action='store_true', help="encode the maps on the GPU (hipops.jpeg_encode, quality 95); the workers "
                                                "only write files")
    a('--sigma', type=float, default=35.0, help="Gaussian sigma in pixels of the 480 x 640 frame")
    a('--workers', type=int, default=8, help="threads encoding maps")
    a('--device', default='cuda', help="torch device the maps are rendered on")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.workers < 1:
        raise SystemExit("--workers must be at least 1")
    if args.gpu_encode and args.gt is None:
        parser.error("--gpu-encode needs --gt DIR: without it no maps are written")
    os.makedirs(args.fixationPath, exist_ok=True)
    pending = []
    with ThreadPoolExecutor(max_workers=args.workers) as pool:
        for t in sorted(os.listdir(args.gazePath)):
            futs = process_track(t, args, pool)
            for fu in pending:
                fu.result()
            pending = futs
        for fu in pending:
            fu.result()


if __name__ == '__main__':
    main()
