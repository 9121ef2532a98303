"""Ground-truth gaze map rendering (hipops.gaze_gt_maps, csrc/gaze_gt.hip) and the dataset-preparation CLI: which one binds.

    python tools/bench_gt_maps.py [--n 4096] [--frames 3000] [--workers 8] [--cpu-frames 32] [--cpu-threads 16]

Prints one JSON line per measurement:
  kernel   maps/s of one N-frame launch per geometry (960 x 1280 sigma 70 mode 0; 480 x 640 sigma 35 mode 1), from device
           events, median of 5 launches after a warm-up; plus the rate with the uint8 read-back to the host.
  cli      frames/s of `python -m egaze_amd.data.dataset_preprocessing` (in process, main()) end to end on a synthetic tree of
           --frames frames under a temporary directory (JPEG maps, frame copies), with the time spent rendering (launch +
           read-back) and the rest (parse, encode, copy, waits) split out.
  cpu      frames/s of the reference's map path on the host -- scipy gaussian_filter, the reference's normalisation and an
           INTER_AREA restatement in numpy -- on --cpu-threads processes, and the ratio to the kernel and to the CLI.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def area_resize(S, out_hw, mode):
    """OpenCV's generic INTER_AREA in its accumulation order (see tests/test_dataset_prep_host.py)."""
    from egaze_amd.hipops import area_table
    wt = np.float64 if mode == 0 else np.float32
    (yo, ys, ya), (xo, xs, xa) = area_table(S.shape[0], out_hw[0]), area_table(S.shape[1], out_hw[1])
    S = S.astype(wt)
    buf = np.zeros((S.shape[0], out_hw[1]), wt)
    for dx in range(out_hw[1]):
        for k in range(xo[dx], xo[dx + 1]):
            buf[:, dx] += S[:, xs[k]] * wt(xa[k])
    out = np.zeros(out_hw, wt)
    for dy in range(out_hw[0]):
        for e in range(yo[dy], yo[dy + 1]):
            t = wt(ya[e]) * buf[ys[e]]
            out[dy] = t if e == yo[dy] else out[dy] + t
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def cpu_frame(job):
    from scipy import ndimage
    (H, W), sigma, mode, r, c = job
    g = np.zeros((H, W))
    g[r, c] = 1
    g = ndimage.gaussian_filter(g, sigma)
    g -= np.min(g)
    g /= np.max(g)
    g *= 255
    return area_resize(g if mode == 0 else g.astype(np.uint8), (224, 224), mode)


GEOMS = (("gplus", (960, 1280), 70.0, 0), ("gaze", (480, 640), 35.0, 1))


def bench_kernel(n, rs):
    import torch
    from egaze_amd import hipops
    res = {}
    for name, hw, sigma, mode in GEOMS:
        rows = torch.from_numpy(rs.randint(0, hw[0], n).astype(np.int32)).cuda()
        cols = torch.from_numpy(rs.randint(0, hw[1], n).astype(np.int32)).cuda()
        run = lambda: hipops.gaze_gt_maps(rows, cols, hw, sigma, (224, 224), mode)[0]
        run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        host = run().cpu()
        t_rb = time.perf_counter() - t0
        med = float(np.median(ms))
        res[name] = n / (med / 1e3)
        print(json.dumps({"bench": "kernel", "geometry": name, "src": list(hw), "sigma": sigma, "mode": mode, "n": n,
                          "ms": round(med, 3), "ms_all": [round(v, 3) for v in ms], "maps_per_s": round(res[name]),
                          "with_readback_maps_per_s": round(n / t_rb), "out_MB": round(host.numel() / 1e6, 1),
                          "write_GB_per_s": round(host.numel() / (med / 1e3) / 1e9, 1)}), flush=True)
    return res


def bench_cli(frames, workers, rs):
    from PIL import Image
    from egaze_amd.data import dataset_preprocessing as D
    per_video = 1000
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "gaze"))
        frame_jpg = os.path.join(tmp, "frame.jpg")
        Image.fromarray(rs.randint(0, 256, (224, 224, 3)).astype(np.uint8)).save(frame_jpg, quality=90)
        blob = open(frame_jpg, "rb").read()
        nv = max(1, frames // per_video)
        for v in range(nv):
            video = f"Synth{v}_Recipe"
            d = os.path.join(tmp, "flow", video)
            os.makedirs(d)
            lines = []
            for n in range(per_video + 1):
                lines.append(f"0\tSMP\t1\t{rs.uniform(0, 1279):.2f}\t{rs.uniform(0, 959):.2f}\t{n}\t"
                             f"{'Fixation' if rs.rand() < 0.7 else 'Saccade'}\n")
                with open(os.path.join(d, f"img_{n + 1:05d}.jpg"), "wb") as fh:
                    fh.write(blob)
            with open(os.path.join(tmp, "gaze", video + "_gaze.txt"), "w") as fh:
                fh.write("".join(lines))
        render = [0.0]
        orig = D.render_maps

        def timed_render(*a, **k):
            t0 = time.perf_counter()
            out = orig(*a, **k)
            render[0] += time.perf_counter() - t0
            return out
        D.render_maps = timed_render
        try:
            argv = ["--gazePath", os.path.join(tmp, "gaze"), "--flowPath", os.path.join(tmp, "flow"), "--imagePath",
                    os.path.join(tmp, "img"), "--gtPath", os.path.join(tmp, "gt"), "--fixsacPath", os.path.join(tmp, "fs"),
                    "--workers", str(workers)]
            D.main(argv + ["--fixsac-only"])                                         # warm-up: parse, imports
            D.render_maps(np.full(4, 640.0).tolist(), np.full(4, 480.0).tolist())
            render[0] = 0.0
            t0 = time.perf_counter()
            D.main(argv)
            total = time.perf_counter() - t0
        finally:
            D.render_maps = orig
        n = nv * per_video
        assert len(os.listdir(os.path.join(tmp, "gt"))) == n
    fps = n / total
    print(json.dumps({"bench": "cli", "frames": n, "videos": nv, "workers": workers, "gt_format": "jpg",
                      "s": round(total, 3), "frames_per_s": round(fps), "render_s": round(render[0], 3),
                      "rest_s": round(total - render[0], 3),
                      "bound_by": "render" if render[0] > 0.5 * total else "encode/copy/parse"}), flush=True)
    return fps


def bench_cpu(frames, threads, rs):
    res = {}
    for name, hw, sigma, mode in GEOMS:
        jobs = [(hw, sigma, mode, int(rs.randint(0, hw[0])), int(rs.randint(0, hw[1]))) for _ in range(frames)]
        with ProcessPoolExecutor(max_workers=threads, mp_context=mp.get_context("fork")) as ex:
            list(ex.map(cpu_frame, jobs[:threads]))            # warm-up: imports in every worker
            t0 = time.perf_counter()
            list(ex.map(cpu_frame, jobs))
            dt = time.perf_counter() - t0
        res[name] = frames / dt
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--cpu-frames", type=int, default=32)
    ap.add_argument("--cpu-threads", type=int, default=16)
    a = ap.parse_args()
    import egaze_amd  # noqa: F401
    rs = np.random.RandomState(0)
    cpu = bench_cpu(a.cpu_frames, a.cpu_threads, rs)        # first: its worker processes fork before the GPU is opened
    kern = bench_kernel(a.n, rs)
    cli = bench_cli(a.frames, a.workers, rs)
    for name, _, _, _ in GEOMS:
        print(json.dumps({"bench": "cpu", "geometry": name, "threads": a.cpu_threads, "frames": a.cpu_frames,
                          "frames_per_s": round(cpu[name], 2), "kernel_speedup": round(kern[name] / cpu[name]),
                          "cli_speedup": round(cli / cpu[name]) if name == "gplus" else None}), flush=True)


if __name__ == "__main__":
    main()
