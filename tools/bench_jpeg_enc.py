"""JPEG encode on the GPU (hipops.jpeg_encode) next to Pillow on the same box; prints one JSON line per item (profiles/jpeg_encode.txt).
  kernel   device time of egz_jpeg_encode cut after each stage (device events, median of --reps) and of the whole
           hipops.jpeg_encode call (both entry points, the read-back of the lengths and the output allocation; wall clock
           around a device synchronisation), for 4,096 gaze maps, 4,096 noisy grey frames and 30 colour overlays
  host     the same images through Pillow in 1 and in 16 processes
  cli      data/dataset_preprocessing on a synthetic tree with and without --gpu-encode, alternated in this call
  vis      overlay batch -> files on disk with and without the device encode (tools/bench_vis.py's chain, 30 overlays)
Usage: python tools/bench_jpeg_enc.py [--reps 7] [--frames 3000] [--workers 8]"""
import argparse
import io
import json
import multiprocessing
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = {1: "transform", 2: "transform+scan", 3: "transform+scan+pack", 4: "all_but_final_write"}


def inputs():
    import torch
    from egaze_amd import hipops as H
    rng = np.random.default_rng(0)
    n = 4096
    rows = torch.from_numpy(rng.integers(0, 960, n).astype(np.int32)).cuda()
    cols = torch.from_numpy(rng.integers(0, 1280, n).astype(np.int32)).cuda()
    maps, _, _ = H.gaze_gt_maps(rows, cols, (960, 1280), 70.0, (224, 224), mode=0)
    y, x = np.mgrid[0:224, 0:224]
    noisy = np.empty((n, 224, 224), np.uint8)
    for i in range(n):                                     # the decoder bench's grey content
        base = 128 + 80 * np.sin(x * rng.uniform(0.02, 0.1) + rng.uniform(0, 6)) * np.cos(y * rng.uniform(0.02, 0.1))
        noisy[i] = np.clip(base + rng.normal(0, 8, (224, 224)), 0, 255).astype(np.uint8)
    frames = np.stack([np.stack([noisy[k], noisy[k][::-1], noisy[k][:, ::-1]]) for k in range(10)])
    hm = torch.from_numpy(rng.integers(0, 256, (30, 14, 14), dtype=np.uint8)).cuda()
    ov = H.heatmap_overlay(hm, torch.from_numpy(np.ascontiguousarray(frames)).cuda(), [k % 10 for k in range(30)],
                           H.jet_lut(torch.device("cuda")))
    return {"gaze_maps": maps, "noisy_grey": torch.from_numpy(noisy).cuda(), "overlays": ov}


def kernel_rows(name, x, reps):
    import torch
    from egaze_amd import hipops as H
    from egaze_amd._lib import LIB
    N, Hh, W = x.shape[:3]
    C = 3 if x.dim() == 4 else 1
    nb = LIB.egz_jpeg_encode_ws_bytes(N, Hh, W, C)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    need = torch.zeros(N, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for stages, label in STAGES.items():
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            H.check(LIB.egz_jpeg_encode(x.data_ptr(), N, Hh, W, C, 95, 420, ws.data_ptr(), nb, need.data_ptr(), stages, stream))
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        print(json.dumps({"item": "kernel_stages", "input": name, "images": N, "upto": label,
                          "ms": round(float(np.median(ts[1:])), 4)}), flush=True)
    del ws
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data, off, st = H.jpeg_encode(x, quality=95)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    assert int(st.abs().sum()) == 0
    t = float(np.median(ts[1:]))
    print(json.dumps({"item": "kernel_whole_call", "input": name, "images": N, "ms": round(t * 1e3, 4),
                      "images_per_s": round(N / t), "output_MB": round(data.numel() / 1e6, 3),
                      "workspace_MB": round(nb / 1e6, 1)}), flush=True)


def _pil_encode(arrs):
    from PIL import Image
    n = 0
    for a in arrs:
        b = io.BytesIO()
        Image.fromarray(a[:, :, ::-1] if a.ndim == 3 else a).save(b, format="JPEG", quality=95)
        n += len(b.getvalue())
    return n


def host_rows(name, arrs, reps):
    for procs in (1, 16):
        chunks = [arrs[i::procs] for i in range(procs)]
        ts = []
        if procs == 1:
            for _ in range(reps):
                t0 = time.perf_counter()
                _pil_encode(arrs)
                ts.append(time.perf_counter() - t0)
        else:
            with ProcessPoolExecutor(procs, mp_context=multiprocessing.get_context("spawn")) as ex:   # no GPU handle in the children
                list(ex.map(_pil_encode, chunks))          # warm the workers
                for _ in range(reps):
                    t0 = time.perf_counter()
                    list(ex.map(_pil_encode, chunks))
                    ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        print(json.dumps({"item": "host_pillow", "input": name, "procs": procs, "images": len(arrs), "ms": round(t * 1e3, 3),
                          "images_per_s": round(len(arrs) / t)}), flush=True)


def cli_rows(frames, workers, rounds=3):
    from PIL import Image
    from egaze_amd.data import dataset_preprocessing as D
    rs = np.random.RandomState(0)
    per_video = 1000
    nv = max(1, frames // per_video)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "gaze"))
        b = io.BytesIO()
        Image.fromarray(rs.randint(0, 256, (224, 224, 3)).astype(np.uint8)).save(b, format="JPEG", quality=90)
        for v in range(nv):
            video = f"Synth{v}_Recipe"
            d = os.path.join(tmp, "flow", video)
            os.makedirs(d)
            lines = []
            for n in range(per_video + 1):
                lines.append(f"0\tSMP\t1\t{rs.uniform(0, 1279):.2f}\t{rs.uniform(0, 959):.2f}\t{n}\t"
                             f"{'Fixation' if rs.rand() < 0.7 else 'Saccade'}\n")
                with open(os.path.join(d, f"img_{n + 1:05d}.jpg"), "wb") as fh:
                    fh.write(b.getvalue())
            with open(os.path.join(tmp, "gaze", video + "_gaze.txt"), "w") as fh:
                fh.write("".join(lines))
        split = {}
        orig_r, orig_e = D.render_maps, D.encode_maps_gpu

        def timed(key, fn):
            def f(*a, **k):
                import torch
                t0 = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                split[key] = split.get(key, 0.0) + time.perf_counter() - t0
                return out
            return f
        D.render_maps, D.encode_maps_gpu = timed("render_s", orig_r), timed("encode_readback_s", orig_e)
        try:
            base = ["--gazePath", os.path.join(tmp, "gaze"), "--flowPath", os.path.join(tmp, "flow"), "--workers", str(workers)]
            k = 0
            for r in range(rounds + 1):                    # round 0 warms both paths
                for flag in ((), ("--gpu-encode",)):
                    k += 1
                    out = [x for kv in (("--imagePath", f"img{k}"), ("--gtPath", f"gt{k}"), ("--fixsacPath", f"fs{k}"))
                           for x in (kv[0], os.path.join(tmp, kv[1]))]
                    split.clear()
                    t0 = time.perf_counter()
                    D.main(base + out + list(flag))
                    total = time.perf_counter() - t0
                    assert len(os.listdir(os.path.join(tmp, f"gt{k}"))) == nv * per_video
                    if r:
                        print(json.dumps({"item": "cli_dataset_preprocessing", "gpu_encode": bool(flag), "round": r,
                                          "frames": nv * per_video, "videos": nv, "workers": workers, "s": round(total, 3),
                                          "frames_per_s": round(nv * per_video / total),
                                          **{kk: round(vv, 3) for kk, vv in split.items()}}), flush=True)
        finally:
            D.render_maps, D.encode_maps_gpu = orig_r, orig_e


def vis_rows(ov, reps, workers=8):
    """30 overlays on the device -> 30 .jpg files: read-back + Pillow in a thread pool, against device encode + byte writes."""
    import torch
    from egaze_amd import hipops as H
    from egaze_amd.data._io import imwrite_bgr
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(workers) as pool:
        for mode in ("host_encode", "gpu_encode"):
            ts = []
            for _ in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "host_encode":
                    arr = ov.cpu().numpy()
                    list(pool.map(lambda i: imwrite_bgr(os.path.join(tmp, f"h{i}.jpg"), arr[i]), range(len(arr))))
                else:
                    data, off, _ = H.jpeg_encode(ov, quality=95)
                    buf, o = data.cpu().numpy(), off.cpu().tolist()

                    def put(i):
                        with open(os.path.join(tmp, f"g{i}.jpg"), "wb") as fh:
                            fh.write(buf[o[i]:o[i + 1]])
                    list(pool.map(put, range(len(o) - 1)))
                ts.append(time.perf_counter() - t0)
            print(json.dumps({"item": "vis_batch_to_files", "mode": mode, "overlays": int(ov.shape[0]), "writer_threads": workers,
                              "ms": round(float(np.median(ts[1:])) * 1e3, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    import egaze_amd  # noqa: F401
    xs = inputs()
    for name, x in xs.items():
        kernel_rows(name, x, a.reps)
    for name, x in xs.items():
        host_rows(name, list(x.cpu().numpy()), max(5, a.reps))
    vis_rows(xs["overlays"], a.reps)
    if not a.skip_cli:
        cli_rows(a.frames, a.workers)


if __name__ == "__main__":
    main()
