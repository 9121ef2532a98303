"""TV-L1 optical flow (hipops.tvl1_flow, csrc/flow_tvl1.hip) and the data/extract_flow.py chain: what a frame pair costs.

    python tools/bench_flow.py [--size 224 224] [--chunks 1 32 128] [--frames 129] [--no-host]

Prints one JSON line per measurement, all at the default parameters (5 scales asked, 5 warps, 30 iterations):
  flow     ms per pair of the whole hipops.tvl1_flow on a chunk of N pairs, for every solver form (fused = 1: one streaming
           launch per iteration; 2 / 3 / 4 / 6 / 8: overlapped tiles), device events, median of 5 calls after a warm-up.
  solver   ms per pair of the 30 inner iterations alone (hipops.tvl1_iterate without its copy: the C entry on prepared buffers),
           per form, and the bytes/s it achieves against its own traffic count: per launch 10 planes read (6 state, 4 constant)
           and 6 written, 4 N H W bytes each -- the halo re-reads of a tile are not counted, they are the price of the form.
  extract  seconds and ms per frame of `python -m egaze_amd.data.extract_flow` (in process, main()) on a temporary folder of
           --frames JPEG frames, second run of two (files in the page cache), decode to written files.
  host     seconds per pair of tests/flow_ref.py in fp32 on one host core, for scale.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = (1, 2, 3, 4, 6, 8)


def median_ms(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def frames_u8(n, hw, seed=0):
    import flow_ref as R
    base = [R.texture(*hw, shift=(0.9 * i, -0.5 * i), seed=seed) for i in range(min(n, 9))]
    return np.stack([base[i % len(base)] for i in range(n)])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, nargs=2, default=(224, 224))
    p.add_argument("--chunks", type=int, nargs="*", default=(1, 32, 128))
    p.add_argument("--frames", type=int, default=129)
    p.add_argument("--no-host", action="store_true")
    args = p.parse_args(argv)
    import torch
    from egaze_amd import _lib
    from egaze_amd import hipops as H
    from egaze_amd.data import extract_flow as X
    hw = tuple(args.size)
    dev = "cuda:0"
    print(json.dumps({"item": "config", "size": hw, "levels": H.flow_level_sizes(*hw, 5, 0.5),
                      "default_k": _lib.LIB.egz_tvl1_default_k(), "tile": 32}), flush=True)

    for n in args.chunks:
        x = torch.from_numpy(frames_u8(n + 1, hw)).to(dev)
        for k in FORMS:
            ms = median_ms(lambda: H.tvl1_flow(x, fused=k))
            print(json.dumps({"item": "flow", "pairs": n, "fused": k, "ms": round(ms, 3), "ms_per_pair": round(ms / n, 4)}),
                  flush=True)
        # the inner solver alone: 30 iterations on the finest level from a real warp
        img = H.flow_gauss(x, H.FLOW_PRESMOOTH_SIGMA)
        gx, gy = H.flow_grad(img[1:].contiguous())
        state = torch.zeros((6, n) + hw, device=dev)
        consts = H.tvl1_warp(img, gx, gy, state[:2].contiguous())
        other = torch.empty_like(state)
        for k in FORMS:
            launches = -(-30 // k)

            def run():
                _lib.check(_lib.LIB.egz_tvl1_iterate(state.data_ptr(), other.data_ptr(), consts.data_ptr(), n, hw[0], hw[1], 30,
                                                     k, 0.25, 0.15, 0.3, H._stream()))
            ms = median_ms(run)
            traffic = launches * 16 * 4 * n * hw[0] * hw[1]
            print(json.dumps({"item": "solver", "pairs": n, "fused": k, "launches": launches, "ms": round(ms, 3),
                              "ms_per_pair": round(ms / n, 4), "counted_GB": round(traffic / 1e9, 4),
                              "counted_GB_per_s": round(traffic / 1e6 / ms, 1)}), flush=True)
        del x, img, gx, gy, state, consts, other

    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "frames", "clip")
        os.makedirs(src)
        for i, f in enumerate(frames_u8(args.frames, hw, seed=1)):
            Image.fromarray(np.stack([f, f[::-1], f[:, ::-1]], -1)).save(os.path.join(src, "img_%05d.jpg" % (i + 1)), quality=95)
        for rnd in (1, 2):
            t0 = time.perf_counter()
            nfiles = X.main(["--framePath", os.path.join(tmp, "frames"), "--flowPath", os.path.join(tmp, "flow"), "--overwrite"])
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            print(json.dumps({"item": "extract", "round": rnd, "frames": args.frames, "files": nfiles, "chunk": 32,
                              "s": round(s, 3), "ms_per_frame": round(1e3 * s / args.frames, 3)}), flush=True)

    if not args.no_host:
        import flow_ref as R
        torch.set_num_threads(1)
        f = frames_u8(2, hw)
        t0 = time.perf_counter()
        R.tvl1_flow(f, np.float32)
        print(json.dumps({"item": "host", "what": "tests/flow_ref.py fp32, numpy, one core", "pairs": 1,
                          "s_per_pair": round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == "__main__":
    main()
