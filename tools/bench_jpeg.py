"""GPU JPEG decode (hipops.jpeg_decode) against Pillow on the host, for the batch-32 input mix of SP training: 32 colour 4:2:0
frames and 672 grayscale frames (20 flow + 1 ground truth per sample) at 224 x 224, quality 95.  One JSON line per item:
  kernel      images/s of the whole decode, and of the entropy stage alone (device events, median of 5)
  host        Pillow decode of the same streams on 1 and on 16 processes
  e2e         SP.trainSP frames/s over an on-disk tree of those streams (temp directory) at B = 8 and 32: host decode with the
              reference's one loader worker, host decode with --workers workers, --gpu_decode (one worker); and the main
              process's host time to issue the staging of one gpu-mode batch (stage_batch: H2D copy, decode, normalise)
Usage: python tools/bench_jpeg.py [--procs 16] [--reps 5] [--workers 8] [--batches 24]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_streams(seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:224, 0:224]
    out = []
    for i in range(704):
        base = 128 + 80 * np.sin(x * rng.uniform(0.02, 0.1) + rng.uniform(0, 6)) * np.cos(y * rng.uniform(0.02, 0.1))
        if i < 32:
            im = np.stack([base, base[::-1], base[:, ::-1]], -1) + rng.normal(0, 8, (224, 224, 3))
            pil = Image.fromarray(np.clip(im, 0, 255).astype(np.uint8))
            kw = dict(subsampling=2)
        else:
            pil = Image.fromarray(np.clip(base + rng.normal(0, 8, (224, 224)), 0, 255).astype(np.uint8))
            kw = {}
        b = io.BytesIO()
        pil.save(b, format="JPEG", quality=95, **kw)
        out.append((b.getvalue(), 3 if i < 32 else 1))
    return out


def _pil_decode(items):
    from PIL import Image
    for data, c in items:
        im = Image.open(io.BytesIO(data))
        np.asarray(im.convert("RGB") if c == 3 else im)
    return len(items)


def host_rate(streams, procs, reps):
    chunks = [streams[i::procs] for i in range(procs)]
    ts = []
    if procs == 1:
        for _ in range(reps):
            t0 = time.perf_counter()
            _pil_decode(streams)
            ts.append(time.perf_counter() - t0)
    else:
        with ProcessPoolExecutor(procs) as ex:
            list(ex.map(_pil_decode, chunks))                      # warm the workers
            for _ in range(reps):
                t0 = time.perf_counter()
                list(ex.map(_pil_decode, chunks))
                ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    return {"item": "host_pillow", "procs": procs, "images": len(streams), "ms": t * 1e3, "images_per_s": len(streams) / t}


def kernel_rate(streams, reps):
    import torch
    import egaze_amd  # noqa: F401
    from egaze_amd import hipops as H
    data = torch.from_numpy(np.frombuffer(b"".join(s for s, _ in streams), np.uint8).copy()).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s, _ in streams])]), dtype=torch.int64).cuda()
    ch = torch.tensor([c for _, c in streams], dtype=torch.int32).cuda()
    n3 = sum(c == 3 for _, c in streams)
    out = torch.empty((len(streams), 3, 224, 224), dtype=torch.uint8, device="cuda")
    res = []
    for stages, name in ((2, "full"), (1, "entropy")):
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, st = H.jpeg_decode(data, off, (224, 224), ch, out=out, n3=n3, stages=stages)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        assert int(st.abs().sum()) == 0
        t = float(np.median(ts[1:]))
        res.append({"item": f"kernel_{name}", "images": len(streams), "ms": t, "images_per_s": len(streams) / t * 1e3,
                    "bytes": int(data.numel())})
    res.append({"item": "kernel_idct_colour", "ms": res[0]["ms"] - res[1]["ms"]})
    return res


def write_tree(root, streams, n):
    """n samples (frames 10 .. n + 9) of 224 x 224 files: colour 4:2:0 frames, grayscale flow and ground truth, cycled from
    the benchmark streams.  -> STDataset positional arguments."""
    folder = "Ahmad_American"
    col = [s for s, c in streams if c == 3]
    gray = [s for s, c in streams if c == 1]
    for d in ("flow/" + folder, "img", "gt", "fs"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    k = 0
    for f in range(1, n + 10):
        for ax in "xy":
            with open(os.path.join(root, "flow", folder, f"flow_{ax}_{f:05d}.jpg"), "wb") as fh:
                fh.write(gray[k % len(gray)])
            k += 1
    names, gts = [], []
    for i, f in enumerate(range(10, n + 10)):
        names.append(f"{folder}_img_{f:05d}.jpg")
        gts.append(f"{folder}_000000_{f:05d}.jpg")
        with open(os.path.join(root, "img", names[-1]), "wb") as fh:
            fh.write(col[i % len(col)])
        with open(os.path.join(root, "gt", gts[-1]), "wb") as fh:
            fh.write(gray[(k + i) % len(gray)])
    np.savetxt(os.path.join(root, "fs", "a.txt"), np.zeros(n))
    return (os.path.join(root, "flow"), os.path.join(root, "img"), os.path.join(root, "gt"), [folder], names, gts, ["a.txt"],
            os.path.join(root, "fs"))


def fake_vgg(path):
    """A VGG16-BN state dict of the right shapes (SP(resume='0') loads it into both encoders: every layer is trained)."""
    import torch
    from egaze_amd.utils import make_layers, cfg
    torch.manual_seed(3)
    sd = {"features." + k: (v.clone().normal_(0, 0.05) if v.is_floating_point() else v.clone())
          for k, v in make_layers(cfg["D"], 3).state_dict().items()}
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = sd[k].abs() + 0.5
    sd["classifier.0.weight"] = torch.zeros(4, 4)
    torch.save(sd, path)


class _Timed:
    """A DataLoader stand-in that stamps the host time at which each batch is handed on."""
    def __init__(self, loader):
        self.loader, self.stamps = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            self.stamps.append(time.perf_counter())
            yield b


def e2e(streams, workers, batches):
    import tempfile
    import torch
    from torch.utils.data import DataLoader
    import egaze_amd  # noqa: F401
    from egaze_amd.SP import SP
    from egaze_amd.data.STdatas import STDataset, stage_batch, check_decode_status
    res = []
    with tempfile.TemporaryDirectory() as root:
        fake_vgg(os.path.join(root, "vgg.pth"))
        os.environ["EGAZE_VGG16_BN"] = os.path.join(root, "vgg.pth")
        for B in (8, 32):
            args = write_tree(os.path.join(root, f"tree{B}"), streams, B * batches)
            for decode, nw in (("host", 1), ("host", workers), ("gpu", 1)):
                ds = STDataset(*args, raw_u8=True, decode=decode)
                torch.manual_seed(0)
                sp = SP(lr=1e-4, save_path=os.path.join(root, "save"), batch_size=B, device="0", resume="0",
                        traindata=ds, valdata=ds)
                if nw != 1:
                    sp.STTrainLoader = DataLoader(ds, batch_size=B, shuffle=True, num_workers=nw, pin_memory=True,
                                                  collate_fn=ds.collate_fn)
                sp.trainSP()                                       # warm: allocations, packings
                timed = _Timed(sp.STTrainLoader)
                sp.STTrainLoader = timed
                sp.trainSP()
                torch.cuda.synchronize()
                # steady state: the interval between two batches handed to the step (each step reads its loss back, so
                # the host cannot run ahead), the first two intervals -- worker start, first prefetch -- left out
                dt = float(np.median(np.diff(timed.stamps)[2:]))
                res.append({"item": "e2e_trainSP", "B": B, "decode": decode, "workers": nw, "steps": batches,
                            "ms_per_step": dt * 1e3, "frames_per_s": B / dt,
                            "epoch_s_incl_worker_start": timed.stamps[-1] - timed.stamps[0]})
                print(json.dumps(res[-1]), flush=True)
                del sp
            ds = STDataset(*args, raw_u8=True, decode="gpu")
            ts = []
            for b in DataLoader(ds, batch_size=B, num_workers=1, pin_memory=True, collate_fn=ds.collate_fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stage_batch(b, torch.device("cuda:0"))
                ts.append(time.perf_counter() - t0)
                check_decode_status(b)
            res.append({"item": "gpu_decode_issue", "B": B, "host_ms_per_batch": float(np.median(ts)) * 1e3})
            print(json.dumps(res[-1]), flush=True)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--procs", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--workers", type=int, default=8)
    p.add_argument("--batches", type=int, default=24)
    p.add_argument("--no-e2e", action="store_true")
    p.add_argument("--only-e2e", action="store_true")
    a = p.parse_args()
    streams = make_streams()
    if not a.only_e2e:
        for r in kernel_rate(streams, a.reps):
            print(json.dumps(r), flush=True)
        for procs in (1, a.procs):
            print(json.dumps(host_rate(streams, procs, a.reps)), flush=True)
    if not a.no_e2e:
        e2e(streams, a.workers, a.batches)


if __name__ == "__main__":
    main()
