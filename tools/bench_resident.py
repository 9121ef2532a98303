"""The resident dataset (data/resident.py, --gpu_resident) measured; one JSON line per item, also written to --out
(default profiles/resident_frames.txt):
  gather      egz_resident_gather at B = 32, 224 x 224 against the launches it replaces on bytes already on the device (three
              egz_u8_normalize, egz_nchw_to_nhwc_pad, egz_absmax), alternating, median device time; GB/s of the counted traffic
  fill        ResidentSTDataset.fill per 1,000 frames with both decoders, and the pool's bytes for the tree used
  e2e         SP.trainSP steady-state step (tools/bench_jpeg.py's protocol and tree: median interval over --batches steps, files
              in the page cache) at B = 8 and 32: host decode with one worker, --gpu_decode, --gpu_resident
  issue       per batch of the resident path: host time to issue the staging (index copy + gather launch + NHWC-32 hand-over),
              device time of the gather
Usage: python tools/bench_resident.py [--reps 30] [--batches 24] [--out FILE] [--no-e2e]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = []


def emit(rec):
    OUT.append(json.dumps(rec))
    print(OUT[-1], flush=True)


def gather_vs_replaced(reps, B=32, H=224, W=224):
    import torch
    from egaze_amd import hipops as Hp
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    dev = torch.device("cuda:0")
    frames = 256                                                   # 6 planes per frame, as the real pool
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (frames * 6, H, W), dtype=torch.uint8, generator=g).to(dev)
    n = frames - 9
    t = torch.arange(9, frames)
    table = torch.empty((n, 22), dtype=torch.int64)
    table[:, 0] = 3 * t
    for m in range(10):
        table[:, 1 + 2 * m] = 3 * frames + 2 * (t - m)
        table[:, 2 + 2 * m] = 3 * frames + 2 * (t - m) + 1
    table[:, 21] = 5 * frames + t
    table = table.to(dev)
    idx = torch.randperm(n, generator=g)[:B].to(dev)
    raw = Hp.resident_gather(pool, table, idx, raw=True)
    u8 = [raw[:, :3].contiguous(), raw[:, 3:23].contiguous(), raw[:, 23:].contiguous()]

    def new():
        return Hp.resident_gather(pool, table, idx, status_to={})

    def old():
        im = Hp.u8_normalize(u8[0], IMAGE_MEAN, IMAGE_STD)
        fl = Hp.u8_normalize(u8[1], FLOW_MEAN, FLOW_STD)
        gt = Hp.u8_normalize(u8[2], (0.0,), (1.0,))
        Hp.prepare_network_input(fl)
        return im, fl, gt
    a, b = new(), old()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[1]._egz_prepared[0], b[1]._egz_prepared[0])
    ts = {"new": [], "old": []}
    for r in range(reps + 5):
        for name, fn in (("new", new), ("old", old)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 5:
                ts[name].append(e0.elapsed_time(e1))
    HW = H * W
    new_bytes = B * HW * (24 + 24 * 4 + 32 * 4)
    old_bytes = B * HW * (24 + 24 * 4) + B * HW * (20 * 4 + 32 * 4) + B * HW * 32 * 4
    for name, nbytes in (("new", new_bytes), ("old", old_bytes)):
        ms = float(np.median(ts[name]))
        emit({"item": "gather" if name == "new" else "replaced_launches", "B": B, "hw": [H, W], "calls": reps,
              "median_ms": ms, "min_ms": float(np.min(ts[name])), "max_ms": float(np.max(ts[name])),
              "counted_bytes": nbytes, "GB_per_s": nbytes / ms / 1e6, "bit_identical": bool(same)})
    return float(np.median(ts["new"]))


def fill_rates(args, frames):
    import torch
    from egaze_amd.data.resident import ResidentSTDataset
    for decode in ("host", "gpu", "host", "gpu"):                  # alternating; the first pair also warms the page cache
        ds = ResidentSTDataset(*args, raw_u8=True, decode=decode)
        torch.cuda.synchronize()
        ds.fill("cuda:0")
        emit({"item": "fill", "decode": decode, "frames": frames, "files": len(ds.files), "pool_bytes": ds.needed_bytes,
              "seconds": ds.fill_seconds, "seconds_per_1000_frames": ds.fill_seconds / frames * 1000})
        del ds


def e2e(batches):
    import torch
    import bench_jpeg as J
    from torch.utils.data import DataLoader
    from egaze_amd.SP import SP
    from egaze_amd.data.STdatas import STDataset, check_decode_status, stage_batch
    from egaze_amd.data.resident import ResidentSTDataset
    streams = J.make_streams()
    with tempfile.TemporaryDirectory() as root:
        J.fake_vgg(os.path.join(root, "vgg.pth"))
        os.environ["EGAZE_VGG16_BN"] = os.path.join(root, "vgg.pth")
        for B in (8, 32):
            args = J.write_tree(os.path.join(root, f"tree{B}"), streams, B * batches)
            if B == 32:
                fill_rates(args, B * batches)
            for mode in ("host", "gpu_decode", "resident", "host", "gpu_decode", "resident"):
                if mode == "resident":
                    ds = ResidentSTDataset(*args, raw_u8=True, decode="gpu").fill("cuda:0")
                else:
                    ds = STDataset(*args, raw_u8=True, decode="gpu" if mode == "gpu_decode" else "host")
                torch.manual_seed(0)
                sp = SP(lr=1e-4, save_path=os.path.join(root, "save"), batch_size=B, device="0", resume="0",
                        traindata=ds, valdata=ds)
                sp.trainSP()                                       # warm: allocations, packings, page cache
                timed = J._Timed(sp.STTrainLoader)
                sp.STTrainLoader = timed
                sp.trainSP()
                torch.cuda.synchronize()
                d = np.diff(timed.stamps)[2:]
                emit({"item": "e2e_trainSP", "B": B, "mode": mode, "workers": sp.STTrainLoader.loader.num_workers,
                      "steps": batches, "ms_per_step": float(np.median(d)) * 1e3, "min_ms": float(d.min()) * 1e3,
                      "max_ms": float(d.max()) * 1e3, "frames_per_s": B / float(np.median(d))})
                del sp
                if mode == "resident":
                    host, devt = [], []
                    for b in DataLoader(ds, batch_size=B, shuffle=True, num_workers=0, pin_memory=True, collate_fn=ds.collate_fn):
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        e0.record()
                        stage_batch(b, torch.device("cuda:0"))
                        e1.record()
                        host.append(time.perf_counter() - t0)
                        check_decode_status(b)
                        torch.cuda.synchronize()
                        devt.append(e0.elapsed_time(e1))
                    emit({"item": "issue", "B": B, "host_ms_per_batch": float(np.median(host[2:])) * 1e3,
                          "device_ms_index_copy_and_gather": float(np.median(devt[2:]))})
                del ds


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--batches", type=int, default=24)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_frames.txt"))
    p.add_argument("--no-e2e", action="store_true")
    a = p.parse_args()
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident: needs the GPU (no timing is taken on a CPU)")
    emit({"item": "device", "name": torch.cuda.get_device_name(0)})
    gather_vs_replaced(a.reps)
    if not a.no_e2e:
        e2e(a.batches)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
