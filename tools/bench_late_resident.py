"""The resident late-fusion dataset (data/late_resident.py, --late_resident) measured; one JSON line per item, also written to
--out (default profiles/late_resident.txt):
  gather      egz_late_gather alone at B = 32 and 64, 224 x 224, from the filled training pool (larger than the Infinity Cache),
              a different random idx per launch: device time of --reps back-to-back launches over their number, alternating
              between the two batch sizes; TB/s of the counted bytes (3 planes read + 3 fp32 planes written per sample)
  gather_call the whole hipops.late_gather call (status zero fill, kernel, status copy), device time per call
  fill        ResidentLateDataset.fill of the training split with both decoders, alternating, files/s
  lf_epoch    LF.trainLate on a synthetic tree of --frames grey JPEG triples at batch --batch: through the file loader
              (resident=False: the parent commit's path), through the resident set, and tools/bench_lf.py's synthetic-input
              iteration (LF.GraphedLateIteration on tensors already on the device) run as an epoch of the same length --
              alternating, --rounds times.  ms_per_iter = the epoch's wall time (ends in a device synchronise; includes the
              two eager steps and the graph capture every epoch starts with) over its iterations; steady_ms_per_iter = the time
              from the drain after iteration 32 (the device is idle there) to the end over the iterations in between.
Usage: python tools/bench_late_resident.py [--frames 8192] [--batch 32] [--rounds 3] [--reps 200] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = []
H = W = 224
SETTLED = 32                # iterations after which an epoch is taken as steady (two drains of GraphedLateIteration.RING)


def emit(rec):
    OUT.append(json.dumps(rec))
    print(OUT[-1], flush=True)


def write_tree(root, frames, val, distinct=32, seed=0):
    """pred / feat / gt folders of grey baseline JPEGs (Pillow), ``frames`` training and ``val`` validation names; the pixel
    content cycles through ``distinct`` smooth maps per folder (every name is its own file).  -> (pred, feat, gt)."""
    import io
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)

    def blobs(n):
        m = np.zeros((H, W), np.float32)
        for _ in range(n):
            cy, cx, s = rs.uniform(20, H - 20), rs.uniform(20, W - 20), rs.uniform(10, 40)
            m += rs.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        return (255 * m / m.max()).astype(np.uint8)
    names = [f"Ahmad_American_frame_{i:06d}.jpg" for i in range(frames)] + [f"Alireza_American_frame_{i:06d}.jpg" for i in range(val)]
    folders = tuple(os.path.join(root, d) for d in ("pred", "feat", "gt"))
    for k, folder in enumerate(folders):
        os.makedirs(folder)
        enc = []
        for _ in range(distinct):
            buf = io.BytesIO()
            Image.fromarray(blobs(1 if k == 2 else 4)).save(buf, format="JPEG")
            enc.append(buf.getvalue())
        for i, name in enumerate(names):
            with open(os.path.join(folder, name), "wb") as f:
                f.write(enc[i % distinct])
    return folders


class _Timed:
    """A DataLoader stand-in that stamps the host time at which each batch is fetched."""
    def __init__(self, loader):
        self.loader, self.stamps = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            self.stamps.append(time.perf_counter())
            yield b


def gather_alone(pool, table, reps, rounds):
    import torch
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    dev = pool.device
    P, N = pool.shape[0], table.shape[0]
    g = torch.Generator().manual_seed(1)
    res = {32: [], 64: []}
    call = {32: [], 64: []}
    bufs = {}
    for B in res:
        bufs[B] = (torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(16)]).to(dev),
                   torch.empty((B, 2, H, W), dtype=torch.float32, device=dev),
                   torch.empty((B, 1, H, W), dtype=torch.float32, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def launches(B, n):
        idx, fused, gt = bufs[B]
        for r in range(n):
            check(Hp.LIB.egz_late_gather(pool.data_ptr(), P, table.data_ptr(), N, idx[r % 16].data_ptr(), B, H, W,
                                         fused.data_ptr(), gt.data_ptr(), None, status.data_ptr(), Hp._stream()),
                  "egz_late_gather")
    for rnd in range(rounds + 1):                                  # round 0 warms up
        for B in res:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launches(B, reps)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[B].append(e0.elapsed_time(e1) / reps)
            idx = bufs[B][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in range(reps):
                Hp.late_gather(pool, table, idx[r % 16], status_to={})
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                call[B].append(e0.elapsed_time(e1) / reps)
    assert int(status.item()) == 0
    for B in res:
        nbytes = B * H * W * (3 + 3 * 4)
        us = float(np.median(res[B])) * 1e3
        emit({"item": "gather", "B": B, "hw": [H, W], "launches_per_window": reps, "windows": rounds, "pool_bytes": pool.numel(),
              "median_us": us, "min_us": float(np.min(res[B])) * 1e3, "max_us": float(np.max(res[B])) * 1e3,
              "counted_bytes": nbytes, "TB_per_s": nbytes / us / 1e6})
        emit({"item": "gather_call", "B": B, "median_us": float(np.median(call[B])) * 1e3,
              "min_us": float(np.min(call[B])) * 1e3, "max_us": float(np.max(call[B])) * 1e3})


def fill_rates(args):
    import torch
    from egaze_amd.data.late_resident import ResidentLateDataset
    ds = None
    for decode in ("host", "gpu", "host", "gpu"):                  # alternating; the first pair also warms the page cache
        del ds
        ds = ResidentLateDataset(*args, decode=decode)
        torch.cuda.synchronize()
        ds.fill("cuda:0")
        emit({"item": "fill", "decode": decode, "frames": len(ds), "files": len(ds.files), "pool_bytes": ds.needed_bytes,
              "seconds": ds.fill_seconds, "files_per_s": len(ds.files) / ds.fill_seconds})
    return ds


def _steady(stamps, t_end, n_iter):
    # batch SETTLED + 1 is fetched right after the drain that follows iteration SETTLED - 1: iterations SETTLED .. n - 1 remain
    return (t_end - stamps[SETTLED + 1]) / (n_iter - SETTLED) * 1e3 if n_iter > 2 * SETTLED else None


def lf_epochs(folders, save, batch, rounds):
    import torch
    from egaze_amd.LF import LF, GraphedLateIteration
    dev = torch.device("cuda:0")
    lfs = {}
    for mode in ("file_loader", "resident"):
        torch.manual_seed(0)
        lfs[mode] = LF(save_path=save, device="0", late_pred_path=folders[0], late_feat_path=folders[1], gt_path=folders[2],
                       val_name="Alireza", batch_size=batch, lr=1e-4, resident=mode == "resident", decode="gpu")
    n_iter = len(lfs["resident"].train_loader)
    torch.manual_seed(0)
    syn = LF(save_path=save, device="0", late_pred_path=folders[0], late_feat_path=folders[1], gt_path=folders[2],
             val_name="Alireza", batch_size=batch, lr=1e-4)                       # its model, criterion and optimizer only
    feat, im, gt = (torch.rand(batch, 1, H, W, device=dev) for _ in range(3))

    def loader_epoch(lf):
        timed = _Timed(lf.train_loader)
        keep, lf.train_loader = lf.train_loader, timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lf.trainLate()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lf.train_loader = keep
        return t1 - t0, _steady(timed.stamps, t1, n_iter)

    def synthetic_epoch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = GraphedLateIteration(syn.model, syn.criterion, syn.optimizer, (feat, im, gt))
        t_settled = None
        for i in range(n_iter):
            it(feat, im, gt)
            if it.full:
                it.drain()
                if i == SETTLED - 1:
                    t_settled = time.perf_counter()
        it.drain()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        it.close()
        return t1 - t0, (t1 - t_settled) / (n_iter - SETTLED) * 1e3 if t_settled and n_iter > 2 * SETTLED else None
    for rnd in range(rounds + 1):                                  # round 0 warms up: allocations, packings, page cache
        for mode in ("file_loader", "resident", "synthetic"):
            sec, steady = synthetic_epoch() if mode == "synthetic" else loader_epoch(lfs[mode])
            if rnd:
                emit({"item": "lf_epoch", "mode": mode, "round": rnd, "B": batch, "iterations": n_iter,
                      "ms_per_iter": sec / n_iter * 1e3, "steady_ms_per_iter": steady,
                      "frames_per_s": batch * n_iter / sec})
    return lfs["resident"].train_loader.dataset


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=8192)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_resident.txt"))
    a = p.parse_args()
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_late_resident: needs the GPU (no timing is taken on a CPU)")
    from egaze_amd.LF import _split
    emit({"item": "device", "name": torch.cuda.get_device_name(0)})
    with tempfile.TemporaryDirectory() as root:
        folders = write_tree(os.path.join(root, "tree"), a.frames, a.batch)
        pred, feat, gt = folders
        args = (pred, gt, feat, _split(pred, "Alireza", None)[0], _split(gt, "Alireza", None)[0], _split(feat, "Alireza", None)[0])
        ds = fill_rates(args)
        gather_alone(ds.pool, ds.table, a.reps, a.rounds)
        del ds
        os.makedirs(os.path.join(root, "save"))
        lf_epochs(folders, os.path.join(root, "save"), a.batch, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
