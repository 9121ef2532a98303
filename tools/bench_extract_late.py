"""AT.extract_late per frame on one GPU, through a DataLoader over frames held in memory (the form gaze_full hands it), with the
PNG writes and the resize replaced by no-ops as in tools/bench_pipeline.py.  One process times ONE variant -- ``--shard none`` (the
one-rank path) or ``--shard 0,1`` (the sharded code path at world size 1: owned loader, windows, gather of one) -- so that variants
and commits can be alternated run by run (profiles/extract_late_sharded.txt).  Prints one line per pass and the median.
Usage: python tools/bench_extract_late.py [--shard none|0,1] [--frames 128] [--chunk 32] [--passes 5]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egaze_amd  # noqa
import egaze_amd.AT as at_mod
from egaze_amd.AT import AT
from egaze_amd.models.model_SP import model_SP
from egaze_amd.utils import cfg, make_layers

ap = argparse.ArgumentParser()
ap.add_argument("--shard", default="none")
ap.add_argument("--frames", type=int, default=128)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--passes", type=int, default=5)
a = ap.parse_args()
kw = {} if a.shard == "none" else {"shard": tuple(int(v) for v in a.shard.split(","))}


class Frames(Dataset):
    """uint8 frames as STDataset(raw_u8=True) yields them."""

    def __init__(self, n):
        rs = np.random.RandomState(1)
        self.image = torch.from_numpy(rs.randint(0, 256, (n, 3, 224, 224)).astype(np.uint8))
        self.flow = torch.from_numpy(rs.randint(0, 256, (n, 20, 224, 224)).astype(np.uint8))
        self.gt = torch.from_numpy(rs.randint(0, 256, (n, 1, 224, 224)).astype(np.uint8))
        self.fixsac = (np.random.RandomState(0).rand(n) < 0.746).astype(float)

    def __len__(self):
        return len(self.fixsac)

    def __getitem__(self, i):
        return {"image": self.image[i], "flow": self.flow[i], "gt": self.gt[i],
                "fixsac": torch.FloatTensor([self.fixsac[i]]), "imname": "f%05d.png" % i}


torch.manual_seed(0)
with tempfile.TemporaryDirectory() as d:
    sp = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    torch.save({'state_dict': sp.state_dict()}, os.path.join(d, "sp.pth.tar"))
    for sub in ("train", "test"):
        os.makedirs(os.path.join(d, "512w", sub))
        for i in range(2):
            torch.save(torch.zeros(512), os.path.join(d, "512w", sub, f"fix_v_{i:010d}.pth.tar"))
    at = AT(pretrained_model=os.path.join(d, "sp.pth.tar"), save_path=d, device='0', lstm_data_path=os.path.join(d, "512w"))
    at_mod.imwrite = lambda path, arr: None                    # disk writes are not part of the path
    at_mod._progress = lambda it: it
    at_mod.resize = lambda arr, size: arr
    at_mod.print = lambda *args, **kwargs: None
    loader = DataLoader(Frames(a.frames), batch_size=1, shuffle=False, num_workers=0, pin_memory=True)
    at.extract_late(loader, d + "/p/", d + "/f/", chunk=a.chunk, **kw)          # warm-up: buffers, weight caches
    dts = []
    for _ in range(a.passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at.extract_late(loader, d + "/p/", d + "/f/", chunk=a.chunk, **kw)
        torch.cuda.synchronize()
        dts.append((time.perf_counter() - t0) / a.frames * 1e3)
    print("extract_late shard=%s frames=%d chunk=%d: passes ms/frame %s median %.4f" %
          (a.shard, a.frames, a.chunk, [round(v, 4) for v in dts], statistics.median(dts)))
