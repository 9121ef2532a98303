"""AT.trainLSTM / AT.testLSTM per sample (B = 1, T = 1) through the three ways the loop can be fed, in one process:
  files     data.LSTMdatas.lstmDataset behind the driver's own batch-1 DataLoader, on N synthetic fix_*.pth.tar files written to a
            temporary 512w folder (a video break every --video files); the page cache is warm (a warm-up epoch read every file)
  resident  data.lstm_resident.ResidentLSTMDataset filled from the same folder (--lstm_resident): hipops.lstm_pool_fetch at the head
            of the step's hipGraph
  hostlist  the loop of tools/bench_at_loop.py: a Python list of sample dicts already in host memory
The three forms alternate over --reps repetitions after one warm-up epoch each; every timed window ends in a device
synchronise; per form the median and the spread (max - min) over the repetitions are printed, and the fill time.
Usage: python tools/bench_lstm_resident.py [--n 20000] [--video 300] [--reps 3] > profiles/lstm_resident.txt"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import egaze_amd  # noqa: F401,E402
import egaze_amd.AT as at_mod  # noqa: E402
from egaze_amd.data.LSTMdatas import lstmDataset  # noqa: E402
from egaze_amd.data.lstm_resident import ResidentLSTMDataset  # noqa: E402
from egaze_amd.functions import MSELoss  # noqa: E402
from egaze_amd.models.LSTMnet import lstmnet  # noqa: E402
from egaze_amd.optim import FusedAdam  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--video", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    lstm = lstmnet().to(dev)
    at = at_mod.AT.__new__(at_mod.AT)            # the constructor wants an SP checkpoint
    at.lstm, at.criterion_lstm, at.device = lstm, MSELoss.apply, dev
    at.optimizer_lstm = FusedAdam(lstm.parameters(), lr=1e-4)

    with tempfile.TemporaryDirectory() as root:
        folder = os.path.join(root, "512w", "train")
        os.makedirs(folder)
        g = torch.Generator().manual_seed(5)
        t0 = time.perf_counter()
        for i in range(args.n):
            torch.save(torch.rand(512, generator=g), os.path.join(folder, f"fix_video{i // args.video:04d}_{i % args.video:010d}.pth.tar"))
        print(f"# {args.n} vectors of 512 floats written in {time.perf_counter() - t0:.1f} s, {-(-args.n // args.video)} videos of "
              f"{args.video} files; per-sample times are epoch time / (N - 2) scored samples; AT_GRAPH = {at_mod.AT_GRAPH}")
        files = lstmDataset(folder)
        loader = lambda ds: DataLoader(dataset=ds, batch_size=1, shuffle=False, num_workers=0)
        resident = ResidentLSTMDataset(folder)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident.fill(dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"fill: {dt:.2f} s for {args.n} files ({args.n / dt:.0f} files/s, {resident.needed_bytes / 1e6:.1f} MB on the device), "
              f"page cache warm from the writes")
        hostlist = [files[i] for i in range(len(files))]
        hostlist = [{"input": s["input"].view(1, -1), "gt": s["gt"].view(1, -1), "same": torch.tensor([int(s["same"])])}
                    for s in hostlist]
        forms = (("files", loader(files)), ("resident", loader(resident)), ("hostlist", hostlist))
        scored = args.n - 2

        def epoch(feed, train):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if train:
                at.lstm.train()
                loss = at._epoch(feed, True)
            else:
                at.lstm.eval()
                with torch.no_grad():
                    loss = at._epoch(feed, False)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / scored * 1e6, loss

        times = {(name, train): [] for name, _ in forms for train in (True, False)}
        for rep in range(args.reps + 1):                  # repetition 0 warms up and is not counted
            for name, feed in forms:
                for train in (True, False):
                    us, loss = epoch(feed, train)
                    if rep:
                        times[(name, train)].append(us)
                    print(f"# rep {rep} {name:8s} {'train' if train else 'eval ':5s} {us:8.1f} us per sample, mean loss {loss:.6f}"
                          f"{'  (warm-up)' if not rep else ''}")
        for train in (True, False):
            for name, _ in forms:
                t = times[(name, train)]
                print(f"{'trainLSTM' if train else 'testLSTM '} {name:8s}: median {statistics.median(t):7.1f} us per sample, "
                      f"spread {max(t) - min(t):5.1f} us over {len(t)} repetitions ({', '.join(f'{v:.1f}' for v in t)})")
        resident.release()


if __name__ == "__main__":
    main()
