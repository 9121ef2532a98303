"""The SP -> AT hand-over measured both ways in one process (gaze_full --lstm_handover against the hand-over through files); one
JSON line per item, also written to --out (default profiles/lstm_handover.txt):
  files     the existing hand-over, whose code is the parent commit's, unchanged: extractLSTMw.extractw of both splits into
            fix_*.pth.tar files on local disk, then ResidentLSTMDataset.fill of both folders.  ms per extracted vector per phase,
            the files written
  memory    ResidentLSTMDataset.from_st + allocate + extractw(into=...), at chunk 1 (the file path's schedule, bit for bit) and
            at --chunk: ms per extracted vector, no file
  waits     counted in the warm-up round: the calls that make the host wait for the device (Tensor.cpu / .item / .tolist of a
            device tensor, Event.synchronize, Stream.synchronize, torch.cuda.synchronize) per extracted vector, on each path
  store     egz_lstm_store alone against egz_window_mean alone at B = 1 and B = 32, (B, 14, 14, 512) features: device time of
            --reps back-to-back launches over their number.  lstm_store also reads the 50 KB ground-truth plane of every sample
            and finds the gaze cell, which the file path does on the host
The paths alternate, --rounds times after a warm-up round; every figure is given per round so the spread shows.
The tree is synthetic: one training video of --frames frames and one validation video of --val, every fourth frame the second
frame of a fixation (one extracted vector), PNG frames and ground truth, JPEG flow, random-initialised weights.
Usage: python tools/bench_lstm_handover.py [--frames 1024] [--val 256] [--chunk 32] [--rounds 3] [--reps 200] [--out F]"""
import argparse
import contextlib
import json
import os
import shutil
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


def write_tree(root, frames, val):
    """bench_late_handover's tree with another fixation pattern: raw flags 0 1 0 0, which STDataset dilates to 1 1 1 0 -- one
    fixation of three frames in every four, so every fourth frame is extracted."""
    from bench_late_handover import TRAIN, VAL, write_tree as late_tree
    paths = late_tree(root, frames, val)
    for folder, n in ((TRAIN, frames), (VAL, val)):
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), np.array(([0, 1, 0, 0] * n)[:n], dtype=float))
    return paths


def encoder(sp_path):
    """features_s alone, as extract_LSTM_training_data builds it."""
    import torch
    from egaze_amd.utils import cfg, make_layers
    model = make_layers(cfg['D'], 3)
    sd = torch.load(sp_path, map_location='cpu', weights_only=False)['state_dict']
    own = model.state_dict()
    own.update({k[len('features_s.'):]: v for k, v in sd.items() if k.startswith('features_s.')})
    model.load_state_dict(own)
    return model.to("cuda:0").eval()


@contextlib.contextmanager
def counted_waits(counts):
    """Counts, while inside, the calls that make the host wait for the device."""
    import torch
    saved = []

    def wrap(owner, name, only_device_tensors):
        inner = getattr(owner, name)

        def counted(*a, **kw):
            if not only_device_tensors or a[0].is_cuda:
                counts[name] = counts.get(name, 0) + 1
            return inner(*a, **kw)
        saved.append((owner, name, inner))
        setattr(owner, name, counted)
    for name in ("cpu", "item", "tolist"):
        wrap(torch.Tensor, name, True)
    wrap(torch.cuda.Event, "synchronize", False)
    wrap(torch.cuda.Stream, "synchronize", False)
    wrap(torch.cuda, "synchronize", False)
    try:
        yield counts
    finally:
        for owner, name, inner in saved:
            setattr(owner, name, inner)


def files_handover(model, sets, out):
    """-> (filled sets, seconds of the extraction, seconds of the fill, files written)."""
    import torch
    from bench_late_handover import _loader
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.extractLSTMw import extractw
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for st, sub in zip(sets, ("train", "test")):
        extractw(_loader(st), model, os.path.join(out, sub), 3, "cuda:0")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    filled = [ResidentLSTMDataset(os.path.join(out, sub)).fill("cuda:0") for sub in ("train", "test")]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return filled, t1 - t0, t2 - t1, sum(len(os.listdir(os.path.join(out, sub))) for sub in ("train", "test"))


def memory_handover(model, sets, chunk):
    import torch
    from bench_late_handover import _loader
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.extractLSTMw import extractw
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    planned = [ResidentLSTMDataset.from_st(st).allocate("cuda:0") for st in sets]
    for st, into in zip(sets, planned):
        extractw(_loader(st), model, None, 3, "cuda:0", into=into, chunk=chunk)
    torch.cuda.synchronize()
    return planned, time.perf_counter() - t0


def store_alone(reps, rounds):
    import torch
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    dev = torch.device("cuda:0")
    Q, rows, C = 2048, 4096, 512                                   # 103 MB of ground-truth planes
    gt_pool = torch.randint(0, 256, (Q, 224, 224), dtype=torch.uint8, device=dev)
    pool = torch.zeros((rows, C), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(1)
    for B in (1, 32):
        feat = torch.randn((B, 14, 14, C), device=dev)
        out = torch.empty((B, C), device=dev)
        dst = torch.stack([torch.randperm(rows, generator=g)[:B] for _ in range(16)]).to(dev)
        src = torch.stack([torch.randperm(Q, generator=g)[:B] for _ in range(16)]).to(dev)
        win = torch.tensor([[5, 9, 5, 9]] * B, dtype=torch.int32, device=dev)

        def run(which, r):
            if which == "lstm_store":
                check(Hp.LIB.egz_lstm_store(feat.data_ptr(), B, 14, 14, C, gt_pool.data_ptr(), Q, src[r % 16].data_ptr(), 16, 3,
                                            pool.data_ptr(), rows, dst[r % 16].data_ptr(), None, status.data_ptr(),
                                            Hp._stream()), "egz_lstm_store")
            else:
                check(Hp.LIB.egz_window_mean(feat.data_ptr(), win.data_ptr(), out.data_ptr(), B, 14, 14, C, Hp._stream()),
                      "egz_window_mean")
        res = {"lstm_store": [], "window_mean": []}
        for rnd in range(rounds + 1):                              # round 0 warms up
            for which in res:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for r in range(reps):
                    run(which, r)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    res[which].append(e0.elapsed_time(e1) / reps * 1e3)
        assert int(status.item()) == 0
        for which, us in res.items():
            emit({"item": "store", "kernel": which, "B": B, "C": C, "launches_per_window": reps, "us_per_launch": us,
                  "median_us": float(np.median(us))})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=1024)
    p.add_argument("--val", type=int, default=256)
    p.add_argument("--chunk", type=int, default=32)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_handover.txt"))
    a = p.parse_args()
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_handover: needs the GPU (no timing is taken on a CPU)")
    from bench_late_handover import st_sets
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    with tempfile.TemporaryDirectory() as root:
        paths = write_tree(os.path.join(root, "tree"), a.frames, a.val)
        torch.manual_seed(0)
        sp = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
        torch.save({'state_dict': sp.state_dict()}, os.path.join(root, "sp.pth.tar"))
        del sp
        model = encoder(os.path.join(root, "sp.pth.tar"))
        sets = st_sets(paths)
        modes = ("files", "memory_1", "memory_%d" % a.chunk)
        got, vectors = {}, None
        for rnd in range(a.rounds + 1):                            # round 0 warms up (weight caches, allocations, page cache)
            for mode in modes:                                     # ... and counts the waits
                got.pop(mode, None)
                waits = {}
                with (counted_waits(waits) if rnd == 0 else contextlib.nullcontext()):
                    if mode == "files":
                        out = os.path.join(root, "out")
                        got[mode], ext, fill, nfiles = files_handover(model, sets, out)
                        shutil.rmtree(out)
                        vectors = sum(len(d.listFiles) for d in got[mode])
                        rec = {"item": "files", "round": rnd, "ms_per_vector": (ext + fill) / vectors * 1e3,
                               "extract_ms_per_vector": ext / vectors * 1e3, "fill_ms_per_vector": fill / vectors * 1e3,
                               "files_per_vector": nfiles / vectors}
                    else:
                        got[mode], sec = memory_handover(model, sets, int(mode[7:]))
                        rec = {"item": "memory", "chunk": int(mode[7:]), "round": rnd, "ms_per_vector": sec / vectors * 1e3,
                               "files_per_vector": 0}
                if rnd:
                    emit(rec)
                elif mode == "files":
                    emit({"item": "device", "name": torch.cuda.get_device_name(0), "frames": a.frames + a.val,
                          "vectors": vectors, "chunk": a.chunk,
                          "note": "the file hand-over is the parent commit's code, unchanged; the paths run in this process, "
                                  "alternating"})
                if rnd == 0:
                    emit({"item": "waits", "path": mode, "calls": waits, "per_vector": sum(waits.values()) / vectors})
        for name in modes[1:]:
            emit({"item": "pools_equal", "files_against": name,
                  "equal": [bool(torch.equal(f.pool.view(torch.int32), m.pool.view(torch.int32)))
                            for f, m in zip(got["files"], got[name])]})
        del got, sets
        torch.cuda.empty_cache()
        store_alone(a.reps, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
