"""The AT -> LF hand-over measured both ways in one process (gaze_full --late_handover against the hand-over through files); one
JSON line per item, also written to --out (default profiles/late_handover.txt):
  files     the existing hand-over, whose code is the parent commit's, unchanged: AT.extract_late of both videos into pred / feat
            folders on local disk (real PNG encodes and writes), then ResidentLateDataset.fill of LF's listing of them, with
            decode='host' and decode='gpu' (--gpu_decode; the hand-over PNGs are host-decoded either way).  ms per frame per
            phase, the files written, the plane bytes that cross PCIe (2 planes read back, 3 uploaded, per frame)
  memory    ResidentLateDataset.from_st + allocate + AT.extract_late(into=...): ms per frame, no file, no plane over PCIe (the
            destination rows go up, 24 bytes a frame, and the status words come back, 8 bytes a chunk)
  lf_iter   LF.trainLate per iteration from the file-filled sets and from the in-memory sets, same seed (equal work: the pools
            are equal byte for byte)
  store     egz_late_store alone against egz_late_input alone at n = 32, 224 x 224 from 14 x 14: device time of --reps
            back-to-back launches over their number, and the bytes each moves
The two hand-overs alternate, --rounds times after a warm-up round; every figure is given per round so the spread shows.
The tree is synthetic: one training video of --frames frames and one validation video of --val, PNG frames and ground truth,
JPEG flow, random-initialised weights.
Usage: python tools/bench_late_handover.py [--frames 512] [--val 64] [--chunk 32] [--batch 32] [--rounds 3] [--reps 200] [--out F]"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = []
H = W = 224
TRAIN, VAL = "Ahmad_Pizza1", "Alireza_Pizza1"


def emit(rec):
    OUT.append(json.dumps(rec))
    print(OUT[-1], flush=True)


def write_tree(root, frames, val, distinct=16, seed=0):
    """A dataset tree as gaze_full's flags name it: PNG frames (so the hand-over files are PNGs), grey JPEG flow, PNG ground
    truth, one fixation file per video (about three frames in four are fixations, as in the real split).  The pixel content
    cycles through ``distinct`` smooth images per kind; every name is its own file."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    paths = {k: os.path.join(root, d) for k, d in (("flowPath", "flow"), ("imagePath", "img"), ("gtPath", "gt"),
                                                   ("fixsacPath", "fs"))}
    for d in paths.values():
        os.makedirs(d)

    def encoded(shape, fmt):
        out = []
        for _ in range(distinct):
            small = rs.randint(0, 256, (28, 28) + shape).astype(np.uint8)
            buf = io.BytesIO()
            Image.fromarray(small).resize((W, H), Image.BICUBIC).save(buf, format=fmt)
            out.append(buf.getvalue())
        return out
    flow, img, gt = encoded((), "JPEG"), encoded((3,), "PNG"), encoded((), "PNG")

    def put(path, data):
        with open(path, "wb") as f:
            f.write(data)
    for folder, n in ((TRAIN, frames), (VAL, val)):
        os.makedirs(os.path.join(paths["flowPath"], folder))
        for num in range(1, 10 + n):
            for k, ax in enumerate("xy"):
                put(os.path.join(paths["flowPath"], folder, f"flow_{ax}_{num:05d}.jpg"), flow[(2 * num + k) % distinct])
        for num in range(10, 10 + n):
            put(os.path.join(paths["imagePath"], f"{folder}_img_{num:05d}.png"), img[num % distinct])
            put(os.path.join(paths["gtPath"], f"{folder}_000000_{num:05d}.png"), gt[num % distinct])
        flags = (rs.rand(n) < 0.37).astype(float)                  # STDataset dilates them: 0.75
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), flags)
    return paths


def st_sets(paths):
    from egaze_amd.data.resident import ResidentSTDataset, fill_all
    from egaze_amd.gaze_full import _split
    sets = []
    for k in (0, 1):
        sets.append(ResidentSTDataset(paths["flowPath"], paths["imagePath"], paths["gtPath"], sorted(os.listdir(paths["flowPath"])),
                                      _split(paths["imagePath"], "Alireza")[k], _split(paths["gtPath"], "Alireza")[k],
                                      _split(paths["fixsacPath"], "Alireza")[k], paths["fixsacPath"], raw_u8=True))
    fill_all(sets, "cuda:0")
    return sets


def _loader(ds):
    from torch.utils.data import DataLoader
    return DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, pin_memory=True, collate_fn=ds.collate_fn)


def files_handover(at, sets, paths, out, chunk, decode):
    """-> (late sets, seconds of the extraction, seconds of the fill, files written)."""
    import torch
    from egaze_amd.LF import _split
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.resident import fill_all
    pred, feat = os.path.join(out, "pred"), os.path.join(out, "feat")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for st in (sets[1], sets[0]):
        at.extract_late(_loader(st), pred + "/", feat + "/", chunk=chunk)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    late = [ResidentLateDataset(pred, paths["gtPath"], feat, _split(pred, "Alireza", None)[k],
                                _split(paths["gtPath"], "Alireza", None)[k], _split(feat, "Alireza", None)[k], decode=decode)
            for k in (0, 1)]
    fill_all(late, "cuda:0", flag="--late_resident")
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return late, t1 - t0, t2 - t1, len(os.listdir(pred)) + len(os.listdir(feat))


def memory_handover(at, sets, chunk):
    import torch
    from egaze_amd.data.late_resident import ResidentLateDataset
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    late = [ResidentLateDataset.from_st(st).allocate("cuda:0") for st in sets]
    for st, into in ((sets[1], late[1]), (sets[0], late[0])):
        at.extract_late(_loader(st), chunk=chunk, into=into)
    torch.cuda.synchronize()
    return late, time.perf_counter() - t0


def lf_iterations(late, save, batch, gt_path):
    import torch
    from egaze_amd.LF import LF
    torch.manual_seed(0)
    lf = LF(save_path=save, device="0", batch_size=batch, lr=1e-4, datasets=late, gt_path=gt_path)
    lf.trainLate()                                                 # warm-up: eager steps, graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lf.trainLate()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(lf.train_loader) * 1e3


def store_alone(reps, rounds, n=32):
    import torch
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    dev = torch.device("cuda:0")
    sp, at = torch.rand((n, H, W), device=dev), torch.rand((n, 14, 14), device=dev)
    P = 3 * 2048                                                   # 308 MB of planes: larger than the Infinity Cache
    pool = torch.zeros((P, H, W), dtype=torch.uint8, device=dev)
    gt_pool = torch.randint(0, 256, (2048, H, W), dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(1)
    dst = torch.stack([torch.randperm(P, generator=g)[:3 * n].view(n, 3) for _ in range(16)]).to(dev)
    src = torch.stack([torch.randperm(2048, generator=g)[:n] for _ in range(16)]).to(dev)
    fused = torch.empty((n, 2, H, W), dtype=torch.float32, device=dev)
    planes = torch.empty((n, 2, H, W), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tabs = [t.data_ptr() for t in Hp._linear_tables(dev, (14, 14), (H, W), "bench")]
    head = (sp.data_ptr(), 0, at.data_ptr(), 0, n, H, W, 14, 14, *tabs)

    def run(which, r):
        if which == "late_store":
            check(Hp.LIB.egz_late_store(*head, pool.data_ptr(), P, dst[r % 16].data_ptr(), gt_pool.data_ptr(), 2048,
                                        src[r % 16].data_ptr(), status.data_ptr(), Hp._stream()), "egz_late_store")
        else:
            check(Hp.LIB.egz_late_input(*head, fused.data_ptr(), planes.data_ptr() if which == "late_input_u8" else None,
                                        status.data_ptr(), Hp._stream()), "egz_late_input")
    res = {"late_store": [], "late_input": [], "late_input_u8": []}
    for rnd in range(rounds + 1):                                  # round 0 warms up
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
    moved = {"late_store": n * (H * W * 4 + 14 * 14 * 4 + 4 * H * W),            # sp read, at read, 3 planes written, gt read
             "late_input": n * (H * W * 4 + 14 * 14 * 4 + 2 * 4 * H * W),        # sp read, at read, fused written
             "late_input_u8": n * (H * W * 4 + 14 * 14 * 4 + 2 * 5 * H * W)}
    for which, us in res.items():
        emit({"item": "store", "kernel": which, "n": n, "hw": [H, W], "launches_per_window": reps, "us_per_launch": us,
              "median_us": float(np.median(us)), "counted_bytes": moved[which],
              "TB_per_s": moved[which] / float(np.median(us)) / 1e6})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=512)
    p.add_argument("--val", type=int, default=64)
    p.add_argument("--chunk", type=int, default=32)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_handover.txt"))
    a = p.parse_args()
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_late_handover: needs the GPU (no timing is taken on a CPU)")
    import egaze_amd.AT as at_mod
    from egaze_amd.AT import AT
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    try:
        import cv2  # noqa: F401
        resizer = "cv2"
    except ImportError:
        resizer = "PIL"
    emit({"item": "device", "name": torch.cuda.get_device_name(0), "frames": a.frames, "val": a.val, "chunk": a.chunk,
          "host_resize_of_the_file_path": resizer,
          "note": "the file hand-over is the parent commit's code, unchanged; both paths run in this process, alternating"})
    frames = a.frames + a.val
    with tempfile.TemporaryDirectory() as root:
        paths = write_tree(os.path.join(root, "tree"), a.frames, a.val)
        torch.manual_seed(0)
        sp = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
        torch.save({'state_dict': sp.state_dict()}, os.path.join(root, "sp.pth.tar"))
        for sub in ("train", "test"):
            os.makedirs(os.path.join(root, "512w", sub))
            for i in range(2):
                torch.save(torch.zeros(512), os.path.join(root, "512w", sub, f"fix_v_{i:010d}.pth.tar"))
        at = AT(pretrained_model=os.path.join(root, "sp.pth.tar"), save_path=root, device='0',
                lstm_data_path=os.path.join(root, "512w"))
        at_mod._progress = lambda it: it
        sets = st_sets(paths)
        late = {}
        for rnd in range(a.rounds + 1):                            # round 0 warms up: weight caches, allocations, page cache
            for mode in ("files_host", "memory", "files_gpu", "memory"):
                late.pop(mode, None)
                if mode == "memory":
                    late[mode], sec = memory_handover(at, sets, a.chunk)
                    rec = {"item": "memory", "round": rnd, "ms_per_frame": sec / frames * 1e3, "files": 0,
                           "pcie_plane_bytes_per_frame": 0, "pcie_other_bytes_per_frame": 24 + 16.0 / a.chunk}
                else:
                    out = os.path.join(root, "out")
                    late[mode], ext, fill, nfiles = files_handover(at, sets, paths, out, a.chunk, mode[6:])
                    shutil.rmtree(out)
                    rec = {"item": "files", "decode": mode[6:], "round": rnd, "ms_per_frame": (ext + fill) / frames * 1e3,
                           "extract_ms_per_frame": ext / frames * 1e3, "fill_ms_per_frame": fill / frames * 1e3,
                           "files": nfiles, "pcie_plane_bytes_per_frame": H * W + 14 * 14 + 3 * H * W}
                if rnd:
                    emit(rec)
        for a_, b_ in zip(late["files_host"], late["memory"]):
            n = len(a_)                                               # (PIL's host resize rounds unlike cv2's: the feat column)
            emit({"item": "pools_equal", "frames": n, "equal": bool(torch.equal(a_.pool, b_.pool)),
                  "bytes_that_differ": {name: int((a_.pool[c * n:(c + 1) * n] != b_.pool[c * n:(c + 1) * n]).sum())
                                        for c, name in enumerate(("pred", "feat", "gt"))},
                  "max_abs_difference": int((a_.pool.int() - b_.pool.int()).abs().max())})
        os.makedirs(os.path.join(root, "save"))
        for rnd in range(a.rounds):
            for mode in ("files_host", "memory"):
                emit({"item": "lf_iter", "sets": mode, "round": rnd + 1, "B": a.batch,
                      "ms_per_iter": lf_iterations(late[mode], os.path.join(root, "save"), a.batch, paths["gtPath"])})
        del late, sets
        torch.cuda.empty_cache()
        store_alone(a.reps, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
