"""The flow hand-over measured against the code it replaces, in one process, runs alternated; one JSON line per item, also
written to --out (default profiles/flow_handover.txt):
  roundtrip  (a) hipops.jpeg_roundtrip against jpeg_encode + jpeg_decode -- the parent commit's VideoPredictor._jpeg_round_trip --
             at 82 planes of 224 x 224, quality 95 (predict's chunk of 32: 41 flow pairs).  Wall ms per call including the wait
             for the result (the pair waits inside, for its file lengths), per round; and the device time of --reps back-to-back
             jpeg_roundtrip launches over their number.  The outputs are compared first.
  handover   (b) per flow pair on a synthetic tree of 2 videos x --frames frames of 224 x 224: extract_flow.main to files on local
             disk + ResidentSTDataset.fill of both sets (decode='host' and decode='gpu'), against fill(flow_from=...).  Both
             include the decode of the image and ground-truth files, which is also given alone (a fill without the flow field).
             Files written and plane bytes over PCIe per pair alongside.
  predict    (c) VideoPredictor over one of those videos (fixsac all, no overlay, flow_jpeg 95), ms per predicted frame, with
             _jpeg_round_trip as the parent has it (the pair) and as it is now.
Every figure is given per round so the spread shows; round 0 of each item is a warm-up and is not printed.
Usage: python tools/bench_flow_handover.py [--frames 128] [--rounds 3] [--reps 200] [--out F]"""
import argparse
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
VIDEOS = ("Ahmad_Pizza1", "Alireza_Pizza1")


def emit(rec):
    OUT.append(json.dumps(rec) if isinstance(rec, dict) else rec)
    print(OUT[-1], flush=True)


def write_tree(root, frames, seed=0):
    """Two videos of ``frames`` JPEG frames (a smooth texture drifting by a pixel or two a frame) under framePath; every frame
    from number 10 on is a sample: PNG image, PNG ground truth, one fixation flag."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    paths = {k: os.path.join(root, d) for k, d in (("framePath", "frames"), ("imagePath", "img"), ("gtPath", "gt"),
                                                   ("fixsacPath", "fs"))}
    for d in paths.values():
        os.makedirs(d)
    yy, xx = np.mgrid[0:H, 0:W]
    for folder in VIDEOS:
        os.makedirs(os.path.join(paths["framePath"], folder))
        low = rs.randint(0, 256, (40, 40 + frames // 2, 3)).astype(np.uint8)
        big = np.asarray(Image.fromarray(low).resize((8 * low.shape[1], 8 * low.shape[0]), Image.BICUBIC))
        for num in range(1, frames + 1):
            dy, dx = int(round(20 + 12 * np.sin(num / 6.0))), 2 * num
            frame = Image.fromarray(big[dy:dy + H, dx:dx + W])
            frame.save(os.path.join(paths["framePath"], folder, f"img_{num:05d}.jpg"), quality=95)
            if 10 <= num < frames:
                frame.save(os.path.join(paths["imagePath"], f"{folder}_img_{num:05d}.png"))
                blob = 255.0 * np.exp(-((yy - rs.uniform(40, 180)) ** 2 + (xx - rs.uniform(40, 180)) ** 2) / (2.0 * 18.0 ** 2))
                Image.fromarray(blob.astype(np.uint8)).save(os.path.join(paths["gtPath"], f"{folder}_000000_{num:05d}.png"))
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), (rs.rand(frames - 10) < 0.4).astype(float))
    return paths


def st_sets(paths, flow_path, decode="host", fields=None):
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.gaze_full import _split
    sets = []
    for k in (0, 1):
        ds = ResidentSTDataset(flow_path, paths["imagePath"], paths["gtPath"], sorted(os.listdir(paths["framePath"])),
                               _split(paths["imagePath"], "Alireza")[k], _split(paths["gtPath"], "Alireza")[k],
                               _split(paths["fixsacPath"], "Alireza")[k], paths["fixsacPath"], raw_u8=True, decode=decode)
        if fields is not None:
            ds.gpu_fields = fields
        sets.append(ds)
    return sets


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def pair(planes, quality):
    """The parent commit's VideoPredictor._jpeg_round_trip."""
    from egaze_amd import hipops as Hh
    N, h, w = planes.shape
    data, offsets, status = Hh.jpeg_encode(planes, quality=quality)
    dec, dstatus = Hh.jpeg_decode(data, offsets, (h, w), [1] * N, n3=0)
    return dec.view(N, h, w), (status, dstatus)


def bench_roundtrip(rounds, reps):
    import torch
    from egaze_amd import hipops as Hh
    rs = np.random.RandomState(1)
    small = rs.randint(96, 160, (82, 28, 28)).astype(np.float32)
    x = torch.from_numpy(small).to("cuda:0")[:, None]
    x = torch.nn.functional.interpolate(x, size=(H, W), mode="bicubic")[:, 0].clamp(0, 255).to(torch.uint8).contiguous()
    want, _ = pair(x, 95)
    got, status = Hh.jpeg_roundtrip(x, 95)
    emit({"item": "roundtrip", "planes": 82, "hw": [H, W], "quality": 95, "equal": bool(torch.equal(got, want)),
          "status_max": int(status.abs().max())})
    for r in range(rounds + 1):
        rec = {"item": "roundtrip", "round": r}
        for name, fn in (("encode_decode_ms", lambda: pair(x, 95)), ("jpeg_roundtrip_ms", lambda: Hh.jpeg_roundtrip(x, 95))):
            dts = [timed(fn)[1] for _ in range(10)]
            rec[name] = round(float(np.median(dts)) * 1e3, 4)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = torch.empty_like(x)
        e0.record()
        for _ in range(reps):
            Hh.jpeg_roundtrip(x, 95, out=out)
        e1.record()
        torch.cuda.synchronize()
        rec["jpeg_roundtrip_device_ms"] = round(e0.elapsed_time(e1) / reps, 4)
        rec["GB_per_s_read_plus_written"] = round(2 * x.numel() / (e0.elapsed_time(e1) / reps * 1e-3) / 1e9, 1)
        if r:
            emit(rec)


def bench_handover(paths, tmp, frames, rounds):
    import torch
    from egaze_amd.data import extract_flow as E
    from egaze_amd.data.resident import FlowFrom
    pairs = 2 * (frames - 1)
    checked = False
    for r in range(rounds + 1):
        rec = {"item": "handover", "round": r, "pairs": pairs}
        flow_path = os.path.join(tmp, f"flow_{r}")
        written, t = timed(lambda: E.main(["--framePath", paths["framePath"], "--flowPath", flow_path]))
        rec["extract_flow_files_ms_per_pair"] = round(t / pairs * 1e3, 4)
        nbytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(flow_path) for f in fs)
        rec["files_per_pair"] = written / pairs
        for decode in ("host", "gpu"):
            sets = st_sets(paths, flow_path, decode)
            _, t = timed(lambda: [ds.fill("cuda:0") for ds in sets])
            rec[f"fill_{decode}_decode_ms_per_pair"] = round(t / pairs * 1e3, 4)
            # down: the encoded files; up: decoded planes (host decode) or the files again (GPU decode)
            rec[f"pcie_plane_bytes_per_pair_{decode}"] = round((nbytes + (2 * pairs * H * W if decode == "host" else nbytes)) / pairs)
            keep = sets
        plain = st_sets(paths, flow_path, fields=("image", "gt"))
        _, t = timed(lambda: [ds.fill("cuda:0") for ds in plain])
        rec["fill_image_gt_only_ms_per_pair"] = round(t / pairs * 1e3, 4)
        memory = st_sets(paths, os.path.join(tmp, "never"))
        _, t = timed(lambda: [ds.fill("cuda:0", flow_from=FlowFrom(paths["framePath"])) for ds in memory])
        rec["handover_fill_ms_per_pair"] = round(t / pairs * 1e3, 4)
        rec["handover_files_per_pair"] = 0
        rec["handover_pcie_plane_bytes_per_pair"] = 0
        rec["handover_pairs_computed"] = sum(ds.flow_counts["pairs"] for ds in memory)
        if not checked:
            rec["pools_equal"] = all(torch.equal(a.pool, b.pool) for a, b in zip(keep, memory))
            checked = True
        shutil.rmtree(flow_path)
        del keep, plain, memory, sets
        if r:
            emit(rec)
        elif "pools_equal" in rec:
            emit({"item": "handover", "pools_equal": rec["pools_equal"], "never_opened": not os.path.exists(os.path.join(tmp, "never"))})


def bench_predict(paths, tmp, frames, rounds):
    import torch
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.predict import VideoPredictor, load_models
    from egaze_amd.utils import cfg, make_layers
    torch.manual_seed(0)
    sp_file, late_file = os.path.join(tmp, "sp.pth.tar"), os.path.join(tmp, "late.pth.tar")
    torch.save({'state_dict': model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20)).state_dict()}, sp_file)
    torch.save({'state_dict': late_fusion().state_dict()}, late_file)
    model, _, late = load_models(sp_file, late_file, None, torch.device("cuda:0"))
    video = os.path.join(paths["framePath"], VIDEOS[0])
    now = VideoPredictor._jpeg_round_trip

    def before(self, planes, quality):
        dec, st = pair(planes, quality)
        self._codec.append(st)
        return dec
    n = frames - 10
    for r in range(rounds + 1):
        rec = {"item": "predict", "round": r, "frames": n, "chunk": 32}
        for name, fn in (("encode_decode_ms_per_frame", before), ("jpeg_roundtrip_ms_per_frame", now)):
            VideoPredictor._jpeg_round_trip = fn
            try:
                pred = VideoPredictor(model, None, late, fixsac='all', chunk=32, overlay=False, out=os.path.join(tmp, "out"))
                if r == 0:
                    pred.run(video)
                _, t = timed(lambda: pred.run(video))
                pred.close()
            finally:
                VideoPredictor._jpeg_round_trip = now
            rec[name] = round(t / n * 1e3, 4)
        if r:
            emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_handover.txt"))
    ap.add_argument("--only", nargs="*", default=["roundtrip", "handover", "predict"])
    a = ap.parse_args()
    import torch
    import egaze_amd  # noqa: F401
    props = torch.cuda.get_device_properties(0)
    emit(f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
         f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}, HIP {torch.version.hip}")
    emit(f"# tools/bench_flow_handover.py --frames {a.frames} --rounds {a.rounds} --reps {a.reps}")
    tmp = tempfile.mkdtemp(prefix="bench_flow_handover_")
    try:
        if "roundtrip" in a.only:
            bench_roundtrip(a.rounds, a.reps)
        if "handover" in a.only or "predict" in a.only:
            paths = write_tree(os.path.join(tmp, "tree"), a.frames)
        if "handover" in a.only:
            bench_handover(paths, tmp, a.frames, a.rounds)
        if "predict" in a.only:
            bench_predict(paths, tmp, a.frames, a.rounds)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
