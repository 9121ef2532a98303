"""egaze_amd.predict on a synthetic 224 x 224 video: ms per frame by phase, in the ``all`` and FILE fixation modes, with and
without ``--overlay``; and, in the same process on the same frames, what the training drivers need for the same maps -- the sum of
extract_flow (files), AT.extract_late (files read back through STDataset, PNG hand-over written) and one LF eval pass over those
files.  Weights are random-initialised: the launches do not depend on the values.  Prints plain lines; kept as
profiles/predict_video.txt.
Usage: python tools/bench_predict.py [--frames 512] [--chunk 32] [--passes 3] [--skip_drivers]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egaze_amd  # noqa
from egaze_amd.predict import VideoPredictor, load_models

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=512)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--skip_drivers", action="store_true", help="time the predictor only")
a = ap.parse_args()
DEV = torch.device("cuda:0")
PHASES = ("decode", "flow", "gather", "sp", "glue", "lf", "encode_write")


def texture(y, x):
    """A smooth seeded pattern with a finer octave, sampled bilinearly at real positions -> (len y, len x, 3) uint8."""
    rng = np.random.RandomState(7)
    out = 0.0
    for period, gain in ((16.0, 0.7), (5.0, 0.3)):
        cells = int(max(y.max(), x.max()) / period) + 3
        grid = rng.rand(cells, cells, 3)
        gy, gx = y / period, x / period
        y0, x0 = np.floor(gy).astype(int), np.floor(gx).astype(int)
        fy, fx = (gy - y0)[:, None, None], (gx - x0)[None, :, None]
        top = grid[y0][:, x0] * (1 - fx) + grid[y0][:, x0 + 1] * fx
        bot = grid[y0 + 1][:, x0] * (1 - fx) + grid[y0 + 1][:, x0 + 1] * fx
        out = out + gain * (top * (1 - fy) + bot * fy)
    return np.clip(np.rint(out * 255), 0, 255).astype(np.uint8)


def write_video(folder, n):
    from PIL import Image
    os.makedirs(folder)
    for k in range(n):
        y, x = np.arange(224) + 8 + 0.7 * k, np.arange(224) + 8 + 1.3 * k
        Image.fromarray(texture(y, x)).save(os.path.join(folder, "img_%05d.jpg" % (k + 1)), quality=95)


def time_predictor(models, video, out, fixsac, overlay):
    """-> (ms / frame of un-instrumented passes, phase -> ms / frame of one instrumented pass)."""
    model, lstm, late = models
    n = a.frames - 10
    kw = dict(fixsac=fixsac, chunk=a.chunk, overlay=overlay, out=out)
    pred = VideoPredictor(model, lstm if fixsac != 'all' else None, late, **kw)
    pred.run(video)                                                       # warm-up: workspaces, weight caches, tables
    dts = []
    for _ in range(a.passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred.run(video)
        torch.cuda.synchronize()
        dts.append((time.perf_counter() - t0) / n * 1e3)
    pred.close()
    prof = {}
    pred = VideoPredictor(model, lstm if fixsac != 'all' else None, late, profile=prof, **kw)
    pred.run(video)
    pred.close()
    return dts, {k: prof.get(k, 0.0) / n * 1e3 for k in PHASES}


def time_drivers(d, video, sp_file, late_file, lstm_file):
    """extract_flow -> AT.extract_late -> LF eval pass over the same frames, through the files: seconds of each leg."""
    import egaze_amd.AT as at_mod
    from egaze_amd.AT import AT
    from egaze_amd.LF import LF
    from egaze_amd.data import extract_flow
    from egaze_amd.data.STdatas import STDataset
    from PIL import Image
    legs = {}
    flow_dir, img_dir, gt_dir, fs_dir = (os.path.join(d, s) for s in ("flow", "img", "gt", "fs"))
    pred_dir, feat_dir = os.path.join(d, "new_pred") + "/", os.path.join(d, "new_feat") + "/"
    for s in (img_dir, gt_dir, fs_dir):
        os.makedirs(s)
    names, gts = [], []
    for k in range(9, a.frames - 1):                                      # the frames the predictor predicts
        names.append("vid_img_%05d.jpg" % (k + 1))
        gts.append("vid_000000_%05d.jpg" % (k + 1))
        os.symlink(os.path.join(video, "img_%05d.jpg" % (k + 1)), os.path.join(img_dir, names[-1]))
        Image.fromarray(np.full((224, 224), 1 + k % 255, np.uint8)).save(os.path.join(gt_dir, gts[-1]), quality=95)      # a dummy
    np.savetxt(os.path.join(fs_dir, "a.txt"), np.ones(len(names)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    extract_flow.main(["--framePath", os.path.dirname(video), "--flowPath", flow_dir, "--chunk", str(a.chunk)])
    torch.cuda.synchronize()
    legs["extract_flow"] = time.perf_counter() - t0

    for sub in ("train", "test"):
        os.makedirs(os.path.join(d, "512w", sub))
        for i in range(2):
            torch.save(torch.zeros(512), os.path.join(d, "512w", sub, f"fix_v_{i:010d}.pth.tar"))
    at = AT(pretrained_model=sp_file, pretrained_lstm=lstm_file, save_path=d, device='0', lstm_data_path=os.path.join(d, "512w"))
    at_mod._progress = lambda it: it
    ds = STDataset(flow_dir, img_dir, gt_dir, ["vid"], names, gts, ["a.txt"], fs_dir, raw_u8=True)
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, pin_memory=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    at.extract_late(loader, pred_dir, feat_dir, chunk=a.chunk)
    torch.cuda.synchronize()
    legs["extract_late"] = time.perf_counter() - t0

    lf = LF(pretrained_model=late_file, save_path=d, device='0', late_pred_path=pred_dir, late_feat_path=feat_dir, gt_path=gt_dir,
            val_name="no-such-video", batch_size=32)                      # every frame lands in the first loader
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        lf._run(lf.train_loader, False, 10 ** 9)                          # LF.testLate's pass over these files
    torch.cuda.synchronize()
    legs["lf_eval"] = time.perf_counter() - t0
    return legs


def main():
    props = torch.cuda.get_device_properties(0)
    print(f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
          f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}, HIP {torch.version.hip}")
    print(f"# video: {a.frames} synthetic frames of 224 x 224 (JPEG quality 95), {a.frames - 10} predictable; chunk {a.chunk}; "
          f"random-initialised weights; flow_jpeg 95, handover_jpeg 0")
    with tempfile.TemporaryDirectory() as d:
        from egaze_amd.models.late_fusion import late_fusion
        from egaze_amd.models.LSTMnet import lstmnet
        from egaze_amd.models.model_SP import model_SP
        from egaze_amd.utils import cfg, make_layers
        torch.manual_seed(0)
        video = os.path.join(d, "frames", "vid")
        write_video(video, a.frames)
        sp_file, late_file, lstm_file = (os.path.join(d, n) for n in ("sp.pth.tar", "late.pth.tar", "lstm.pth.tar"))
        torch.save({'state_dict': model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20)).state_dict()}, sp_file)
        torch.save({'state_dict': late_fusion().state_dict()}, late_file)
        torch.save(lstmnet().state_dict(), lstm_file)
        flags = os.path.join(d, "fixsac.txt")
        np.savetxt(flags, (np.random.RandomState(0).rand(a.frames) < 0.5).astype(float))
        models = load_models(sp_file, late_file, lstm_file, DEV)
        print("# predictor: ms per predicted frame; 'wall' = un-instrumented passes (median), phases = one pass that waits for "
              "the device after every phase (they can add up to more than 'wall')")
        walls = {}
        for fixsac, label in (('all', 'all'), (flags, 'FILE')):
            for overlay in (False, True):
                dts, prof = time_predictor(models, video, os.path.join(d, "out"), fixsac, overlay)
                walls[(label, overlay)] = statistics.median(dts)
                print(f"predict fixsac={label:4s} overlay={int(overlay)}  wall {statistics.median(dts):7.3f}  (passes "
                      f"{[round(v, 3) for v in dts]})  " + "  ".join(f"{k} {prof[k]:.3f}" for k in PHASES))
        if not a.skip_drivers:
            legs = time_drivers(d, video, sp_file, late_file, lstm_file)
            n = a.frames - 10
            total = sum(legs.values())
            print("# the training drivers over the same frames, through their files (one pass each, same process): ms per frame")
            print("drivers  " + "  ".join(f"{k} {v / n * 1e3:.3f}" for k, v in legs.items()) + f"  sum {total / n * 1e3:.3f}")
            print(f"# sum of the drivers / predictor (fixsac=all, no overlay): {total / n * 1e3 / walls[('all', False)]:.2f}x")


if __name__ == "__main__":
    main()
