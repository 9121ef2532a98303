"""Feature visualisation (vis_features.py, csrc/vis_overlay.hip): where the time of a visualised batch goes.

    python tools/bench_vis.py [--batch 10] [--iters 20] [--host-iters 3]

Prints one JSON line per measurement, on 224 x 224 synthetic data with the config-5 synthetic weights:
  chain    device ms per visualised batch and per frame (all_frames: 3 overlays per row) for each phase -- forward (the
           model_SP forward whose features_s the driver hooks), crop (gt cell + its read-back + window means), lstm (T = batch, batch 1), maps (three weighted min-max maps
           + uint8), overlay (one launch for every overlay of the batch) -- from device events, median of --iters batches.
  overlay  egz_heatmap_overlay alone for 30 overlays: median device ms, and the bytes it writes and reads against HBM.
  host     the same map -> overlay chain restated on the host in numpy (tests/test_vis_host.py), ms for 30 overlays.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def _median_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    import test_vis_host as V
    from egaze_amd import hipops as H
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    from egaze_amd.functions import to_nhwc
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    from egaze_amd.vis_features import CROP, crop_window
    from oracle import synth

    dev = "cuda:0"
    B = args.batch
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1,
                                                 head_gain=0.25))
    lstm = lstmnet()
    lstm.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in lstm.state_dict().items()}, seed=2))
    model.to(dev).eval()
    lstm.to(dev).eval()
    inp = V.synth_inputs(51, B)
    image = torch.from_numpy(inp['image']).to(dev)
    gt = torch.from_numpy(inp['gt']).to(dev)
    flow = torch.from_numpy(inp['flow']).to(dev)
    seen = []
    model.features_s.register_forward_hook(lambda m, i, o: seen.append(o))
    lut = torch.from_numpy(V.random_lut(51)).to(dev)
    st = {}
    phases = ("forward", "crop", "lstm", "maps", "overlay")
    times = {p: [] for p in phases}
    hidden = None
    with torch.no_grad():
        for it in range(args.iters + 3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
            ev[0].record()
            del seen[:]
            model(H.u8_normalize(image, IMAGE_MEAN, IMAGE_STD), H.u8_normalize(flow, FLOW_MEAN, FLOW_STD))
            feat = to_nhwc(seen[0])
            ev[1].record()
            cells = H.cell_argmax_u8(gt, 16).cpu().tolist()
            chn = H.window_mean(feat, [crop_window(c, 14, 14, CROP) for c in cells])
            ev[2].record()
            out, hidden = lstm(chn.unsqueeze(1), hidden)
            pred = out.reshape(B, -1)
            ev[3].record()
            maps = [(255 * H.weighted_minmax(feat, w)).to(torch.uint8) for w in (chn, torch.ones_like(chn), pred)]
            sel = torch.cat(maps)
            ev[4].record()
            ov = H.heatmap_overlay(sel, image, list(range(B)) * 3, lut)
            ev[5].record()
            ev[5].synchronize()
            if it >= 3:
                for k, p in enumerate(phases):
                    times[p].append(ev[k].elapsed_time(ev[k + 1]))
        H.lstm_persist_check()
    med = {p: round(float(np.median(times[p])), 4) for p in phases}
    total = sum(med.values())
    print(json.dumps({"bench": "chain", "batch": B, "overlays_per_batch": 3 * B, "ms_per_batch": med,
                      "ms_per_batch_total": round(total, 4), "ms_per_frame_total": round(total / B, 4),
                      "ms_per_frame": {p: round(v / B, 4) for p, v in med.items()}}), flush=True)

    # the overlay kernel alone, 30 overlays of 224 x 224 over 10 frames
    M = 30
    maps30 = torch.from_numpy(np.random.RandomState(52).randint(0, 256, size=(M, 14, 14)).astype(np.uint8)).to(dev)
    fi = [m % B for m in range(M)]
    for _ in range(3):
        H.heatmap_overlay(maps30, image, fi, lut)
    ms, all_ms = _median_ms(lambda: H.heatmap_overlay(maps30, image, fi, lut), args.iters)
    wr = M * 224 * 224 * 3
    rd = M * 224 * 224 * 3 + M * 196
    st["overlay"] = ms
    print(json.dumps({"bench": "overlay", "overlays": M, "ms": round(ms, 4), "ms_all": [round(t, 4) for t in all_ms],
                      "write_MB": round(wr / 1e6, 3), "read_MB_max": round(rd / 1e6, 3),
                      "GB_per_s_written": round(wr / ms / 1e6, 1)}), flush=True)

    # the same chain on the host, numpy
    maps_h = maps30.cpu().numpy()
    frames_h = inp['image']
    lut_h = lut.cpu().numpy()
    ts = []
    for _ in range(args.host_iters):
        t0 = time.perf_counter()
        for m in range(M):
            V.overlay(maps_h[m], frames_h[fi[m]], lut_h)
        ts.append((time.perf_counter() - t0) * 1e3)
    hm = float(np.median(ts))
    print(json.dumps({"bench": "host", "overlays": M, "ms": round(hm, 2), "kernel_speedup": round(hm / st["overlay"], 1)}),
          flush=True)


if __name__ == "__main__":
    main()
