#!/usr/bin/env python3
"""Generate the stream pre-training fixtures in this directory by running the REAL reference scripts.

Runs only where the reference tree is available (REF below, read-only).  Nothing from the reference is copied: the fixtures
hold numbers only (plus the reference model's state-dict key list); weights and inputs are regenerated on the consumer side
from oracle/synth.py with the same seeds.

    python tests/golden/make_golden_streams.py     # rewrites tests/golden/{spatial,temporal}_stream_s*.npz byte-identically

Maps above 64 x 64 are stored quantised to 16 bits and full gradients above 4096 entries as float16 (compact_map /
compact_grad); the tests decode them by dtype.

Both reference scripts parse argv, list the data folders and download VGG16-BN at import, so only their ``VGG`` class and
``train`` / ``validate`` functions are extracted (ast) and executed, with ``device = cpu``:
  spatialstream.py:65-116   VGG (frozen encoder)       temporalstream.py:63-111  VGG (20-channel encoder, not frozen)
  spatialstream.py:121-151  train                      spatialstream.py:154-184  validate   (temporalstream.py: the same)
"""
import ast
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

for name in ("cv2", "skimage", "skimage.io", "skimage.transform"):      # image I/O only, absent here
    sys.modules.setdefault(name, types.ModuleType(name))

from oracle import synth  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

# Adam moves every weight by about lr in step 1, in the direction of the sign of a gradient that is rounding noise for some
# entries: at 3e-6 the step-2 map stays comparable at 1e-4 relative (at 1e-4 it does not, for any fp32 implementation)
LR = 3e-6
SEEDS = {"spatial": 5, "temporal": 6}
HEAD_GAIN = 0.25


def compact_map(a):
    """A (B, 1, H, W) sigmoid map: float32 up to 64 x 64, above that quantised to 16 bits (round(v * 65535), absolute error
    <= 7.7e-6, a thirteenth of the tests' 1e-4 bar) to keep the fixture small."""
    if a.shape[-1] * a.shape[-2] <= 64 * 64:
        return a
    assert a.min() >= 0.0 and a.max() <= 1.0
    return np.round(a.astype(np.float64) * 65535.0).astype(np.uint16)


def compact_grad(g):
    """A full gradient tensor: float32 up to 4096 entries, float16 above (relative rounding 5e-4, far inside robust_close)."""
    return g if g.size <= 4096 else g.astype(np.float16)


def save(name, **arrs):
    """np.savez_compressed layout with a fixed member timestamp, so that a rerun writes the same bytes."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", name, "%.1f KB" % (os.path.getsize(path) / 1024))


def reference_defs(stream):
    """VGG / train / validate of <stream>stream.py, executed in a namespace with the reference's utils and device = cpu."""
    import math
    import time
    import torch.nn as nn
    import utils as rutils
    src = open(os.path.join(REF, stream + "stream.py")).read()
    keep = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "VGG"
            or isinstance(n, ast.FunctionDef) and n.name in ("train", "validate")]
    ns = {k: getattr(rutils, k) for k in dir(rutils) if not k.startswith("_")}
    ns.update({"nn": nn, "math": math, "np": np, "torch": torch, "time": time, "tqdm": lambda it: it,
               "device": torch.device("cpu")})
    exec(compile(ast.Module(body=keep, type_ignores=[]), stream + "stream_defs", "exec"), ns)
    return ns, rutils


def gen_stream(stream, size, tag):
    from floss import floss
    ns, rutils = reference_defs(stream)
    cin, key = (3, "image") if stream == "spatial" else (20, "flow")
    model = ns["VGG"](rutils.make_layers(rutils.cfg["D"], cin))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=SEEDS[stream], head_gain=HEAD_GAIN))
    arrs = {"keys": np.array(list(model.state_dict().keys())), "lr": np.array(LR)}
    criterion = floss()

    # ---- validate on a 2-batch loader (batches of 2 and 1: the per-sample and the 2-D branch of computeAAEAUC)
    v_s, v_t, v_gt, _ = synth.synth_sp_batch(3, size, seed=7)
    v_in = v_s if stream == "spatial" else v_t
    val_loader = [{key: v_in[:2], "gt": v_gt[:2]}, {key: v_in[2:], "gt": v_gt[2:]}]
    metrics = []
    base = ns["computeAAEAUC"]

    def recording(o, t):
        r = base(o, t)
        metrics.append((r[0], r[1]))
        return r
    ns["computeAAEAUC"] = recording
    arrs["val_loss"] = np.array(ns["validate"](val_loader, model, criterion, 0))
    ns["computeAAEAUC"] = base
    arrs["val_aae"] = np.array([m[0] for m in metrics], np.float64)
    arrs["val_auc"] = np.array([m[1] for m in metrics], np.float64)

    # ---- eval-mode output (running statistics)
    x_s, x_t, gt, _ = synth.synth_sp_batch(2, size, seed=0)
    x = x_s if stream == "spatial" else x_t
    model.eval()
    with torch.no_grad():
        arrs["eval_out"] = compact_map(model(x).numpy())

    # ---- two literal reference training steps: the reference's own train() over a 2-batch loader of the same batch
    optimizer = torch.optim.Adam(model.decoder.parameters(), lr=LR)
    p0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    outs, grads = [], []
    h = model.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()))
    optimizer.register_step_pre_hook(lambda opt, a, kw: grads.append(
        {k: p.grad.detach().clone() for k, p in model.named_parameters() if k.startswith("decoder.")}))
    losses = []
    crit = lambda o, t: losses.append(criterion(o, t)) or losses[-1]      # noqa: E731
    ns["train"]([{key: x, "gt": gt}, {key: x, "gt": gt}], model, crit, optimizer, 0)
    h.remove()
    for s in (0, 1):
        arrs[f"train_out{s + 1}"] = compact_map(outs[s].numpy())
        arrs[f"train_loss{s + 1}"] = np.array(losses[s].item())
    for k, g in grads[0].items():
        g64 = g.double()
        arrs["gsum/" + k] = np.array([g64.norm().item(), g64.sum().item(), g64.abs().max().item()])
        if g.numel() <= 512 or k == "decoder.28.weight":
            arrs["grad/" + k] = compact_grad(g.numpy())
    for k, p in model.named_parameters():
        if k.startswith("decoder."):
            d = (p.detach() - p0[k]).double()
            arrs["delta/" + k] = np.array([d.sum().item(), d.abs().max().item()])
        else:
            assert torch.equal(p.detach(), p0[k]), k          # the reference never updates the encoder
    for k, v in model.state_dict().items():
        if "running_" in k and v.numel() <= 64:
            arrs["after/" + k] = v.numpy()
        elif "running_" in k:
            arrs["after_sum/" + k] = np.array([v.double().sum().item(), v.double().norm().item()])
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 2, k
    print(tag, "eval out", arrs["eval_out"].min(), arrs["eval_out"].max(), "losses", losses[0].item(), losses[1].item(),
          "val", float(arrs["val_loss"]), arrs["val_aae"], arrs["val_auc"])
    save(f"{stream}_stream_{tag}.npz", **arrs)


if __name__ == "__main__":
    gen_stream("spatial", 32, "s32")
    gen_stream("temporal", 32, "s32")
    gen_stream("spatial", 224, "s224")
