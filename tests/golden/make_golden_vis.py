#!/usr/bin/env python3
"""Generate tests/golden/vis_features.npz by running the REAL reference vis_features() (vis_features.py:40-124) in place.

Runs only where the reference tree is available (REF below, read-only); nothing from it is copied.  Its script does not run
as written, so the module is given what it lacks: ``batch_size`` and ``device`` (cpu) as module globals, and the model
instance a forward that accepts and drops the extra arguments of its four-argument call.  cv2 and skimage (absent here) are
stubbed: resize = the INTER_LINEAR restatement of tests/test_vis_host.py (its 14 x 14 input is recorded), applyColorMap = a
lookup in the LUT stored below, imread = the synthetic frame of that name, imwrite / imsave capture the arrays.
crop_feature_var and the LSTM are wrapped to record the gt cells, the window means and the LSTM outputs.

Inputs: test_vis_host.synth_inputs(SEED, 6) as three batches of B = 2 after 100 placeholder batches (never touched);
weights: the config-5 synthetic weights (seeds 1 and 2).

    python tests/golden/make_golden_vis.py      # rewrites tests/golden/vis_features.npz byte-identically

Keys: lut (256, 3); cells (6,); window_mean (6, 512); lstm_out (6, 512); maps14 (8, 14, 14) in the reference's order (per
batch gt, noweight, then pred from the second batch); map_names (text); gaze (3, 224, 224); full_<kind> (224, 224, 3) for
the last batch's row 0; digests (text, one 'name sha256' per line of every overlay, after rint).
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED, B, NB, FIRST = 11, 2, 3, 100


def main():
    import test_vis_host as V                      # before REF joins sys.path: it imports the package under test
    from oracle import synth
    sys.path.insert(0, REF)
    for name in ("cv2", "skimage", "skimage.io"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    torch.manual_seed(0)
    torch.set_num_threads(8)

    inp = V.synth_inputs(SEED, B * NB)
    lut = V.random_lut(SEED)
    names = ["Alireza_f%02d.jpg" % k for k in range(B * NB)]
    frames = {n: inp["image"][k].transpose(1, 2, 0).copy() for k, n in enumerate(names)}

    written, maps14 = {}, []
    cv2 = sys.modules["cv2"]
    cv2.COLORMAP_JET = 2
    cv2.imread = lambda path, *a: frames[os.path.basename(path)].copy()
    cv2.applyColorMap = lambda arr, code: lut[arr]
    cv2.imwrite = lambda path, arr: written.__setitem__(path, np.array(arr, copy=True))

    def _resize(arr, size):
        maps14.append(np.array(arr, copy=True))
        return V.resize_linear(arr, (size[1], size[0]))
    cv2.resize = _resize
    sys.modules["skimage.io"].imsave = lambda path, arr: written.__setitem__(path, np.array(arr, copy=True))

    import vis_features as rvis
    from models.model_SP import model_SP
    from models.LSTMnet import lstmnet
    import utils as rutils

    rvis.batch_size = B
    rvis.device = torch.device("cpu")
    model = model_SP(rutils.make_layers(rutils.cfg["D"], 3), rutils.make_layers(rutils.cfg["D"], 20))
    model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1,
                                                 head_gain=0.25))
    two_arg = model.forward
    model.forward = lambda x_s, x_t, *dropped: two_arg(x_s, x_t)
    model._modules.get(rvis.hook_name).register_forward_hook(rvis.hook_feature)
    lstm = lstmnet()
    lstm.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in lstm.state_dict().items()}, seed=2))

    cells, means, outs = [], [], []
    crop = rvis.crop_feature_var

    def _crop(feature, maxind, size):
        cells.extend(int(m.item()) for m in maxind)
        res = crop(feature, maxind, size)
        means.append(res.view(res.size(0), res.size(1), -1).mean(2).detach().numpy().copy())
        return res
    rvis.crop_feature_var = _crop
    lstm.register_forward_hook(lambda mod, args, out: outs.append(out[0].detach().numpy().reshape(-1, 512).copy()))

    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    loader = [None] * FIRST
    for b in range(NB):
        s = slice(b * B, (b + 1) * B)
        loader.append({"imname": names[s],
                       "image": (torch.from_numpy(inp["image"][s]).float().div(255) - mean) / std,
                       "flow": (torch.from_numpy(inp["flow"][s]).float().div_(255) - 0.5) / 0.5,
                       "gt": torch.from_numpy(inp["gt"][s]).float().div(255)})
    with torch.no_grad():
        rvis.vis_features(loader, model, lstm, "vis/")

    kinds = ["gt_", "noweight_", "pred_"]
    map_names = []
    for b in range(NB):
        map_names += [k + names[b * B] for k in kinds if k != "pred_" or b > 0]
    ov = {}
    for n in map_names:
        ov[n] = np.clip(np.rint(written["vis/" + n]), 0, 255).astype(np.uint8)
    gaze = np.stack([np.uint8(np.rint(written["vis/gaze_" + names[b * B]] * 255)) for b in range(NB)])
    last = names[(NB - 1) * B]
    full = {"full_" + k.rstrip("_"): ov[k + last] for k in kinds}
    digests = "\n".join(f"{n} {V.digest(ov[n])}" for n in map_names)
    assert len(maps14) == len(map_names) and cells == [int(c) for c in inp["cells"]], (cells, inp["cells"])
    arrs = dict(lut=lut, cells=np.array(cells, np.int64), window_mean=np.concatenate(means), lstm_out=np.concatenate(outs),
                maps14=np.stack(maps14), map_names=np.frombuffer("\n".join(map_names).encode(), np.uint8),
                gaze=gaze, digests=np.frombuffer(digests.encode(), np.uint8), **full)
    path = os.path.join(HERE, "vis_features.npz")
    np.savez_compressed(path, **arrs)
    print("wrote vis_features.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
