"""Feature visualisation on the GPU (csrc/vis_overlay.hip, vis_features.py): the INTER_LINEAR resize, the overlay chain and
the gt cell bit-identical to the numpy restatements of test_vis_host.py; the spatial encoder run alone equal to the features_s
a full model_SP forward hooks; the driver against the reference's own vis_features() (tests/golden/vis_features.npz, made
by make_golden_vis.py); and the CLI end to end on a small synthetic GTEA tree, host and GPU JPEG decode."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vis_host as V  # noqa: E402  (the numpy restatements and the seeded inputs)

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_features.npz")


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- kernels
RESIZE_CASES = [
    ("14to224", 1, (14, 14), (224, 224), 1, "chw"),
    ("224to14", 1, (224, 224), (14, 14), 1, "chw"),
    ("720pto224_chw", 1, (720, 1280), (224, 224), 3, "chw"),
    ("720pto224_hwc", 1, (720, 1280), (224, 224), 3, "hwc"),
    ("224to720p_chw", 1, (224, 224), (720, 1280), 3, "chw"),
    ("224to720p_hwc", 1, (224, 224), (720, 1280), 3, "hwc"),
    ("1x1", 1, (1, 1), (5, 7), 1, "chw"),
    ("odd_up_batch30", 30, (13, 29), (31, 11), 1, "chw"),
    ("odd_down_batch30", 30, (97, 61), (23, 40), 3, "hwc"),
    ("odd_ratio", 1, (37, 53), (100, 19), 3, "chw"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resize_linear_bit_identical_to_restatement(case):
    from egaze_amd import hipops as H
    _, N, src, dst, C, layout = case
    rs = np.random.RandomState(sum(map(ord, case[0])))
    if C == 1:
        img = rs.randint(0, 256, size=(N,) + src).astype(np.uint8)
        got = H.resize_linear_u8(_u8(img), dst, layout).cpu().numpy()
        want = np.stack([V.resize_linear(im, dst) for im in img])
    elif layout == "hwc":
        img = rs.randint(0, 256, size=(N,) + src + (3,)).astype(np.uint8)
        got = H.resize_linear_u8(_u8(img), dst, layout).cpu().numpy()
        want = np.stack([V.resize_linear(im, dst) for im in img])
    else:
        img = rs.randint(0, 256, size=(N, 3) + src).astype(np.uint8)
        got = H.resize_linear_u8(_u8(img), dst, layout).cpu().numpy()
        want = np.stack([V.resize_linear(im.transpose(1, 2, 0), dst).transpose(2, 0, 1) for im in img])
    assert got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_resize_rejects_exact_2x_decimation_and_bad_shapes():
    from egaze_amd import hipops as H
    with pytest.raises(ValueError, match="2x decimation"):
        H.resize_linear_u8(torch.zeros((28, 28), dtype=torch.uint8, device=DEV), (14, 14))
    with pytest.raises(ValueError, match="channels"):
        H.resize_linear_u8(torch.zeros((1, 2, 8, 8), dtype=torch.uint8, device=DEV), (4, 3))
    with pytest.raises(ValueError, match="layout"):
        H.resize_linear_u8(torch.zeros((8, 8), dtype=torch.uint8, device=DEV), (4, 3), layout="hwc")


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(224, 224), (30, 45)])
def test_heatmap_overlay_bit_identical_with_ties(hw):
    from egaze_amd import hipops as H
    rs = np.random.RandomState(7)
    M, F = 12, 4
    maps = rs.randint(0, 256, size=(M, 14, 14)).astype(np.uint8)
    lut = V.random_lut(8)
    lut[::3] = (rs.randint(0, 52, size=lut[::3].shape) * 5).astype(np.uint8)    # multiples of 5: h * 0.3 lands on .5 often
    frames = rs.randint(0, 256, size=(F, 3) + hw).astype(np.uint8)
    frames[:2] = (rs.randint(0, 8, size=(2, 3) + hw) * 2 + 1).astype(np.uint8)   # small odd values: i * 0.5 = k + .5
    frames[2, :, ::2] = 0
    fi = rs.randint(0, F, size=M)
    got = H.heatmap_overlay(_u8(maps), _u8(frames), fi.tolist(), _u8(lut)).cpu().numpy()
    want = np.stack([V.overlay(maps[m], frames[fi[m]], lut) for m in range(M)])
    assert np.array_equal(got, want)
    # the ties were hit: some blended value is exactly k + .5 before rounding
    heat = lut[V.resize_linear(maps[0], hw)]
    v = heat * 0.3 + frames[fi[0]].transpose(1, 2, 0) * 0.5
    assert np.any(v == np.floor(v) + 0.5)


@pytest.mark.gpu
def test_heatmap_overlay_argument_checks():
    from egaze_amd import hipops as H
    maps = torch.zeros((2, 14, 14), dtype=torch.uint8, device=DEV)
    frames = torch.zeros((2, 3, 224, 224), dtype=torch.uint8, device=DEV)
    lut = torch.zeros((256, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="frame indices"):
        H.heatmap_overlay(maps, frames, [0, 2], lut)
    with pytest.raises(ValueError, match="frame indices"):
        H.heatmap_overlay(maps, frames, [0], lut)
    with pytest.raises(ValueError, match="lut"):
        H.heatmap_overlay(maps, frames, [0, 1], lut[:128])
    with pytest.raises(ValueError, match="frames"):
        H.heatmap_overlay(maps, frames[:, :2].contiguous(), [0, 1], lut)
    with pytest.raises(ValueError, match="contiguous"):
        H.heatmap_overlay(maps.transpose(1, 2), frames, [0, 1], lut)


@pytest.mark.gpu
def test_cell_argmax_matches_numpy_first_argmax():
    from egaze_amd import hipops as H
    rs = np.random.RandomState(9)
    g = rs.randint(0, 256, size=(20, 1, 224, 224)).astype(np.uint8)
    g[5] = 0                                               # all cells tie: cell 0
    g[6] = 0
    g[6, 0, 16 * 9 + 2, 16 * 3 + 5] = 40                   # two tied cells: the earlier one (4, 11) wins
    g[6, 0, 16 * 4 + 1, 16 * 11 + 15] = 40
    g[7] = 3
    g[7, 0, 200:, 200:] = 200                              # the last cell (and its neighbours)
    g[8, 0, 0:16, 16:32] = 255
    g[8, 0, 16:32, 0:16] = 255                             # equal full cells 1 and 14 -> 1
    got = H.cell_argmax_u8(_u8(g), 16).cpu().numpy()
    want = np.array([V.cell_argmax(x[0]) for x in g])
    assert np.array_equal(got, want)
    assert got[5] == 0 and got[6] == 4 * 14 + 11 and got[8] == 1
    # a grid with a remainder (AvgPool2d drops it): 40 x 50 with cell 16 -> 2 x 3 cells
    h = rs.randint(0, 256, size=(3, 40, 50)).astype(np.uint8)
    h[:, 32:, :] = 255
    h[:, :, 48:] = 255
    assert np.array_equal(H.cell_argmax_u8(_u8(h), 16).cpu().numpy(), [V.cell_argmax(x) for x in h])


# ----------------------------------------------------------------------------- model side
def _models():
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    from oracle import synth

    def shapes(m):
        return {k: tuple(v.shape) for k, v in m.state_dict().items()}
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    model.load_state_dict(synth.synth_state_dict(shapes(model), seed=1, head_gain=0.25))
    lstm = lstmnet()
    lstm.load_state_dict(synth.synth_state_dict(shapes(lstm), seed=2))
    return model.to(DEV), lstm.to(DEV)


@pytest.mark.gpu
def test_driver_features_are_the_hooked_full_forward(monkeypatch, tmp_path):
    """The spatial encoder run alone is not bit-identical to the features_s a full model_SP forward hooks (DESIGN.md section
    12), so the driver runs the full forward and hooks it: the map its crop sees is that hooked output, bit for bit."""
    from egaze_amd import hipops as H
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    from egaze_amd.functions import to_nhwc
    from egaze_amd.vis_features import vis_features
    model, lstm = _models()
    model.eval()
    inp = V.synth_inputs(21, 4)
    seen = []
    handle = model.features_s.register_forward_hook(lambda m, i, o: seen.append(to_nhwc(o).clone()))
    with torch.no_grad():
        model(H.u8_normalize(_u8(inp['image']), IMAGE_MEAN, IMAGE_STD), H.u8_normalize(_u8(inp['flow']), FLOW_MEAN, FLOW_STD))
    handle.remove()
    got = []
    mean_fn = H.window_mean
    monkeypatch.setattr(H, "window_mean", lambda feat, win: (got.append(feat.clone()), mean_fn(feat, win))[1])
    loader = [{'image': torch.from_numpy(inp['image']), 'flow': torch.from_numpy(inp['flow']),
               'gt': torch.from_numpy(inp['gt']), 'fixsac': torch.zeros(4, 1), 'imname': ["a%d.jpg" % k for k in range(4)]}]
    vis_features(loader, model, lstm, str(tmp_path), first=0, lut=V.random_lut(1), writer=lambda p, a: None)
    assert len(seen) == 1 and len(got) == 1 and got[0].shape == (4, 14, 14, 512)
    assert torch.equal(seen[0], got[0])
    assert not model.features_s._forward_hooks                # the driver's hook is gone again


def _golden_loader(inp, names, B):
    loader = [None] * 100
    for b in range(len(names) // B):
        s = slice(b * B, (b + 1) * B)
        loader.append({'image': torch.from_numpy(inp['image'][s]), 'flow': torch.from_numpy(inp['flow'][s]),
                       'gt': torch.from_numpy(inp['gt'][s]), 'fixsac': torch.zeros(B, 1), 'imname': names[s]})
    return loader


@pytest.mark.gpu
def test_vis_features_against_reference_golden(monkeypatch, tmp_path):
    from egaze_amd import hipops as H
    from egaze_amd.vis_features import vis_features
    gold = np.load(GOLDEN)
    B, NB = 2, 3
    inp = V.synth_inputs(11, B * NB)
    names = ["Alireza_f%02d.jpg" % k for k in range(B * NB)]
    lut = gold['lut']
    assert np.array_equal(lut, V.random_lut(11))
    model, lstm = _models()

    rec = {'cells': [], 'means': [], 'maps': [], 'lstm': []}
    cell_fn, mean_fn, ov_fn = H.cell_argmax_u8, H.window_mean, H.heatmap_overlay

    def cells(gt, cell=16):
        r = cell_fn(gt, cell)
        rec['cells'] += r.cpu().tolist()
        return r

    def means(feat, windows):
        r = mean_fn(feat, windows)
        rec['means'].append(r.cpu().numpy())
        return r

    def overlays(maps, frames, fi, lut_):
        rec['maps'].append(maps.cpu().numpy())
        return ov_fn(maps, frames, fi, lut_)
    monkeypatch.setattr(H, "cell_argmax_u8", cells)
    monkeypatch.setattr(H, "window_mean", means)
    monkeypatch.setattr(H, "heatmap_overlay", overlays)
    lstm.register_forward_hook(lambda m, a, o: rec['lstm'].append(o[0].detach().reshape(-1, 512).cpu().numpy()))
    written = {}
    vis_features(_golden_loader(inp, names, B), model, lstm, str(tmp_path), lut=lut,
                 writer=lambda p, a: written.__setitem__(os.path.basename(p), np.array(a, copy=True)))

    # cells and windows exact
    assert rec['cells'] == gold['cells'].tolist()
    # window means and LSTM outputs close to the reference's CPU fp32 (different summation order in the encoder)
    for key, gkey in (('means', 'window_mean'), ('lstm', 'lstm_out')):
        got, want = np.concatenate(rec[key]), gold[gkey]
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < 1e-4, (key, err)
    # the 14 x 14 maps: +-1 LSB on < 2 % of the cells (np.uint8(255 x) truncation next to an integer)
    maps = np.concatenate(rec['maps'])
    assert maps.shape == gold['maps14'].shape
    d = maps.astype(int) - gold['maps14']
    assert np.abs(d).max() <= 1 and np.count_nonzero(d) < 0.02 * d.size, (np.abs(d).max(), np.count_nonzero(d))
    # every overlay: the restatement applied to the port's own map; equal to the reference wherever the maps agree
    map_names = bytes(gold['map_names']).decode().split("\n")
    digests = dict(line.split(" ") for line in bytes(gold['digests']).decode().split("\n"))
    assert sorted(written) == sorted(map_names + ['gaze_' + names[b * B] for b in range(NB)])
    agreeing = 0
    for k, n in enumerate(map_names):
        frame = inp['image'][names.index(n.split('_', 1)[1])]
        assert np.array_equal(written[n], V.overlay(maps[k], frame, lut)), n
        if np.array_equal(maps[k], gold['maps14'][k]):
            agreeing += 1
            assert V.digest(written[n]) == digests[n], n
            if n.endswith(names[(NB - 1) * B]):
                assert np.array_equal(written[n], gold['full_' + n.split('_')[0]])
    assert agreeing >= len(map_names) // 2
    for b in range(NB):
        assert np.array_equal(written['gaze_' + names[b * B]], gold['gaze'][b])


# ----------------------------------------------------------------------------- CLI on a synthetic GTEA tree
def _tree(root, n=6, val="Alireza"):
    from PIL import Image
    inp = V.synth_inputs(31, n)
    folder = val + "_Pizza"
    p = {k: root / k for k in ("gtea_imgflow", "gtea_images", "gtea_gts", "fixsac")}
    for d in p.values():
        d.mkdir()
    (p["gtea_imgflow"] / folder).mkdir()
    rs = np.random.RandomState(32)
    for num in range(1, 10 + n):
        for ax in "xy":
            Image.fromarray(rs.randint(100, 156, size=(224, 224)).astype(np.uint8)).save(
                p["gtea_imgflow"] / folder / ("flow_%s_%05d.jpg" % (ax, num)), quality=90)
    for k in range(n):
        num = 10 + k
        Image.fromarray(inp['image'][k].transpose(1, 2, 0)[:, :, ::-1]).save(
            p["gtea_images"] / ("%s_img_%05d.jpg" % (folder, num)), quality=95)
        Image.fromarray(inp['gt'][k, 0]).save(p["gtea_gts"] / ("%s_img_gt_%05d.png" % (folder, num)))
    (p["fixsac"] / (val + "_Pizza.txt")).write_text("\n".join(str(k % 2) for k in range(n)) + "\n")
    return {k: str(v) for k, v in p.items()}


def _weights(root):
    model, lstm = _models()
    mp, lp = str(root / "sp.pth.tar"), str(root / "lstm.pth.tar")
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, mp)
    torch.save({'state_dict': {k: v.cpu() for k, v in lstm.state_dict().items()}}, lp)
    return mp, lp


def _run_cli(p, mp, lp, out, *extra):
    from egaze_amd.vis_features import main
    main(["--flowPath", p["gtea_imgflow"], "--imagePath", p["gtea_images"], "--gtPath", p["gtea_gts"], "--fixsacPath",
          p["fixsac"], "--batch_size", "2", "--trained_model", mp, "--trained_lstm", lp, "--savefolder", out,
          "--first", "1", "--last", "2", *extra])
    return sorted(os.listdir(out))


@pytest.mark.gpu
def test_cli_end_to_end_host_and_gpu_decode(tmp_path):
    from PIL import Image
    p = _tree(tmp_path)
    mp, lp = _weights(tmp_path)
    frames = ["Alireza_Pizza_img_%05d.jpg" % (10 + k) for k in range(6)]
    files = _run_cli(p, mp, lp, str(tmp_path / "vis"))
    # batches 1 and 2 of 3 (rows 2 .. 5), row 0 of each: gt_, noweight_, gaze_ twice, pred_ from the second
    want = sorted([pre + frames[b] for b in (2, 4) for pre in ("gt_", "noweight_", "gaze_")] + ["pred_" + frames[4]])
    assert files == want
    files_all = _run_cli(p, mp, lp, str(tmp_path / "vis_all"), "--all_frames")
    assert len(files_all) == 2 * len(files)
    assert set(files) <= set(files_all) and "pred_" + frames[5] in files_all and "pred_" + frames[3] not in files_all
    files_gpu = _run_cli(p, mp, lp, str(tmp_path / "vis_gpu"), "--gpu_decode")
    assert files_gpu == files
    for f in files:
        a = np.asarray(Image.open(tmp_path / "vis" / f))
        b = np.asarray(Image.open(tmp_path / "vis_gpu" / f))
        assert a.shape == b.shape and np.array_equal(a, b), f
        assert a.shape == ((224, 224) if f.startswith("gaze_") else (224, 224, 3))


@pytest.mark.gpu
def test_frames_of_another_size_raise(tmp_path):
    from egaze_amd.vis_features import vis_features
    model, lstm = _models()
    inp = V.synth_inputs(41, 2, hw=160)
    loader = [{'image': torch.from_numpy(inp['image']), 'flow': torch.from_numpy(inp['flow']),
               'gt': torch.from_numpy(inp['gt']), 'fixsac': torch.zeros(2, 1), 'imname': ["a.jpg", "b.jpg"]}]
    with pytest.raises(ValueError, match="224"):
        vis_features(loader, model, lstm, str(tmp_path), first=0, writer=lambda p, a: None)
