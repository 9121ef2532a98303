"""egaze_amd.predict on the GPU: a 14-frame synthetic video through VideoPredictor and the CLI.  The network inputs against the
training path's (extract_flow files -> STDataset -> stage_batch), steps 1 - 7 against their restatement as public ops at the same
chunking, the three fixation modes, the JPEG hand-over, another frame size with overlays and maps, the CLI's files."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 14                                            # frames 0 .. 13 (file numbers 1 .. 14): predictable 9 .. 12
CHUNK = 3                                         # one full and one partial chunk


# ----------------------------------------------------------------------------- fixtures
def _texture(y, x, rng_seed=7):
    """A smooth seeded pattern with a finer octave on top, sampled bilinearly at real positions (y, x) -> (len y, len x, 3)."""
    rng = np.random.RandomState(rng_seed)
    out = 0.0
    for cells, period, gain in ((40, 16.0, 0.7), (90, 5.0, 0.3)):
        grid = rng.rand(cells, cells, 3)
        gy, gx = y / period, x / period
        y0, x0 = np.floor(gy).astype(int), np.floor(gx).astype(int)
        fy, fx = (gy - y0)[:, None, None], (gx - x0)[None, :, None]
        a, b = grid[y0][:, x0], grid[y0][:, x0 + 1]
        c, d = grid[y0 + 1][:, x0], grid[y0 + 1][:, x0 + 1]
        out = out + gain * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)
    return np.clip(np.rint(out * 255), 0, 255).astype(np.uint8)


def _write_video(folder, hw, nframes=F):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    H, W = hw
    for k in range(nframes):                      # the pattern moves by (0.7, 1.3) pixels of a 224-frame per frame
        y = (np.arange(H) * 224.0 / H) + 8 + 0.7 * k
        x = (np.arange(W) * 224.0 / W) + 8 + 1.3 * k
        Image.fromarray(_texture(y, x)).save(os.path.join(folder, "img_%05d.jpg" % (k + 1)), quality=95)
    return folder


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("predict")


@pytest.fixture(scope="module")
def video(root):
    return _write_video(str(root / "frames" / "vid"), (224, 224))


@pytest.fixture(scope="module")
def weights(root):
    """Seeded random-initialised SP / LSTM / LF checkpoints in the layouts SP.py, AT.py and LF.py save."""
    from oracle import synth
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sp, lstm, late = str(root / "best_SP.pth.tar"), str(root / "best_lstm.pth.tar"), str(root / "best_late.pth.tar")
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    torch.save({'state_dict': synth.synth_state_dict(shapes(model), seed=1, head_gain=0.25)}, sp)
    torch.save(synth.synth_state_dict(shapes(lstmnet()), seed=2), lstm)
    torch.save({'state_dict': synth.synth_state_dict(shapes(late_fusion()), seed=3, head_gain=0.25)}, late)
    return sp, lstm, late


@pytest.fixture(scope="module")
def models(weights):
    from egaze_amd.predict import load_models
    return load_models(*weights[:1], weights[2], weights[1], torch.device(DEV))


@pytest.fixture(scope="module")
def flag_file(root):
    """After STDataset's dilation the frames 9 .. 12 are fixation, saccade, saccade, fixation."""
    a = np.zeros(F)
    a[[8, 13]] = 1
    path = str(root / "fixsac.txt")
    np.savetxt(path, a)
    from egaze_amd.predict import dilate_fixsac
    assert dilate_fixsac(a)[9:13].tolist() == [1.0, 0.0, 0.0, 1.0]
    return path


def _run(models, video, **kw):
    from egaze_amd.predict import VideoPredictor
    model, lstm, late = models
    if kw.get('fixsac', 'all') == 'all':
        lstm = kw.pop('lstm', None)
    kw.setdefault('chunk', CHUNK)
    pred = VideoPredictor(model, lstm, late, keep=True, **kw)
    try:
        return pred.run(video)
    finally:
        pred.close()


def _csv(path):
    lines = open(path).read().splitlines()
    conv = lambda v: None if v == '' else float(v)
    return lines[0], [[conv(v) for v in line.split(',')] for line in lines[1:]]


def _all_frames_and_flows(video, flow_jpeg):
    """The whole video at once with the public ops: BGR planes (F, 3, 224, 224) and flow planes (F - 1, 2, 224, 224) uint8."""
    from egaze_amd import hipops as H
    from egaze_amd.data.extract_flow import decode_frames, flow_images, list_frames
    files = [os.path.join(video, name) for _, name in list_frames(video)]
    bgr = decode_frames(files, (224, 224), DEV)
    u8 = flow_images(bgr, 20.0, {})                                           # (2, F - 1, H, W)
    if flow_jpeg:
        data, off, st = H.jpeg_encode(u8.reshape(-1, 224, 224), quality=flow_jpeg)
        dec, st2 = H.jpeg_decode(data, off, (224, 224), [1] * (2 * (F - 1)), n3=0)
        assert not int(st.abs().max()) and not int(st2.abs().max())
        u8 = dec.view(2, F - 1, 224, 224)
    return bgr, u8.permute(1, 0, 2, 3).contiguous()


# ----------------------------------------------------------------------------- network inputs
@pytest.fixture(scope="module")
def file_run(models, video, flag_file):
    return _run(models, video, fixsac=flag_file)


def test_network_inputs_equal_the_training_path(root, video, file_run):
    """extract_flow's files read back by STDataset(raw_u8=True) and normalised by stage_batch: what SP / AT train on."""
    from egaze_amd.data import extract_flow
    from egaze_amd.data.STdatas import STDataset, stage_batch
    flow_dir, img_dir, gt_dir, fs_dir = (str(root / d) for d in ("flow", "img", "gt", "fs"))
    assert extract_flow.main(["--framePath", os.path.dirname(video), "--flowPath", flow_dir]) == 2 * (F - 1)
    names, gts = [], []
    for d in (img_dir, gt_dir, fs_dir):
        os.makedirs(d, exist_ok=True)
    for k in range(9, F - 1):                                                 # frame index k has file number k + 1
        names.append("vid_img_%05d.jpg" % (k + 1))
        gts.append("vid_000000_%05d.jpg" % (k + 1))
        shutil.copy(os.path.join(video, "img_%05d.jpg" % (k + 1)), os.path.join(img_dir, names[-1]))
        shutil.copy(os.path.join(video, "img_%05d.jpg" % (k + 1)), os.path.join(gt_dir, gts[-1]))      # a dummy ground truth
    np.savetxt(os.path.join(fs_dir, "a.txt"), np.zeros(len(names)))
    ds = STDataset(flow_dir, img_dir, gt_dir, ["vid"], names, gts, ["a.txt"], fs_dir, raw_u8=True)
    assert len(ds) == len(file_run) == F - 10
    for i, rec in enumerate(file_run):
        s = ds[i]
        image, flow, _ = stage_batch({k: s[k].unsqueeze(0) for k in ('image', 'flow', 'gt')}, DEV)
        assert rec['index'] == 9 + i and rec['frame'] == 10 + i and rec['name'] == "img_%05d.jpg" % (10 + i)
        assert torch.equal(rec['image'], image[0]), i
        assert torch.equal(rec['flow'], flow[0]), i


def test_without_the_flow_jpeg_the_inputs_are_the_unencoded_flow_images(models, video):
    from egaze_amd import hipops as H
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    recs = _run(models, video, flow_jpeg=0)
    bgr, flows = _all_frames_and_flows(video, 0)
    for rec in recs:
        k = rec['index']
        stack = torch.stack([flows[k - m, c] for m in range(10) for c in range(2)])
        assert torch.equal(rec['flow'], H.u8_normalize(stack.unsqueeze(0), FLOW_MEAN, FLOW_STD)[0]), k
        assert torch.equal(rec['image'], H.u8_normalize(bgr[k:k + 1], IMAGE_MEAN, IMAGE_STD)[0]), k
    with_jpeg = _run(models, video)
    assert not torch.equal(with_jpeg[0]['flow'], recs[0]['flow'])             # the round trip does change the bytes


# ----------------------------------------------------------------------------- the chain
def _restate(models, video, flags, chunk, flow_jpeg=95):
    """Steps 1 - 7 of the predictor as a composition of public ops, at the same chunking, over a pool of the WHOLE video."""
    from egaze_amd import hipops as H
    from egaze_amd.functions import to_nhwc
    from egaze_amd.utils import repackage_hidden
    model, lstm, late = models
    bgr, flows = _all_frames_and_flows(video, flow_jpeg)
    pool = torch.cat((bgr.reshape(-1, 224, 224), flows.reshape(-1, 224, 224)))       # frame k at 3 k, flow i at 3 F + 2 i
    table = torch.tensor([[3 * k] + [3 * F + 2 * (k - m) + c for m in range(10) for c in range(2)] + [-1]
                          for k in range(F)], dtype=torch.int64, device=DEV)
    feats = []
    hook = model.features_s.register_forward_hook(lambda mod, i, o: feats.append(o))
    hidden, out_all = None, []
    try:
        with torch.no_grad():
            for k0 in range(9, F - 1, chunk):
                ks = list(range(k0, min(k0 + chunk, F - 1)))
                n = len(ks)
                image, flow, _ = H.resident_gather(pool, table, torch.tensor(ks, device=DEV), fields=('image', 'flow'))
                del feats[:]
                out = model(image, flow)                                                      # 1
                fn = to_nhwc(feats[-1])
                com_sp, gp, q_sp = H.u8_center_of_mass(out.reshape(n, 224, 224), want_u8=True)          # 2
                rows = H.crop_mean(fn, gp, 3, 16)                                             # 3
                sacc = [i for i, k in enumerate(ks) if int(flags[k]) != 1]                    # 4, 5
                if sacc:
                    sel = torch.tensor(sacc, device=DEV)
                    hidden = repackage_hidden(hidden)
                    seq, hidden = lstm(rows.index_select(0, sel).unsqueeze(1), hidden)
                    rows = rows.index_copy(0, sel, seq.squeeze(1))
                at = H.weighted_minmax(fn, rows)                                              # 6
                fused, planes = H.late_input(q_sp, at, want_u8=True, status_to={})
                fin = late.fusion(fused, fuse_sigmoid=True)                                   # 7
                com, _, q_fin = H.u8_center_of_mass(fin.reshape(n, 224, 224), want_u8=True)
                for i in range(n):
                    out_all.append(dict(out=out[i], at=at[i], fused=fused[i], fin=fin[i], com=com[i].cpu().tolist(),
                                        com_sp=com_sp[i].cpu().tolist(), q_fin=q_fin[i], sacc=i in sacc))
    finally:
        hook.remove()
    return out_all


@pytest.mark.parametrize("chunk", [CHUNK, 2])
def test_chain_equals_its_restatement(models, video, flag_file, root, chunk):
    """chunk 3: frames 9 10 11 | 12, both LSTM steps in one call; chunk 2: frames 9 10 | 11 12, the second step starts from the
    state the first chunk left."""
    from egaze_amd.predict import load_fixsac
    outdir = str(root / f"chain{chunk}")
    recs = _run(models, video, fixsac=flag_file, chunk=chunk, out=outdir)
    flags = load_fixsac(flag_file, F)
    want = _restate(models, video, flags, chunk)
    header, rows = _csv(os.path.join(outdir, "gaze.csv"))
    assert header == "frame,row,col,x,y,fixation,sp_row,sp_col"
    assert [r['fixation'] for r in recs] == [1, 0, 0, 1] and [w['sacc'] for w in want] == [False, True, True, False]
    assert len(recs) == len(want) == len(rows) == 4
    for rec, w, row in zip(recs, want, rows):
        for key in ('out', 'at', 'fused', 'fin', 'q_fin'):
            assert torch.equal(rec[key], w[key]), (rec['index'], key)
        assert [rec['row'], rec['col']] == w['com'] and [rec['sp_row'], rec['sp_col']] == w['com_sp']
        assert (rec['x'], rec['y']) == ((rec['col'] + 0.5) * 224 / 224 - 0.5, (rec['row'] + 0.5) * 224 / 224 - 0.5)
        assert (rec['x'], rec['y']) == pytest.approx((rec['col'], rec['row']), abs=1e-12)       # 224 x 224 frames: the identity
        assert row == [rec['frame'], rec['row'], rec['col'], rec['x'], rec['y'], rec['fixation'], rec['sp_row'], rec['sp_col']]
    # the saccade frames went through the LSTM: their AT maps differ from what their own crop means give
    plain = _restate(models, video, np.ones(F), chunk)
    assert torch.equal(plain[0]['at'], want[0]['at']) and not torch.equal(plain[1]['at'], want[1]['at'])
    assert not torch.equal(plain[2]['at'], want[2]['at'])


def test_all_mode_needs_no_lstm_and_equals_an_all_ones_file(models, video, root):
    ones = str(root / "ones.txt")
    np.savetxt(ones, np.ones(F))
    a = _run(models, video)                                                       # lstm=None
    b = _run(models, video, fixsac=ones)
    assert [r['fixation'] for r in a] == [r['fixation'] for r in b] == [1] * 4
    for ra, rb in zip(a, b):
        for key in ('out', 'at', 'fused', 'fin'):
            assert torch.equal(ra[key], rb[key])
        assert all(ra[key] == rb[key] for key in ('row', 'col', 'x', 'y', 'sp_row', 'sp_col', 'frame'))
    from egaze_amd.predict import VideoPredictor
    with pytest.raises(ValueError, match="lstm is None"):
        VideoPredictor(models[0], None, models[2], fixsac='auto')


@pytest.mark.parametrize("radius", [17.5, 1e-3, 1e3])
def test_auto_mode_runs_the_online_rule_on_its_own_gaze_points(models, video, radius):
    from egaze_amd.predict import OnlineFixation
    a = _run(models, video, fixsac='auto', fix_radius=radius)
    rule = OnlineFixation(radius)
    assert [r['fixation'] for r in a] == [rule.step(r['sp_col'], r['sp_row']) for r in a]
    assert a[0]['fixation'] == 0                                                  # the first predictable frame: a saccade
    if radius == 1e3:
        assert [r['fixation'] for r in a] == [0, 1, 1, 1]
    b = _run(models, video, fixsac='auto', fix_radius=radius)
    for ra, rb in zip(a, b):
        assert torch.equal(ra['fin'], rb['fin']) and torch.equal(ra['at'], rb['at'])
        assert all(ra[key] == rb[key] for key in ('row', 'col', 'sp_row', 'sp_col', 'fixation'))


def test_handover_jpeg(models, video, file_run, flag_file):
    from egaze_amd import hipops as H
    recs = _run(models, video, fixsac=flag_file, handover_jpeg=95)
    out = torch.stack([r['out'] for r in recs])
    at = torch.stack([r['at'] for r in recs])
    for r, base in zip(recs, file_run):                                           # nothing upstream of the hand-over moves
        assert torch.equal(r['out'], base['out']) and torch.equal(r['at'], base['at'])
    _, _, q_sp = H.u8_center_of_mass(out.reshape(4, 224, 224), want_u8=True)
    _, planes = H.late_input(q_sp, at, want_u8=True, status_to={})
    data, off, st = H.jpeg_encode(planes.view(8, 224, 224), quality=95)
    dec, st2 = H.jpeg_decode(data, off, (224, 224), [1] * 8, n3=0)
    assert not int(st.abs().max()) and not int(st2.abs().max())
    dec = dec.view(4, 2, 224, 224)
    want = H.late_input(dec[:, 1].contiguous(), dec[:, 0].contiguous(), status_to={})
    assert torch.equal(torch.stack([r['fused'] for r in recs]), want)
    assert not torch.equal(want, torch.stack([r['fused'] for r in file_run]))


# ----------------------------------------------------------------------------- another frame size, overlays, maps
def test_other_frame_size_overlays_and_maps(models, root):
    from PIL import Image
    from egaze_amd import hipops as H
    from egaze_amd.data.extract_flow import decode_frames, list_frames
    from egaze_amd.predict import ring_radii
    H0, W0 = 96, 128
    video = _write_video(str(root / "small" / "vid"), (H0, W0))
    outdir = str(root / "small_out")
    recs = _run(models, video, overlay=True, save_maps=True, out=outdir)
    _, rows = _csv(os.path.join(outdir, "gaze.csv"))
    assert sorted(os.listdir(outdir)) == sorted(["gaze.csv"] + ["pred_img_%05d.jpg" % n for n in range(10, 14)] +
                                                ["gaze_img_%05d.jpg" % n for n in range(10, 14)])
    centers = []
    for rec, row in zip(recs, rows):
        assert rec['x'] == (rec['col'] + 0.5) * W0 / 224 - 0.5 and rec['y'] == (rec['row'] + 0.5) * H0 / 224 - 0.5
        assert row[1:5] == [rec['row'], rec['col'], rec['x'], rec['y']]
        assert 0 <= rec['x'] <= W0 - 1 and 0 <= rec['y'] <= H0 - 1
        centers.append([int(np.rint(rec['y'])), int(np.rint(rec['x']))])
    files = [os.path.join(video, name) for _, name in list_frames(video)]
    frames = decode_frames(files, None, DEV)
    assert tuple(frames.shape) == (F, 3, H0, W0)
    q_fin = torch.stack([r['q_fin'] for r in recs])
    over = H.heatmap_overlay(q_fin, frames, [r['index'] for r in recs], H.jet_lut(DEV))
    plain = over.clone()
    assert ring_radii(H0) == (3, 4)
    H.draw_ring(over, torch.tensor(centers, dtype=torch.int32, device=DEV), 3, 4, (255, 255, 255))
    assert not torch.equal(over, plain)                                           # the marker is inside the frame
    for images, fmt in ((over, "gaze_img_%05d.jpg"), (q_fin, "pred_img_%05d.jpg")):
        data, off, _ = H.jpeg_encode(images, quality=95)
        data, off = data.cpu().numpy(), off.cpu().tolist()
        for i, rec in enumerate(recs):
            path = os.path.join(outdir, fmt % rec['frame'])
            assert open(path, 'rb').read() == data[off[i]:off[i + 1]].tobytes(), path
            size = Image.open(path).size
            assert size == ((W0, H0) if fmt.startswith("gaze") else (224, 224))


# ----------------------------------------------------------------------------- the CLI
def test_cli_end_to_end(weights, video, flag_file, root, capsys):
    from egaze_amd.predict import main
    sp, lstm, late = weights
    for mode in ("all", "file"):
        outdir = str(root / ("cli_" + mode))
        extra = [] if mode == "all" else ["--fixsac", flag_file, "--trained_lstm", lstm]
        recs = main(["--framePath", video, "--trained_model", sp, "--trained_late", late, "--out", outdir, "--chunk", "3"] + extra)
        assert os.listdir(outdir) == ["gaze.csv"]
        header, rows = _csv(os.path.join(outdir, "gaze.csv"))
        assert header == "frame,row,col,x,y,fixation,sp_row,sp_col"
        assert len(rows) == len(recs) == F - 10 and [r[0] for r in rows] == [10, 11, 12, 13]
        assert [r[5] for r in rows] == ([1, 1, 1, 1] if mode == "all" else [1, 0, 0, 1])
        assert all(len(r) == 8 and None not in r for r in rows)
    short = str(root / "short" / "vid")
    os.makedirs(short)
    for n in range(1, 11):                                                        # F = 10: one frame too few
        shutil.copy(os.path.join(video, "img_%05d.jpg" % n), short)
    with pytest.raises(SystemExit) as e:
        main(["--framePath", short, "--trained_model", sp, "--trained_late", late, "--out", str(root / "cli_short")])
    assert "10 frames" in str(e.value) and "at least 11 frames" in str(e.value)
    assert not os.path.exists(str(root / "cli_short"))
