"""hipops.jpeg_encode (csrc/jpeg_encode.hip) against Pillow's (libjpeg-turbo's default) encoder, whole file, byte for byte: the
fixture, the host core on a random set, the batches the drivers really make, slot isolation and the too-small-capacity status,
argument errors, the round trip through hipops.jpeg_decode, and the drivers' --gpu-encode / --gpu_encode end to end."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_enc_host import first_diff, fixture, host_encode, pil_encode, random_cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _files(enc):
    """(data, offsets, status) of jpeg_encode -> list of bytes; every status must be 0."""
    data, off, status = enc
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * status.numel()
    buf, o = data.cpu().numpy().tobytes(), off.cpu().tolist()
    assert o[0] == 0 and o[-1] == len(buf) and len(o) == status.numel() + 1
    return [buf[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def test_fixture_byte_for_byte():
    from egaze_amd import hipops as H
    groups = {}
    for c in fixture():
        groups.setdefault((c["pixels"].shape, c["quality"]), []).append(c)
    assert len(groups) > 20
    for (shape, q), group in groups.items():
        x = torch.from_numpy(np.stack([c["pixels"] for c in group])).to(DEV)
        got = _files(H.jpeg_encode(x, quality=q))
        for c, g in zip(group, got):
            assert g == c["expect"], (c["name"], len(g), len(c["expect"]), first_diff(g, c["expect"]))


def test_random_images_equal_the_host_core():
    from egaze_amd import hipops as H
    imgs = random_cases()
    ref = host_encode(imgs)                                # itself byte-identical with Pillow (tests/test_jpeg_enc_host.py)
    for (a, q), (need, want) in zip(imgs, ref):
        got = _files(H.jpeg_encode(torch.from_numpy(a[None]).to(DEV), quality=q))[0]
        assert got == want, (a.shape, q, len(got), need, first_diff(got, want))


def test_batch_of_4096_gaze_maps_equals_pillow_per_image():
    from egaze_amd import hipops as H
    rng = np.random.default_rng(5)
    n = 4096
    rows = torch.from_numpy(rng.integers(0, 960, n).astype(np.int32)).to(DEV)
    cols = torch.from_numpy(rng.integers(0, 1280, n).astype(np.int32)).to(DEV)
    u8, _, _ = H.gaze_gt_maps(rows, cols, (960, 1280), 70.0, (224, 224), mode=0)
    assert u8.shape == (n, 224, 224)
    got = _files(H.jpeg_encode(u8, quality=95))
    maps = u8.cpu().numpy()
    for i in range(n):
        want = pil_encode(maps[i], 95)
        assert got[i] == want, (i, len(got[i]), len(want), first_diff(got[i], want))


def test_batch_of_30_overlays_equals_pillow_per_image():
    from egaze_amd import hipops as H
    rng = np.random.default_rng(6)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_jpeg import content
    frames = np.ascontiguousarray(np.stack([content(224, 224, 50 + k).transpose(2, 0, 1) for k in range(10)]))
    maps = torch.from_numpy(rng.integers(0, 256, (30, 14, 14), dtype=np.uint8)).to(DEV)
    ov = H.heatmap_overlay(maps, torch.from_numpy(frames).to(DEV), [k % 10 for k in range(30)], H.jet_lut(torch.device(DEV)))
    assert ov.shape == (30, 224, 224, 3)
    got = _files(H.jpeg_encode(ov, quality=95))
    arr = ov.cpu().numpy()
    for i in range(30):
        want = pil_encode(arr[i], 95)
        assert got[i] == want, (i, len(got[i]), len(want), first_diff(got[i], want))


def _mixed_batch():
    cases = {c["name"]: c for c in fixture()}
    names = ["gray_noise_40x56_q95", "gray_noise_40x56_q50", "gray_noise_40x56_q100", "gray_noise_40x56_q1"]
    px = np.stack([cases[n]["pixels"] for n in names])
    want = [pil_encode(p, 95) for p in px]
    return px, want


def test_slots_are_isolated_by_sentinels():
    from egaze_amd import hipops as H
    px, want = _mixed_batch()
    gap, n = 64, len(want)
    offs, p = [], gap
    for w in want:
        offs.append(p)
        p += len(w) + gap
    out = torch.full((p,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths, status = H.jpeg_encode_into(torch.from_numpy(px).to(DEV), out, offs, [len(w) for w in want], quality=95)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and lengths.cpu().tolist() == [len(w) for w in want]
    o = out.cpu().numpy()
    expect = np.full(p, 0xA5, np.uint8)
    for off, w in zip(offs, want):
        expect[off:off + len(w)] = np.frombuffer(w, np.uint8)
    assert np.array_equal(o, expect)                       # every file in its slot, every byte between the slots untouched


def test_too_small_capacity_reports_needed_length_and_writes_nothing():
    from egaze_amd import hipops as H
    px, want = _mixed_batch()
    n = len(want)
    slot = max(len(w) for w in want) + 32
    caps = [len(want[0]), len(want[1]) - 1, 10, 0]
    out = torch.full((n * slot,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths, status = H.jpeg_encode_into(torch.from_numpy(px).to(DEV), out, [i * slot for i in range(n)], caps, quality=95)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 1, 1, 1]
    assert lengths.cpu().tolist() == [len(w) for w in want]                # the length each file needs
    o = out.cpu().numpy()
    assert o[:len(want[0])].tobytes() == want[0]
    assert (o[len(want[0]):] == 0xA5).all()
    # a slot that fits its capacity but leaves the buffer is refused too
    out2 = torch.full((len(want[0]) + 5,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths, status = H.jpeg_encode_into(torch.from_numpy(px[:1]).to(DEV), out2, [6], [len(want[0])], quality=95)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1] and lengths.cpu().tolist() == [len(want[0])]
    assert (out2.cpu().numpy() == 0xA5).all()


def test_argument_errors():
    from egaze_amd import hipops as H
    from egaze_amd._lib import EgazeHipError, LIB
    g = torch.zeros((2, 16, 16), dtype=torch.uint8, device=DEV)
    c = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.jpeg_encode(g.cpu())
    with pytest.raises(ValueError, match="quality"):
        H.jpeg_encode(g, quality=0)
    with pytest.raises(ValueError, match="quality"):
        H.jpeg_encode(g, quality=101)
    with pytest.raises(ValueError, match="layout"):
        H.jpeg_encode(c, layout="rgb")
    with pytest.raises(ValueError, match="layout"):
        H.jpeg_encode(c, layout="gray")
    with pytest.raises(ValueError, match="layout"):
        H.jpeg_encode(torch.zeros((2, 3, 16, 16), dtype=torch.uint8, device=DEV))
    for sub in ("444", "422", 0):
        with pytest.raises(ValueError, match="subsampling"):
            H.jpeg_encode(c, subsampling=sub)
    with pytest.raises(ValueError, match="uint8"):
        H.jpeg_encode(g.float())
    with pytest.raises(ValueError, match="4096"):
        H.jpeg_encode(torch.zeros((1, 1, 4097), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="slot_offsets"):
        H.jpeg_encode_into(g, torch.zeros(4096, dtype=torch.uint8, device=DEV), [0], [100, 100])
    # the C entry points refuse the same with the library's error code
    nb = LIB.egz_jpeg_encode_ws_bytes(2, 16, 16, 1)
    assert nb > 0 and LIB.egz_jpeg_encode_ws_bytes(2, 0, 16, 1) == 0 and LIB.egz_jpeg_encode_ws_bytes(2, 16, 16, 2) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    need = torch.zeros(2, dtype=torch.int64, device=DEV)
    good = [g.data_ptr(), 2, 16, 16, 1, 95, 420, ws.data_ptr(), nb, need.data_ptr(), 4, None]
    for i, v in ((1, 0), (2, 0), (3, 4097), (4, 2), (5, 0), (5, 101), (6, 444), (8, nb - 1), (10, 5), (0, None)):
        a = list(good)
        a[i] = v
        with pytest.raises(EgazeHipError):
            H.check(LIB.egz_jpeg_encode(*a), "egz_jpeg_encode")
    H.check(LIB.egz_jpeg_encode(*good), "egz_jpeg_encode")
    torch.cuda.synchronize()
    assert need.cpu().tolist() == [len(pil_encode(np.zeros((16, 16), np.uint8), 95))] * 2


def test_round_trip_through_the_decoder_equals_pillow():
    from PIL import Image
    from egaze_amd import hipops as H
    cases = {c["name"]: c for c in fixture()}
    for name, ch in (("gray_224x224_q95", 1), ("bgr_224x224_q95", 3), ("bgr_225x223_q95", 3), ("bgr_17x31_q75", 3)):
        c = cases[name]
        x = torch.from_numpy(c["pixels"][None]).to(DEV)
        data, off, _ = H.jpeg_encode(x, quality=c["quality"])
        h, w = c["pixels"].shape[:2]
        u8, st = H.jpeg_decode(data, off, (h, w), [ch])
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0]
        im = Image.open(io.BytesIO(pil_encode(c["pixels"], c["quality"])))
        want = np.asarray(im)[None] if ch == 1 else np.asarray(im.convert("RGB"))[:, :, ::-1].transpose(2, 0, 1)
        assert np.array_equal(u8.cpu().numpy()[0], want), name


def test_dataset_preprocessing_gpu_encode_end_to_end(tmp_path):
    import test_dataset_prep_host as R
    import test_hip_gt_maps as G
    from egaze_amd.data import dataset_preprocessing as D
    gold = R._golden()
    videos = G._synthetic_tree(tmp_path, gold)
    src = {k: str(tmp_path / v) for k, v in (("gaze", "gtea_gaze"), ("flow", "gtea_imgflow"))}

    def run(tag, *extra):
        p = {k: str(tmp_path / (v + tag)) for k, v in (("img", "gtea_images"), ("gt", "gtea_gts"), ("fs", "fixsac"))}
        D.main(["--gazePath", src["gaze"], "--flowPath", src["flow"], "--imagePath", p["img"], "--gtPath", p["gt"],
                "--fixsacPath", p["fs"], "--workers", "4", *extra])
        return p
    a, b = run("_host"), run("_gpu", "--gpu-encode")
    for k in ("img", "gt", "fs"):
        assert sorted(os.listdir(a[k])) == sorted(os.listdir(b[k])) and os.listdir(a[k])
    for k in ("img", "fs"):                                # frame copies and label files: identical with and without the flag
        for f in os.listdir(a[k]):
            assert open(os.path.join(a[k], f), "rb").read() == open(os.path.join(b[k], f), "rb").read(), f
    n = 0
    for video in videos:
        gx, gy = gold[f"gplus_{video}_gazex"].tolist(), gold[f"gplus_{video}_gazey"].tolist()
        maps = D.render_maps(gx[1:], gy[1:])
        for i in range(1, len(gx)):
            got = open(os.path.join(b["gt"], f"{video}_gt_img_{i + 1:05d}.jpg"), "rb").read()
            want = pil_encode(maps[i - 1], 95)
            assert got == want, (video, i, first_diff(got, want))
            n += 1
    assert n == len(os.listdir(b["gt"])) and n > 0
    with pytest.raises(SystemExit):                        # argparse error
        run("_png", "--gpu-encode", "--gt-format", "png")


def test_vis_features_gpu_encode_end_to_end(tmp_path):
    import test_hip_vis as T
    import test_vis_host as V
    from egaze_amd.vis_features import vis_features
    model, lstm = T._models()
    inp = V.synth_inputs(51, 4)
    names = ["Alireza_f%02d.jpg" % k for k in range(4)]

    def loader():
        return [{'image': torch.from_numpy(inp['image'][s]), 'flow': torch.from_numpy(inp['flow'][s]),
                 'gt': torch.from_numpy(inp['gt'][s]), 'fixsac': torch.zeros(2, 1), 'imname': names[s]}
                for s in (slice(0, 2), slice(2, 4))]
    arrays = {}
    vis_features(loader(), model, lstm, str(tmp_path), first=0, all_frames=True,
                 writer=lambda p, a: arrays.__setitem__(os.path.basename(p), np.array(a, copy=True)))
    assert not os.listdir(tmp_path)
    out = tmp_path / "enc"
    out.mkdir()
    vis_features(loader(), model, lstm, str(out), first=0, all_frames=True, gpu_encode=True)
    assert sorted(os.listdir(out)) == sorted(arrays) and len(arrays) == 4 * 3 + 2
    for f, a in arrays.items():
        got = open(out / f, "rb").read()
        want = pil_encode(a, 95)
        assert got == want, (f, a.shape, first_diff(got, want))
    with pytest.raises(ValueError, match="writer"):
        vis_features(loader(), model, lstm, str(out), first=0, gpu_encode=True, writer=lambda p, a: None)
