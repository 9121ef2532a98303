"""hipops.jpeg_decode (csrc/jpeg_decode.hip) against the fixture's libjpeg-turbo decodes, its status words and slot isolation on
broken batches, and STDataset(decode='gpu') end to end against the host decode: staged tensors, one SP training step and one
extract_late chunk.  Broken inputs go through the sanitizer build of the same core (tests/test_jpeg_host.py) first."""
import os

import numpy as np
import pytest
import torch

from test_jpeg_host import broken_streams, fixture, host_decode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pack(streams):
    data = np.frombuffer(b"".join(streams), np.uint8) if any(len(s) for s in streams) else np.zeros(1, np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    return torch.from_numpy(data.copy()).to(DEV), torch.from_numpy(off)


def test_fixture_bit_exact():
    from egaze_amd import hipops as H
    cases, _ = fixture()
    by_size = {}
    for c in cases:
        by_size.setdefault((c["h"], c["w"]), []).append(c)
    for (h, w), group in by_size.items():
        data, off = _pack([c["data"] for c in group])
        u8, st = H.jpeg_decode(data, off, (h, w), [c["c"] for c in group])
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * len(group), [c["name"] for c in group]
        got = u8.cpu().numpy()
        for i, c in enumerate(group):
            assert np.array_equal(got[i, :c["c"]], c["expect"]), (c["name"], int((got[i, :c["c"]] != c["expect"]).sum()))


def test_broken_batch_status_and_slot_isolation():
    from egaze_amd import hipops as H
    cases, extra = fixture()
    good = [c for c in cases if (c["h"], c["w"]) == (224, 224)]
    g0, g1 = good[0], good[1]
    trunc = g1["data"][: len(g1["data"]) // 2]
    bad_soi = b"\x00" + g0["data"][1:]
    streams = [g0["data"], trunc, g1["data"], bad_soi, extra["progressive"], cases[-1]["data"], extra["png"]]
    chans = [g0["c"], g1["c"], g1["c"], g0["c"], 3, 3, 1]
    # the sanitizer build first: same inputs, and its output is what the GPU must write for the truncated stream
    ref = host_decode([(s, 224, 224, c) for s, c in zip(streams, chans)])
    assert [r[0] for r in ref] == [0, 1, 0, 4, 2, 3, 4]
    data, off = _pack(streams)
    # one plane of sentinel between every slot
    planes, p = [], 1
    for c in chans:
        planes.append(p)
        p += c + 1
    out = torch.full((p, 224, 224), 0xA5, dtype=torch.uint8, device=DEV)
    _, st = H.jpeg_decode(data, off, (224, 224), chans, out=out, planes=planes)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 1, 0, 4, 2, 3, 4]
    o = out.cpu().numpy()
    written = np.zeros(p, bool)
    for i, (pl, c) in enumerate(zip(planes, chans)):
        if ref[i][0] in (2, 3, 4):
            assert (o[pl:pl + c] == 0xA5).all(), i             # nothing written
        else:
            assert np.array_equal(o[pl:pl + c], ref[i][1]), i   # ok and padded-corrupt slots as the host core
            written[pl:pl + c] = True
    assert (o[~written] == 0xA5).all()


def test_fuzzed_streams_match_host_core():
    from egaze_amd import hipops as H
    cases, _ = fixture()
    br = [b for b in broken_streams(cases, flips=120) if (b[1], b[2]) == (225, 223)]
    ref = host_decode([b[:4] for b in br])
    data, off = _pack([b[0] for b in br])
    u8, st = H.jpeg_decode(data, off, (225, 223), [b[3] for b in br])
    torch.cuda.synchronize()
    st, u8 = st.cpu().tolist(), u8.cpu().numpy()
    for i, (s, img) in enumerate(ref):
        assert st[i] == s, i
        if s in (0, 1):
            assert np.array_equal(u8[i, :br[i][3]], img), i


def _loader(ds, B):
    from torch.utils.data import DataLoader
    return DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, pin_memory=True, collate_fn=ds.collate_fn)


def test_staged_batches_gpu_decode_matches_host(tmp_path):
    """decode='gpu' and decode='host' give bit-identical staged image / flow / gt (colour 4:2:0 and 4:4:4 frames, grayscale
    flow, JPEG and PNG ground truth, one progressive frame left to the host), then identical SP training steps; the
    batch-1 raw_u8 form AT.extract_late stages (to_raw_u8) matches the host bytes."""
    from test_jpeg_host import make_tree
    from egaze_amd.data.STdatas import STDataset, staged_batches, to_raw_u8
    args = make_tree(str(tmp_path))
    host = STDataset(*args, raw_u8=True)
    gpu = STDataset(*args, raw_u8=True, decode="gpu")
    dev = torch.device(DEV)
    a = [tuple(t.clone() for t in st) for _, st in staged_batches(_loader(host, 3), dev)]
    b = [tuple(t.clone() for t in st) for _, st in staged_batches(_loader(gpu, 3), dev)]
    torch.cuda.synchronize()
    assert len(a) == len(b) == 1
    for x, y in zip(a[0], b[0]):
        assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape
        assert torch.equal(x, y)
    for s_h, s_g in zip(_loader(host, 1), _loader(gpu, 1)):
        r = to_raw_u8(s_g, dev)
        for k in ("image", "flow", "gt"):
            assert torch.equal(r[k].cpu(), s_h[k]), k
    # one SP training step on each staged batch (synthetic weights, as smoke()): identical outputs and parameters
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import make_layers, cfg
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from oracle import egaze_oracle as O
    from oracle import synth
    sd = synth.synth_state_dict(O.sp_shapes(), seed=1, head_gain=0.25)
    res = []
    for x_s, x_t, gt in (a[0], b[0]):
        model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
        model.load_state_dict(sd)
        model.to(dev).train()
        opt = FusedAdam(model.parameters(), lr=1e-4)
        opt.zero_grad()
        out = model(x_s, x_t)
        loss = floss()(out, gt.view(out.size()))
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        res.append((out.detach().cpu(), [p.detach().cpu() for p in model.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(p, q) for p, q in zip(res[0][1], res[1][1]))


def test_staged_batches_reports_bad_files(tmp_path):
    """Status words reach the consumer at hand-over: a truncated frame warns naming the file, a frame of the wrong size
    raises naming the file."""
    from test_jpeg_host import fixture, make_tree
    from egaze_amd.data.STdatas import STDataset, staged_batches
    args = make_tree(str(tmp_path))
    img = os.path.join(args[1], args[4][0])
    data = open(img, "rb").read()
    with open(img, "wb") as f:
        f.write(data[: len(data) // 2])
    ds = STDataset(*args, raw_u8=True, decode="gpu")
    with pytest.warns(RuntimeWarning, match=os.path.basename(img)):
        for _ in staged_batches(_loader(ds, 3), torch.device(DEV)):
            pass
    cases, _ = fixture()
    with open(img, "wb") as f:
        f.write(data)
    gt = os.path.join(args[2], args[5][0])
    with open(gt, "wb") as f:                      # a baseline JPEG of 225 x 223 in a 224 x 224 batch: sniffed size differs
        f.write(next(c for c in cases if c["name"] == "gray_225x223_q75")["data"])
    with pytest.raises(RuntimeError, match=os.path.basename(gt)):
        for _ in staged_batches(_loader(ds, 3), torch.device(DEV)):
            pass


def _sp(ds, save):
    from egaze_amd.SP import SP
    os.makedirs(save, exist_ok=True)
    empty = os.path.join(save, "empty.pth.tar")
    torch.save({'state_dict': {}}, empty)              # resume=1 with nothing to load: seeded init, frozen encoders
    torch.manual_seed(0)
    return SP(lr=1e-4, save_path=save, batch_size=3, device='0', resume=1, pretrained_spatial=empty,
              pretrained_temporal=empty, traindata=ds, valdata=ds)


def test_sp_trainsp_and_extract_late_identical_on_both_paths(tmp_path):
    """SP.trainSP (its own loaders: one worker, the dataset's collate) and one AT.extract_late chunk give identical results
    with decode='gpu' and decode='host'."""
    from test_jpeg_host import make_tree
    from egaze_amd.data.STdatas import STDataset
    from egaze_amd.AT import AT
    from oracle import synth
    from torch.utils.data import DataLoader
    args = make_tree(str(tmp_path / "tree"))
    res = {}
    for mode in ("host", "gpu"):
        ds = STDataset(*args, raw_u8=True, decode=mode)
        sp = _sp(ds, str(tmp_path / mode))
        torch.manual_seed(1)
        loss = sp.trainSP()
        torch.cuda.synchronize()
        res[mode] = (loss, [p.detach().cpu() for p in sp.model.parameters()])
        ck = str(tmp_path / mode / "sp.pth.tar")
        torch.save({'state_dict': sp.model.state_dict()}, ck)
        for sub in ("train", "test"):
            d = tmp_path / mode / "512w" / sub
            d.mkdir(parents=True)
            ins, _ = synth.synth_at_batch(4, 1, seed=1)
            for i in range(4):
                torch.save(ins[i, 0].clone(), str(d / f"fix_Ahmad_Pizza1_{i:010d}.pth.tar"))
        torch.manual_seed(2)
        at = AT(pretrained_model=ck, save_path=str(tmp_path / mode), device='0', lstm_data_path=str(tmp_path / mode / "512w"))
        out = tmp_path / mode / "out"
        at.extract_late(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=ds.collate_fn), str(out / "pred") + "/",
                        str(out / "feat") + "/")
        res[mode] += ({f"{k}/{n}": open(str(out / k / n), "rb").read() for k in ("pred", "feat")
                       for n in sorted(os.listdir(str(out / k)))},)
    assert res["host"][0] == res["gpu"][0]
    assert all(torch.equal(p, q) for p, q in zip(res["host"][1], res["gpu"][1]))
    assert len(res["host"][2]) == 6 and res["host"][2] == res["gpu"][2]
