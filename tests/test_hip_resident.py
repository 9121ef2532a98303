"""The resident dataset on the GPU: egz_resident_gather against the passes it replaces (bit for bit), its bounds, the fill,
and the staging pipeline / SP / AT / stream training on a resident dataset against the host dataset."""
import os

import numpy as np
import pytest
import torch

from test_resident_host import resident_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                       # sentinel elements on each side of an output cut from an arena


def _consts():
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    mean, std = IMAGE_MEAN + FLOW_MEAN + (0.0,), IMAGE_STD + FLOW_STD + (1.0,)
    return torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)


def _case(P, N, B, H, W, seed):
    """A random pool, a table with planes repeated across samples and across the channels of one sample, the first and the
    last plane in use, and idx unsorted with repeats."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, 256, (P, H, W), dtype=torch.uint8, generator=g)
    table = torch.randint(0, P, (N, 22), dtype=torch.int64, generator=g)
    table[:, 0] = torch.randint(0, P - 2, (N,), generator=g)
    table[0, 0], table[0, 1:21], table[0, 21] = 0, 0, P - 1            # one plane in all 20 channels
    table[1, 0], table[1, 1], table[1, 2] = P - 3, P - 1, 0
    table[2] = table[1]                                                # a whole sample repeated
    table[3, 5:9] = table[3, 5]
    idx = torch.tensor([2] if B == 1 else [4, 1, 1] if B == 3 else
                       [4, 1, 1, 0, 3, 2] + torch.randint(0, N, (B - 6,), generator=g).tolist(), dtype=torch.int64)
    assert idx.numel() == B
    return pool, table, idx


def _planes(table, idx):
    t = table[idx]
    return torch.cat([t[:, :1], t[:, :1] + 1, t[:, :1] + 2, t[:, 1:]], dim=1)           # (B, 24)


class _Arena:
    """Outputs cut from one filled buffer with GUARD sentinel elements around each."""

    def __init__(self, dtype, fill, sizes):
        self.offsets, n = [], GUARD
        for s in sizes:
            self.offsets.append((n, s))
            n += s + GUARD + (-s % 4)
        self.buf = torch.empty(n, dtype=dtype, device=DEV)
        self.fill = fill
        if dtype == torch.float32:
            self.buf.fill_(float("nan"))
        else:
            self.buf.fill_(fill)

    def cut(self, i, shape):
        o, s = self.offsets[i]
        return self.buf[o:o + s].view(shape)

    def sentinels_intact(self):
        edges = [0] + [e for o, s in self.offsets for e in (o, o + s)] + [self.buf.numel()]
        for lo, hi in zip(edges[0::2], edges[1::2]):
            g = self.buf[lo:hi]
            if not bool((torch.isnan(g) if g.dtype == torch.float32 else g == self.fill).all()):
                return False
        return True


def _launch(pool, table, idx, H, W, image=None, flow=None, gt=None, nhwc=None, absmax=None, raw=None, raw_fields=7):
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    mean, std = (t.to(DEV) for t in _consts())
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    check(Hp.LIB.egz_resident_gather(pool.data_ptr(), pool.shape[0], table.data_ptr(), table.shape[0], idx.data_ptr(),
                                     idx.numel(), H, W, mean.data_ptr(), std.data_ptr(), p(image), p(flow), p(gt), p(nhwc),
                                     p(absmax), p(raw), raw_fields, status.data_ptr(), Hp._stream()), "egz_resident_gather")
    torch.cuda.synchronize()
    return int(status.item())


SHAPES = [(H, W, B) for (H, W) in ((2, 2), (6, 10), (16, 16), (33, 48), (224, 224)) for B in (1, 3)] + \
         [(16, 16, 32), (224, 224, 32)]


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_gather_bit_identical_with_the_passes_it_replaces(H, W, B):
    from egaze_amd import hipops as Hp
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    P, N, HW = 11, 5, H * W
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=H * 1000 + W * 10 + B)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
    image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
    nhwc, raw = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W))
    am = Hp._new_absmax(torch.device(DEV))
    assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw) == 0
    assert fa.sentinels_intact() and ra.sentinels_intact()

    ref_u8 = pool_h[_planes(table_h, idx_h)]                                            # (B, 24, H, W), torch gather
    assert torch.equal(raw.cpu(), ref_u8)
    mean, std = _consts()
    cpu = (ref_u8.float().div(255) - mean.view(1, 24, 1, 1)) / std.view(1, 24, 1, 1)
    dev_u8 = ref_u8.to(DEV)
    for got, sl, m, s in ((image, slice(0, 3), IMAGE_MEAN, IMAGE_STD), (flow, slice(3, 23), FLOW_MEAN, FLOW_STD),
                          (gt, slice(23, 24), (0.0,), (1.0,))):
        assert torch.equal(got, Hp.u8_normalize(dev_u8[:, sl].contiguous(), m, s))
        assert torch.equal(got.cpu(), cpu[:, sl])
    pad = Hp.nchw_to_nhwc_pad(flow.contiguous(), 32)
    assert torch.equal(nhwc, pad)
    assert bool((nhwc[..., 20:] == 0).all())                                            # zeros over the NaN fill
    assert torch.equal(Hp.absmax_value(am), Hp.absmax_value(Hp.absmax_of(pad)))
    assert float(Hp.absmax_value(am)) == float(cpu[:, 3:23].abs().max())


@pytest.mark.parametrize("fields", [("image", "gt"), ("flow", "gt")])
def test_field_subsets_write_only_their_fields(fields):
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 6, 10, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=5)
    if "image" not in fields:
        table_h[:, 0] = -1                                # what plan() leaves for a field not in use: never read
    else:
        table_h[:, 1:21] = -1
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    mask = sum({"image": 1, "flow": 2, "gt": 4}[f] for f in fields)
    ra = _Arena(torch.uint8, 0xA5, [B * 24 * H * W])
    raw = ra.cut(0, (B, 24, H, W))
    assert _launch(pool, table, idx, H, W, raw=raw, raw_fields=mask) == 0
    ref = torch.full((B, 24, H, W), 0xA5, dtype=torch.uint8)
    t = table_h[idx_h]
    if "image" in fields:
        for c in range(3):
            ref[:, c] = pool_h[t[:, 0] + c]
    else:
        ref[:, 3:23] = pool_h[t[:, 1:21]]
    ref[:, 23] = pool_h[t[:, 21]]
    assert torch.equal(raw.cpu(), ref) and ra.sentinels_intact()
    # the wrapper: fp32 outputs of the fields asked for, None for the rest, same bytes
    got = Hp.resident_gather(pool, table, idx, fields=fields)
    mean, std = _consts()
    cpu = (ref.float().div(255) - mean.view(1, 24, 1, 1)) / std.view(1, 24, 1, 1)
    for name, g, sl in (("image", got[0], slice(0, 3)), ("flow", got[1], slice(3, 23)), ("gt", got[2], slice(23, 24))):
        if name in fields:
            assert torch.equal(g.cpu(), cpu[:, sl]), name
        else:
            assert g is None
    r = Hp.resident_gather(pool, table, idx, fields=fields, raw=True)
    for name, sl in (("image", slice(0, 3)), ("flow", slice(3, 23)), ("gt", slice(23, 24))):
        if name in fields:
            assert torch.equal(r[:, sl].cpu(), ref[:, sl])


def test_wrapper_attaches_the_prepared_input_like_prepare_network_input():
    from egaze_amd import hipops as Hp
    H, W, B = 16, 16, 3
    pool_h, table_h, idx_h = _case(11, 5, B, H, W, seed=9)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    before = Hp.ABSMAX_STATS["standalone"]
    image, flow, gt = Hp.resident_gather(pool, table, idx)
    xin, version, ev = flow._egz_prepared
    assert version == flow._version and Hp.ABSMAX_STATS["standalone"] == before
    assert Hp.prepare_network_input(flow) is xin                       # early return: nothing is redone
    assert Hp.ABSMAX_STATS["standalone"] == before
    ref = flow.clone()
    want = Hp.prepare_network_input(ref)
    assert torch.equal(xin, want)
    assert torch.equal(Hp.absmax_value(xin._egz_absmax), Hp.absmax_value(want._egz_absmax))
    assert Hp.take_prepared_input(flow) is xin and not hasattr(flow, "_egz_prepared")
    _, flow2, _ = Hp.resident_gather(pool, table, idx, prepare=False)
    assert not hasattr(flow2, "_egz_prepared") and torch.equal(flow2, flow)


def test_offsets_above_4_gib():
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory for a pool above 4 GiB, {free >> 30} GiB are free")
    from egaze_amd import hipops as Hp
    H = W = 16
    P = (1 << 32) // 256 + 24
    flat = torch.empty((1 << 32) + 24 * 256, dtype=torch.uint8, device=DEV)
    pool = flat.view(P, H, W)
    last = torch.randint(0, 256, (24, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    pool[P - 24:] = last.to(DEV)
    row = [P - 24] + list(range(P - 21, P - 1)) + [P - 1]
    table = torch.tensor([row], dtype=torch.int64, device=DEV)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)
    raw = Hp.resident_gather(pool, table, idx, raw=True)
    assert torch.equal(raw.cpu()[0], last)
    image, flow, gt = Hp.resident_gather(pool, table, idx)
    mean, std = _consts()
    cpu = (last.float().div(255) - mean.view(24, 1, 1)) / std.view(24, 1, 1)
    assert torch.equal(torch.cat([image, flow, gt], dim=1).cpu()[0], cpu)
    # The same pool and table through the gathers with augmentation, whose pixel numbers are 32 bits wide but whose plane offsets
    # are not: identity rows of 5 words (egz_resident_gather_aug) and of 7 (egz_resident_gather_affine) give the same bytes and
    # values, a flipped and shifted row gives the restatement applied to the 24 planes.
    import augment_ref as A
    one, zero = np.float32(1.0), np.float32(0.0)
    five = A.rows([A.IDENTITY])
    seven = np.concatenate([five, np.array([[one, zero]], dtype=np.float32).view(np.int32)], axis=1)
    for rows in (five, seven):
        params = torch.from_numpy(rows).to(DEV)
        raw = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, raw=True, params=params)
        assert torch.equal(raw.cpu()[0], last), rows.shape
        image, flow, gt = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=params)
        got = torch.cat([image, flow, gt], dim=1).cpu()[0]
        assert torch.equal(got.view(torch.int32), cpu.view(torch.int32)), rows.shape
    moved = [(1, 1, -3, one, zero)]
    want_raw, want = A.batch(last.numpy()[None], moved, mean.numpy(), std.numpy())
    params = torch.from_numpy(A.rows(moved)).to(DEV)
    raw = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, raw=True, params=params)
    assert torch.equal(raw.cpu(), torch.from_numpy(want_raw))
    image, flow, gt = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=params)
    got = torch.cat([image, flow, gt], dim=1).cpu()
    assert torch.equal(got.view(torch.int32), torch.from_numpy(want).view(torch.int32))
    del flat, pool


@pytest.mark.parametrize("what", ["idx_high", "idx_negative", "table_high", "table_negative", "image_last_planes"])
def test_bad_indices_are_refused_not_dereferenced(what):
    """A bounds check that refuses: the bad sample is skipped (its outputs keep the arena's fill), the status word says why,
    the wrapper raises, the other samples of the batch are right."""
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 6, 10, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=11)
    bad, want = 1, 2
    if what == "idx_high":
        idx_h[bad], want = N, 1
    elif what == "idx_negative":
        idx_h[bad], want = -1, 1
    elif what == "table_high":
        idx_h[bad] = 3
        table_h[3, 7] = P
    elif what == "table_negative":
        idx_h[bad] = 3
        table_h[3, 21] = -(1 << 40)
    else:
        idx_h[bad] = 3
        table_h[3, 0] = P - 2                             # the image's third plane would be plane P
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    HW = H * W
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    image, flow, gt, nhwc = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W)), fa.cut(3, (B, H, W, 32))
    am = Hp._new_absmax(torch.device(DEV))
    assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am) == want
    assert fa.sentinels_intact()
    good = [b for b in range(B) if b != bad]
    ok_idx = idx_h[good]
    ref_u8 = pool_h[_planes(table_h, ok_idx)]
    mean, std = _consts()
    cpu = (ref_u8.float().div(255) - mean.view(1, 24, 1, 1)) / std.view(1, 24, 1, 1)
    got = torch.cat([image, flow, gt], dim=1).cpu()
    assert torch.equal(got[good], cpu)
    assert bool(torch.isnan(got[bad]).all()) and bool(torch.isnan(nhwc[bad]).all())
    assert torch.equal(nhwc.cpu()[good][..., :20], cpu[:, 3:23].permute(0, 2, 3, 1))
    with pytest.raises(RuntimeError, match="resident_gather"):
        Hp.resident_gather(pool, table, idx)
    sample = {}
    Hp.resident_gather(pool, table, idx, status_to=sample)             # deferred: raised at hand-over
    from egaze_amd.data.STdatas import check_decode_status
    with pytest.raises(RuntimeError, match="resident_gather"):
        check_decode_status(sample)


# ----------------------------------------------------------------------------- fill
@pytest.mark.parametrize("decode", ["host", "gpu"])
def test_fill_every_plane_equals_imread(tmp_path, decode, capsys):
    from egaze_amd.data._io import imread
    from egaze_amd.data.resident import ResidentSTDataset
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True, decode=decode)
    ds.fill(DEV, chunk=17)                                # several chunks, the staging buffer reused
    out = capsys.readouterr().out
    assert "46 files" in out and str(ds.needed_bytes) in out
    pool = ds.pool.cpu().numpy()
    assert pool.shape == (60, 224, 224) and torch.equal(ds.table.cpu(), ds.plane_table)
    for path, plane, channels in ds.files:
        a = imread(path, gray=channels == 1)
        a = a[None] if a.ndim == 2 else a.transpose((2, 0, 1))
        assert np.array_equal(pool[plane:plane + channels], a), path


def test_fill_reports_bad_files(tmp_path):
    from test_jpeg_host import fixture
    from egaze_amd.data.resident import ResidentSTDataset
    args = resident_tree(tmp_path)
    img = os.path.join(args[1], args[4][0])
    data = open(img, "rb").read()
    with open(img, "wb") as f:
        f.write(data[: len(data) // 2])
    with pytest.warns(RuntimeWarning, match=os.path.basename(img)):
        ResidentSTDataset(*args, raw_u8=True, decode="gpu").fill(DEV)
    with open(img, "wb") as f:
        f.write(data)
    cases, _ = fixture()
    gt = os.path.join(args[2], args[5][0])
    keep = open(gt, "rb").read()
    with open(gt, "wb") as f:
        f.write(next(c for c in cases if c["name"] == "gray_225x223_q75")["data"])
    for decode in ("host", "gpu"):
        with pytest.raises(RuntimeError, match=os.path.basename(gt)):
            ResidentSTDataset(*args, raw_u8=True, decode=decode).fill(DEV)
    with open(gt, "wb") as f:
        f.write(keep)
    flow = os.path.join(args[0], args[3][0], "flow_y_00005.jpg")
    os.remove(flow)
    for decode in ("host", "gpu"):
        with pytest.raises(RuntimeError, match=os.path.basename(flow)):
            ResidentSTDataset(*args, raw_u8=True, decode=decode).fill(DEV)


# ----------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return resident_tree(tmp_path_factory.mktemp("resident"))


@pytest.fixture(scope="module")
def datasets(tree):
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    return STDataset(*tree, raw_u8=True), ResidentSTDataset(*tree, raw_u8=True, decode="gpu").fill(DEV)


def test_staged_batches_identical_to_the_host_loader(datasets):
    from torch.utils.data import DataLoader
    from egaze_amd import hipops as Hp
    from egaze_amd.data.STdatas import staged_batches
    got, grown = {}, {}
    for name, ds in zip(("host", "resident"), datasets):
        torch.manual_seed(4)
        loader = DataLoader(ds, batch_size=3, shuffle=True, num_workers=0, pin_memory=True, collate_fn=ds.collate_fn)
        before = Hp.ABSMAX_STATS["standalone"]
        res = []
        for _ in range(2):
            for sample, staged in staged_batches(loader, torch.device(DEV)):
                xin = staged[1]._egz_prepared[0]
                res.append((list(sample["imname"]), [t.clone() for t in staged], xin.clone(),
                            Hp.absmax_value(xin._egz_absmax).clone()))
        torch.cuda.synchronize()
        got[name], grown[name] = res, Hp.ABSMAX_STATS["standalone"] - before
    assert len(got["host"]) == len(got["resident"]) == 6
    for (n_h, st_h, x_h, am_h), (n_r, st_r, x_r, am_r) in zip(got["host"], got["resident"]):
        assert n_h == n_r
        for a, b in zip(st_h, st_r):
            assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b)
        assert torch.equal(x_h, x_r) and torch.equal(am_h, am_r)
    assert grown["resident"] <= grown["host"]


def test_to_raw_u8_matches_the_host_bytes(datasets):
    from torch.utils.data import DataLoader
    from egaze_amd.data.STdatas import to_raw_u8
    host, res = datasets
    for B in (1, 3):
        lh = DataLoader(host, batch_size=B, shuffle=False, num_workers=0)
        lr = DataLoader(res, batch_size=B, shuffle=False, num_workers=0, collate_fn=res.collate_fn)
        for s_h, s_r in zip(lh, lr):
            r = to_raw_u8(s_r, torch.device(DEV))
            for k in ("image", "flow", "gt"):
                assert r[k].is_contiguous() and torch.equal(r[k].cpu(), s_h[k]), k
            assert r["imname"] == s_h["imname"] and torch.equal(r["fixsac"], s_h["fixsac"])


def test_sp_and_extract_late_identical_on_host_and_resident(tree, datasets, tmp_path):
    """SP.trainSP / testSP through SP's own loaders and one AT.extract_late: the resident dataset gives the host dataset's
    loss, parameters, metrics and output files under the same seeds."""
    from test_hip_jpeg import _sp
    from egaze_amd.AT import AT
    from oracle import synth
    from torch.utils.data import DataLoader
    res = {}
    for mode, ds in zip(("host", "resident"), datasets):
        sp = _sp(ds, str(tmp_path / mode))
        assert sp.STTrainLoader.num_workers == (0 if mode == "resident" else 1)
        torch.manual_seed(1)
        loss = sp.trainSP()
        torch.cuda.synchronize()
        res[mode] = (loss, [p.detach().cpu() for p in sp.model.parameters()], sp.testSP())
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
    assert res["host"][0] == res["resident"][0]
    assert all(torch.equal(p, q) for p, q in zip(res["host"][1], res["resident"][1]))
    assert np.array_equal(np.array([float(v) for v in res["host"][2]]), np.array([float(v) for v in res["resident"][2]]),
                          equal_nan=True)
    assert len(res["host"][3]) == 14 and res["host"][3] == res["resident"][3]


def test_temporal_stream_epoch_identical_on_host_and_resident(tree):
    from torch.utils.data import DataLoader
    from egaze_amd import streamtrain
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import cfg, make_layers
    res = {}
    for mode in ("host", "resident"):
        if mode == "host":
            ds = STDataset(*tree, raw_u8=True)
        else:
            ds = ResidentSTDataset(*tree, raw_u8=True)
            ds.gpu_fields = ("flow", "gt")
            ds.fill(DEV)
            assert ds.planes == 32 + 7
        torch.manual_seed(0)
        model = streamtrain.StreamVGG(make_layers(cfg['D'], 20), freeze_features=False).to(DEV)
        opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
        torch.manual_seed(1)
        loader = DataLoader(ds, batch_size=3, shuffle=True, num_workers=getattr(ds, 'loader_workers', 0), pin_memory=True,
                            collate_fn=ds.collate_fn)
        loss = streamtrain.train_epoch(loader, model, floss().to(DEV), opt, 0, DEV, stream='temporal')
        torch.cuda.synchronize()
        res[mode] = (loss, [p.detach().cpu() for p in model.parameters()], [b.detach().cpu() for b in model.buffers()])
    assert res["host"][0] == res["resident"][0]
    assert all(torch.equal(p, q) for p, q in zip(res["host"][1], res["resident"][1]))
    assert all(torch.equal(p, q) for p, q in zip(res["host"][2], res["resident"][2]))


def test_extractw_identical_on_host_and_resident(tree, datasets, tmp_path):
    """extractLSTMw.extractw stages a resident batch as it stages a decode='gpu' one: the host dataset's files."""
    from torch.utils.data import DataLoader
    from egaze_amd.data.STdatas import STDataset
    from egaze_amd.extractLSTMw import extractw
    from egaze_amd.utils import cfg, make_layers
    torch.manual_seed(5)
    model = make_layers(cfg['D'], 3).to(DEV).eval()
    out = {}
    for mode, ds in (("host", STDataset(*tree)), ("resident", datasets[1])):       # host: normalised in __getitem__
        loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=ds.collate_fn)
        extractw(loader, model, str(tmp_path / mode), device='0')
        out[mode] = {n: torch.load(str(tmp_path / mode / n)) for n in sorted(os.listdir(str(tmp_path / mode)))}
    assert len(out["host"]) >= 1 and list(out["host"]) == list(out["resident"])
    assert all(torch.equal(out["host"][n], out["resident"][n]) for n in out["host"])


def test_make_loaders_with_gpu_resident(tree):
    """The CLI path of the stream scripts: --gpu_resident builds filled resident datasets (the stream's fields only), loaders
    without workers, and stage_stream hands over what the host loaders' batches give."""
    import argparse
    from egaze_amd import streamtrain
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import check_decode_status
    base = dict(flowPath=tree[0], imagePath=tree[1], gtPath=tree[2], fixsacPath=tree[7], val_name="Alireza", batch_size=3,
                device="0")
    got = {}
    for mode, extra in (("host", {}), ("resident", dict(gpu_resident=True, gpu_decode=True, gpu_resident_gb=0.5))):
        torch.manual_seed(3)
        train, val, _ = streamtrain.make_loaders(argparse.Namespace(**base, **extra), key="flow")
        if mode == "resident":
            ds = train.dataset
            assert isinstance(ds, ResidentSTDataset) and ds.decode == "gpu" and train.num_workers == 0
            assert ds.pool.shape == (32 + 7, 224, 224) and val.dataset.pool is None and len(val.dataset) == 0
        res = []
        for sample in train:
            x, gt = streamtrain.stage_stream(sample, torch.device(DEV), key="flow")
            check_decode_status(sample)
            res.append((list(sample["imname"]), x.clone(), gt.clone(), x._egz_prepared[0].clone()))
        got[mode] = res
    assert len(got["host"]) == 3
    for (n_h, x_h, g_h, p_h), (n_r, x_r, g_r, p_r) in zip(got["host"], got["resident"]):
        assert n_h == n_r and torch.equal(x_h, x_r) and torch.equal(g_h, g_r) and torch.equal(p_h, p_r)
