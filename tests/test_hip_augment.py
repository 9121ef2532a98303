"""The augmented resident gather on the GPU (egz_resident_gather_aug, hipops.resident_gather_aug) against
the numpy restatement tests/augment_ref.py, bit for bit: geometry with explicit parameters, the identity against
egz_resident_gather, the photometric step at every byte value, the device-side draw, the status word, and the two training
loops that use it (SP.trainSP, streamtrain.train_epoch) on a resident dataset."""
import os

import numpy as np
import pytest
import torch

import augment_ref as A
from test_hip_resident import DEV, _Arena, _case, _consts, _launch as _launch_plain, _planes
from test_resident_host import resident_tree

pytestmark = pytest.mark.gpu
ONE, ZERO = np.float32(1.0), np.float32(0.0)
TABLE = dict(seed=1, flip_thr=1 << 31, shift=16, contrast=0.2, brightness=0.1)       # the setting of the known answers


def _launch(pool, table, idx, H, W, image=None, flow=None, gt=None, nhwc=None, absmax=None, raw=None, raw_fields=7,
            params=None, params_out=None, epoch=0, seed=0, flip_thr=0, shift=0, contrast=0.0, brightness=0.0):
    """egz_resident_gather_aug through the C ABI -> the status word."""
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    mean, std = (t.to(DEV) for t in _consts())
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    check(Hp.LIB.egz_resident_gather_aug(pool.data_ptr(), pool.shape[0], table.data_ptr(), table.shape[0], idx.data_ptr(),
                                         idx.numel(), H, W, mean.data_ptr(), std.data_ptr(), p(image), p(flow), p(gt), p(nhwc),
                                         p(absmax), p(raw), raw_fields, status.data_ptr(), seed, epoch, flip_thr, shift,
                                         contrast, brightness, p(params), p(params_out), Hp._stream()),
          "egz_resident_gather_aug")
    torch.cuda.synchronize()
    return int(status.item())


def _refill(arena):
    arena.buf.fill_(float("nan") if arena.buf.dtype == torch.float32 else arena.fill)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dev_same(a, b):
    """Two device tensors of one dtype and shape: equal bit patterns, compared where they are."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _same_bits(got, want):
    """A device fp32 tensor against a numpy fp32 array: equal bit patterns (so -0 and NaN count too)."""
    return torch.equal(_bits(got), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


def _expected(pool_h, table_h, idx_h, params):
    """The restatement on the torch-gathered bytes -> (raw u8 (B,24,H,W), fp32 (B,24,H,W), nhwc (B,H,W,32), max |flow|)."""
    mean, std = _consts()
    u8 = pool_h[_planes(table_h, idx_h)].numpy()
    raw, f32 = A.batch(u8, params, mean.numpy(), std.numpy())
    B, _, H, W = f32.shape
    nhwc = np.zeros((B, H, W, 32), dtype=np.float32)
    nhwc[..., :20] = f32[:, 3:23].transpose(0, 2, 3, 1)
    return raw, f32, nhwc, np.abs(f32[:, 3:23]).max()


def _geometry_rows(H, W):
    rows = [A.IDENTITY, (1, 0, 0, ONE, ZERO)]
    for flip in (0, 1):
        for d in (1, 2, 3, 4, 5, W - 1, W, W + 3):
            rows += [(flip, 0, d, ONE, ZERO), (flip, 0, -d, ONE, ZERO)]
        for d in (1, 2, 3, 4, 5, H - 1, H, H + 3):
            rows += [(flip, d, 0, ONE, ZERO), (flip, -d, 0, ONE, ZERO)]
    g, b = np.float32(1.25), np.float32(-0.1)
    rows += [(1, 2, -3, g, b), (0, -H, 5, ONE, ZERO), (1, H + 3, -(W + 3), g, ZERO), (1, -1, W - 1, ONE, b), (0, 1, 1, g, b),
             (1, -(H - 1), 2, ONE, ZERO), (0, 3, -(W - 1), g, b), (1, 32767, -32767, ONE, ZERO), (0, -32767, 32767, ONE, ZERO)]
    return rows


SHAPES = [(H, W, B) for (H, W) in ((2, 4), (6, 12), (16, 16), (33, 48), (224, 224)) for B in (1, 3)] + [(16, 16, 32)]


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_geometry_bit_identical_with_the_restatement(H, W, B):
    """Explicit parameter rows -- identity, flip, every shift that moves the interior / border split, rows and columns that
    leave the frame, mixed rows in one batch -- in chunks of B; every output form, cut from sentinel-filled arenas."""
    from egaze_amd import hipops as Hp
    P, N, HW = 11, 5, H * W
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=H * 1000 + W * 10 + B)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
    pa = _Arena(torch.int32, -77, [B * 5])
    image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
    nhwc, raw, used = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W)), pa.cut(0, (B, 5))
    rows = _geometry_rows(H, W)
    rows += [A.IDENTITY] * (-len(rows) % B)
    for k in range(0, len(rows), B):
        chunk = rows[k:k + B]
        for a in (fa, ra, pa):
            _refill(a)
        am = Hp._new_absmax(torch.device(DEV))
        params = torch.from_numpy(A.rows(chunk)).to(DEV)
        assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params=params, params_out=used) == 0, chunk
        assert fa.sentinels_intact() and ra.sentinels_intact() and pa.sentinels_intact(), chunk
        want_raw, want, want_nhwc, want_am = _expected(pool_h, table_h, idx_h, chunk)
        assert torch.equal(raw.cpu(), torch.from_numpy(want_raw)), chunk
        assert _same_bits(image, want[:, :3]) and _same_bits(flow, want[:, 3:23]) and _same_bits(gt, want[:, 23:]), chunk
        assert _same_bits(nhwc, want_nhwc), chunk
        assert float(Hp.absmax_value(am)) == float(want_am), chunk
        assert torch.equal(used.cpu(), params.cpu()), chunk


@pytest.mark.parametrize("fields", [("image", "gt"), ("flow", "gt"), ("flow",)])
def test_field_subsets_write_only_their_fields(fields):
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 6, 12, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=5)
    if "image" not in fields:
        table_h[:, 0] = -1                                # what plan() leaves for a field not in use: never read
    else:
        table_h[:, 1:21] = -1
    if "gt" not in fields:
        table_h[:, 21] = -1
    chunk = [(1, 1, -2, np.float32(0.75), np.float32(0.125)), (0, -2, 5, ONE, ZERO), (1, 0, 13, np.float32(1.5), ZERO)]
    params = torch.from_numpy(A.rows(chunk)).to(DEV)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    mask = sum({"image": 1, "flow": 2, "gt": 4}[f] for f in fields)
    ra = _Arena(torch.uint8, 0xA5, [B * 24 * H * W])
    raw = ra.cut(0, (B, 24, H, W))
    assert _launch(pool, table, idx, H, W, raw=raw, raw_fields=mask, params=params) == 0
    safe = table_h.clamp(min=0)                           # the planes of the unused fields: anything, they are masked below
    want_raw, want, want_nhwc, _ = _expected(pool_h, safe, idx_h, chunk)
    sl = {"image": slice(0, 3), "flow": slice(3, 23), "gt": slice(23, 24)}
    ref = np.full((B, 24, H, W), 0xA5, dtype=np.uint8)
    for f in fields:
        ref[:, sl[f]] = want_raw[:, sl[f]]
    assert torch.equal(raw.cpu(), torch.from_numpy(ref)) and ra.sentinels_intact()
    # the wrapper: fp32 outputs of the fields asked for, None for the rest; the NHWC-32 form rides on flow
    got, used = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, fields=fields, params=params, want_params=True)
    assert torch.equal(used, params)
    for name, g in zip(("image", "flow", "gt"), got):
        if name in fields:
            assert _same_bits(g, want[:, sl[name]]), name
        else:
            assert g is None
    if "flow" in fields:
        assert _same_bits(got[1]._egz_prepared[0], want_nhwc)
    r = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, fields=fields, raw=True, params=params)
    for f in fields:
        assert torch.equal(r[:, sl[f]].cpu(), torch.from_numpy(want_raw[:, sl[f]]))


@pytest.mark.parametrize("H,W,B", [(2, 4, 1), (6, 12, 3), (33, 48, 3), (224, 224, 3), (16, 16, 32)])
def test_identity_parameters_reproduce_the_plain_gather(H, W, B):
    """flip 0, dy = dx = 0, gain 1, bias 0 -- as an explicit row and as the draw of an all-zero spec -- against
    egz_resident_gather on the same inputs: every output bit-identical, the abs-max included."""
    from egaze_amd import hipops as Hp
    HW = H * W
    pool_h, table_h, idx_h = _case(11, 5, B, H, W, seed=H + W + B)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    outs = []
    for mode in ("plain", "explicit", "drawn"):
        fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
        ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
        image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
        nhwc, raw = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W))
        am = Hp._new_absmax(torch.device(DEV))
        if mode == "plain":
            assert _launch_plain(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw) == 0
        else:
            params = torch.from_numpy(A.rows([A.IDENTITY] * B)).to(DEV) if mode == "explicit" else None
            used = torch.full((B, 5), -1, dtype=torch.int32, device=DEV)
            assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params=params, params_out=used, seed=3,
                           epoch=4) == 0
            # the draw of an all-zero spec: gain 1 and bias 0 * t = +-0, which adds nothing to a byte's value either way
            want = A.rows([A.IDENTITY] * B) if mode == "explicit" else A.draw_rows(3, 4, idx_h.tolist(), 0, 0, 0.0, 0.0)
            assert torch.equal(used.cpu(), torch.from_numpy(want)) and (want[:, :4] == [0, 0, 0, 0x3f800000]).all()
            assert ((want[:, 4] & 0x7fffffff) == 0).all()
        assert fa.sentinels_intact() and ra.sentinels_intact()
        outs.append((fa.buf, ra.buf, Hp.absmax_value(am).clone()))
    for other in outs[1:]:
        assert all(_dev_same(a, b) for a, b in zip(outs[0], other))


def test_photometric_step_at_every_byte_value():
    """All 256 byte values in every plane, the three colour channels (three mean / std pairs), at gains and biases that clamp at
    0, at 1 and at both ends, at a negative gain, and at the known answers' values: the colour frame equals the fp32
    restatement bit for bit, flow and ground truth are those of gain 1, bias 0."""
    H = W = 16
    g = torch.Generator().manual_seed(2)
    pool_h = torch.stack([torch.randperm(256, generator=g).to(torch.uint8).view(H, W) for _ in range(6)])
    table_h = torch.tensor([[0] + [3, 4] * 10 + [5], [3] + [4, 5] * 10 + [0]], dtype=torch.int64)
    known = [A.draw(1, e, s, 1 << 31, 16, 0.2, 0.1)[3:] for e, s in ((0, 0), (0, 1), (0, 6), (0, (1 << 33) + 5), (3, 1))]
    pairs = [(3.0, -1.0), (0.5, 0.75), (2.0, -1.5), (-2.0, 1.5), (1e-30, 0.0), (1.0, 1e-8), (4.0, 0.0), (0.0, 0.5)] + known
    idx_h = torch.tensor([0, 1] * len(pairs), dtype=torch.int64)
    chunk = [(0, 0, 0, np.float32(a), np.float32(b)) for a, b in pairs for _ in range(2)]
    B = len(chunk)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa = _Arena(torch.float32, None, [B * 3 * H * W, B * 20 * H * W, B * H * W])
    image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
    params = torch.from_numpy(A.rows(chunk)).to(DEV)
    assert _launch(pool, table, idx, H, W, image, flow, gt, params=params) == 0 and fa.sentinels_intact()
    _, want, _, _ = _expected(pool_h, table_h, idx_h, chunk)
    assert _same_bits(image, want[:, :3])
    _, neutral, _, _ = _expected(pool_h, table_h, idx_h, [A.IDENTITY] * B)
    assert _same_bits(flow, neutral[:, 3:23]) and _same_bits(gt, neutral[:, 23:])
    lo, hi = want[0:2, :3].min(axis=(0, 2, 3)), want[0:2, :3].max(axis=(0, 2, 3))       # (3.0, -1.0) clamps at both ends
    mean, std = (t.numpy() for t in _consts())
    assert np.array_equal(lo, (ZERO - mean[:3]) / std[:3]) and np.array_equal(hi, (ONE - mean[:3]) / std[:3])


@pytest.mark.parametrize("H,W", [(16, 16), (224, 224)])
def test_device_draw_equals_the_restatement_and_the_explicit_mode(H, W):
    """params_out for sample numbers that include 0 and a repeat, under the known answers' setting and two epochs; the outputs of
    the drawn mode equal the explicit mode fed with params_out; a second launch gives the same bits.  (A sample number above
    2^32 needs a table of that many rows: that case is pinned on the host only, tests/test_augment_host.py.)"""
    from egaze_amd import hipops as Hp
    P, N, HW = 11, 8, H * W
    pool_h, table_h, _ = _case(P, N, 6, H, W, seed=H)
    idx_h = torch.tensor([6, 0, 1, 6, 7, 3, 0], dtype=torch.int64)
    B = idx_h.numel()
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    spec = Hp.AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=1)
    assert spec.flip_thr == TABLE["flip_thr"]
    for epoch in (0, 3):
        want_rows = A.draw_rows(1, epoch, idx_h.tolist(), 1 << 31, 16, 0.2, 0.1)
        if epoch == 0:                                    # the known answers of samples 6, 0, 1
            assert want_rows[:3, :3].tolist() == [[1, -11, 1], [1, -12, -11], [0, -1, 11]]
        runs = []
        for mode in ("drawn", "drawn", "explicit"):
            fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
            ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
            pa = _Arena(torch.int32, -77, [B * 5])
            image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
            nhwc, raw, used = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W)), pa.cut(0, (B, 5))
            am = Hp._new_absmax(torch.device(DEV))
            kw = dict(params=runs[0][2].clone()) if mode == "explicit" else \
                dict(seed=1, flip_thr=1 << 31, shift=16, contrast=0.2, brightness=0.1)
            assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params_out=used, epoch=epoch, **kw) == 0
            assert fa.sentinels_intact() and ra.sentinels_intact() and pa.sentinels_intact()
            assert torch.equal(used.cpu(), torch.from_numpy(want_rows)), (epoch, mode)
            assert torch.equal(used[0], used[3]) and torch.equal(used[1], used[6])       # the same sample, the same row
            runs.append((fa.buf, ra.buf, used, Hp.absmax_value(am).clone()))
        for other in runs[1:]:
            assert all(_dev_same(a, b) for a, b in zip(runs[0], other))
        want_raw, want, want_nhwc, _ = _expected(pool_h, table_h, idx_h, A.unrows(want_rows))
        assert torch.equal(raw.cpu(), torch.from_numpy(want_raw)) and _same_bits(nhwc, want_nhwc)
        assert _same_bits(torch.cat([image, flow, gt], dim=1), want)
    # the wrapper draws the same rows, whatever the batch around a sample
    (_, _, _), rows_a = Hp.resident_gather_aug(pool, table, idx, spec, 3, want_params=True)
    (_, _, _), rows_b = Hp.resident_gather_aug(pool, table, idx[2:5].contiguous(), spec, 3, want_params=True)
    assert torch.equal(rows_a.cpu(), torch.from_numpy(want_rows)) and torch.equal(rows_b, rows_a[2:5])


# ----------------------------------------------------------------------------- status
BAD_ROWS = {"flip_2": (0, 2), "flip_negative": (0, -1), "dy_high": (1, 32768), "dy_low": (1, -32768), "dx_high": (2, 32768),
            "dx_low": (2, -(1 << 31)), "gain_inf": (3, 0x7f800000), "gain_nan": (3, 0x7fc00000),
            "bias_minus_inf": (4, -8388608), "bias_nan": (4, 0x7f800001)}


@pytest.mark.parametrize("what", ["idx_high", "idx_negative", "table_high", "image_last_planes", "idx_and_row"] + list(BAD_ROWS))
def test_bad_samples_are_refused_by_value(what):
    """Bits 0 and 1 as in the plain gather, bit 2 for each kind of bad explicit row: the sample is skipped (its outputs keep the
    arena's fill), the others are right, the wrapper raises.  Nothing here dereferences a bad index."""
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 6, 12, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=11)
    chunk = [(1, 1, -2, np.float32(1.1), np.float32(0.05)), (0, 2, 1, ONE, ZERO), (1, 0, 3, np.float32(0.9), ZERO)]
    rows = A.rows(chunk)
    bad, want = [1], 4
    if what == "idx_high":
        idx_h[1], want = N, 1
    elif what == "idx_negative":
        idx_h[1], want = -1, 1
    elif what == "table_high":
        idx_h[1], want = 3, 2
        table_h[3, 7] = P
    elif what == "image_last_planes":
        idx_h[1], want = 3, 2
        table_h[3, 0] = P - 2
    elif what == "idx_and_row":
        idx_h[0], want, bad = N + 5, 5, [0, 1]
        rows[1, 0] = 7
    else:
        col, val = BAD_ROWS[what]
        rows[1, col] = val
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    params = torch.from_numpy(rows).to(DEV)
    HW = H * W
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    pa = _Arena(torch.int32, -77, [B * 5])
    image, flow, gt, nhwc = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W)), fa.cut(3, (B, H, W, 32))
    used = pa.cut(0, (B, 5))
    am = Hp._new_absmax(torch.device(DEV))
    assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, params=params, params_out=used) == want
    assert fa.sentinels_intact() and pa.sentinels_intact()
    good = [b for b in range(B) if b not in bad]
    _, ref, ref_nhwc, _ = _expected(pool_h, table_h, idx_h[good], [chunk[b] for b in good])
    got = torch.cat([image, flow, gt], dim=1)
    assert _same_bits(got[good], ref) and _same_bits(nhwc[good], ref_nhwc)
    assert bool(torch.isnan(got[bad]).all()) and bool(torch.isnan(nhwc[bad]).all())
    assert torch.equal(used[good].cpu(), torch.from_numpy(rows[good])) and bool((used[bad] == -77).all())
    with pytest.raises(RuntimeError, match="resident_gather: .*skipped") as e:
        Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=params)
    assert Hp.RESIDENT_STATUS[want] in str(e.value)
    sample = {}
    Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=params, status_to=sample)   # deferred to the hand-over
    from egaze_amd.data.STdatas import check_decode_status
    with pytest.raises(RuntimeError, match="resident_gather"):
        check_decode_status(sample)


def test_a_width_that_is_no_multiple_of_4_is_refused_by_message():
    from egaze_amd import hipops as Hp
    pool_h, table_h, idx_h = _case(11, 5, 3, 6, 10, seed=1)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    Hp.resident_gather(pool, table, idx)                  # the plain gather takes it: H * W % 4 == 0
    with pytest.raises(RuntimeError, match="W = 10 must be a multiple of 4"):
        Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(flip=0.5), 0)
    with pytest.raises(ValueError, match="AugSpec"):
        Hp.resident_gather_aug(pool, table, idx, "flip", 0)
    with pytest.raises(ValueError, match="params"):
        Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=torch.zeros((3, 5), dtype=torch.int64, device=DEV))


# ----------------------------------------------------------------------------- drivers
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return resident_tree(tmp_path_factory.mktemp("augment"))


@pytest.fixture(scope="module")
def host_bytes(tree):
    """(7, 24, H, W) uint8: the host dataset's planes of every sample."""
    from egaze_amd.data.STdatas import STDataset
    host = STDataset(*tree, raw_u8=True)
    return np.stack([np.concatenate([host[i][k].numpy() for k in ("image", "flow", "gt")]) for i in range(len(host))])


def _spy(ds, monkeypatch):
    """Records, per gather of ``ds``, the sample numbers, whether the batch was stamped, and which binding ran."""
    from egaze_amd import hipops as Hp
    log = {"index": [], "stamped": [], "calls": []}
    inner = ds.gather

    def gather(sample, *a, **k):
        log["index"].append(sample["index"].tolist())
        log["stamped"].append("augment" in sample)
        return inner(sample, *a, **k)
    ds.gather = gather
    for name in ("resident_gather", "resident_gather_aug"):
        def wrapped(*a, _f=getattr(Hp, name), _n=name, **k):
            log["calls"].append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(Hp, name, wrapped)
    return log


def _capture(module, seen, pick):
    return module.register_forward_pre_hook(lambda m, inp: seen.append(pick(inp)))


def _new_sp(ds, save, augment):
    from egaze_amd.SP import SP
    os.makedirs(save, exist_ok=True)
    empty = os.path.join(save, "empty.pth.tar")
    torch.save({'state_dict': {}}, empty)                 # resume=1 with nothing to load: seeded init, frozen encoders
    torch.manual_seed(0)
    return SP(lr=1e-4, save_path=save, batch_size=3, device='0', resume=1, pretrained_spatial=empty,
              pretrained_temporal=empty, traindata=ds, valdata=ds, augment=augment)


def test_sp_trainsp_augments_its_batches_and_nothing_else(tree, host_bytes, tmp_path, monkeypatch):
    """One epoch of SP.trainSP with a spec: the batches the loop saw equal the restatement applied to the host dataset's
    bytes; the same seed gives the same loss twice; testSP, to_raw_u8 and the batch-1 extraction batch afterwards are those of
    the unaugmented run; augment=None goes through the plain gather and gives the loss of an SP built the way it was before the
    argument existed (test_hip_jpeg._sp), bit for bit."""
    from torch.utils.data import DataLoader
    from egaze_amd import hipops as Hp
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import to_raw_u8
    from test_hip_jpeg import _sp
    mean, std = (t.numpy() for t in _consts())
    ds = ResidentSTDataset(*tree, raw_u8=True, decode="gpu").fill(DEV)
    log = _spy(ds, monkeypatch)
    spec = Hp.AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=1)
    losses, state = {}, {}
    for mode in ("plain", "none", "aug", "aug_again"):
        sp = _sp(ds, str(tmp_path / mode)) if mode == "plain" else \
            _new_sp(ds, str(tmp_path / mode), spec if mode.startswith("aug") else None)
        sp.epochnow = 3
        seen_in, seen_gt = [], []
        hooks = [_capture(sp.model, seen_in, lambda inp: (inp[0].clone(), inp[1].clone())),
                 _capture(sp.criterion, seen_gt, lambda inp: inp[1].clone())]
        first = len(log["index"])
        torch.manual_seed(1)
        losses[mode] = sp.trainSP()
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        order, stamped, calls = log["index"][first:], log["stamped"][first:], log["calls"][first:]
        assert sorted(i for b in order for i in b) == list(range(7)) and len(order) == len(seen_in) == 3
        if mode in ("plain", "none"):
            assert not any(stamped) and calls == ["resident_gather"] * 3
        if mode == "plain":
            continue
        if mode == "none":
            state["none"] = {k: v.clone() for k, v in sp.model.state_dict().items()}
            state["val"] = sp.testSP()
            continue
        assert all(stamped) and calls == ["resident_gather_aug"] * 3 and ds._augment is None
        for idxs, (im, fl), gt in zip(order, seen_in, seen_gt):
            params = [A.draw(1, 3, i, 1 << 31, 16, 0.2, 0.1) for i in idxs]
            _, want = A.batch(host_bytes[idxs], params, mean, std)
            assert _same_bits(im, want[:, :3]) and _same_bits(fl, want[:, 3:23])
            assert _same_bits(gt.reshape(len(idxs), 1, 224, 224), want[:, 23:])
        if mode == "aug":
            # after the augmented epoch: validation, raw bytes and the extraction's batch-1 loader are the unaugmented run's
            sp.model.load_state_dict(state["none"])
            first = len(log["index"])
            val = sp.testSP()
            assert np.array_equal(np.array([float(v) for v in val]), np.array([float(v) for v in state["val"]]),
                                  equal_nan=True)
            assert not any(log["stamped"][first:]) and set(log["calls"][first:]) == {"resident_gather"}
            for B in (1, 3):
                for k, s in enumerate(DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, collate_fn=ds.collate_fn)):
                    r = to_raw_u8(s, torch.device(DEV))
                    got = torch.cat([r["image"], r["flow"], r["gt"]], dim=1).cpu().numpy()
                    assert np.array_equal(got, host_bytes[k * B:k * B + B])
    assert losses["none"] == losses["plain"]
    assert losses["aug"] == losses["aug_again"] and losses["aug"] != losses["none"]


def test_temporal_stream_epoch_augments_its_batches(tree, host_bytes, monkeypatch):
    """streamtrain.train_epoch on the temporal stream: the same checks -- the batches seen, the same loss twice under one seed,
    another epoch number another draw, augment=None through the plain gather with the host dataset's loss -- and evaluate()
    afterwards unaugmented."""
    from torch.utils.data import DataLoader
    from egaze_amd import hipops as Hp
    from egaze_amd import streamtrain
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import cfg, make_layers
    mean, std = (t.numpy() for t in _consts())
    ds = ResidentSTDataset(*tree, raw_u8=True)
    ds.gpu_fields = ("flow", "gt")
    ds.fill(DEV)
    log = _spy(ds, monkeypatch)
    spec = Hp.AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=1)
    losses = {}
    for mode, epoch in (("host", 0), ("none", 0), ("aug", 2), ("aug_again", 2), ("aug_epoch5", 5)):
        data = STDataset(*tree, raw_u8=True) if mode == "host" else ds
        torch.manual_seed(0)
        model = streamtrain.StreamVGG(make_layers(cfg['D'], 20), freeze_features=False).to(DEV)
        opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
        crit = floss().to(DEV)
        seen_in, seen_gt = [], []
        hooks = [_capture(model.features, seen_in, lambda inp: inp[0].clone()),
                 _capture(crit, seen_gt, lambda inp: inp[1].clone())]
        torch.manual_seed(1)
        loader = DataLoader(data, batch_size=3, shuffle=True, num_workers=getattr(data, 'loader_workers', 0), pin_memory=True,
                            collate_fn=data.collate_fn)
        first = len(log["index"])
        losses[mode] = streamtrain.train_epoch(loader, model, crit, opt, epoch, DEV, stream='temporal',
                                               augment=spec if mode.startswith("aug") else None)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        if mode == "host":
            continue
        order, stamped, calls = log["index"][first:], log["stamped"][first:], log["calls"][first:]
        assert len(order) == len(seen_in) == 3
        if mode == "none":
            assert not any(stamped) and calls == ["resident_gather"] * 3
            continue
        assert all(stamped) and calls == ["resident_gather_aug"] * 3 and ds._augment is None
        for idxs, fl, gt in zip(order, seen_in, seen_gt):
            params = [A.draw(1, epoch, i, 1 << 31, 16, 0.2, 0.1) for i in idxs]
            _, want = A.batch(host_bytes[idxs], params, mean, std)
            assert _same_bits(fl, want[:, 3:23]) and _same_bits(gt.reshape(len(idxs), 1, 224, 224), want[:, 23:])
        if mode == "aug":
            first = len(log["index"])
            streamtrain.evaluate(DataLoader(ds, batch_size=3, shuffle=False, num_workers=0, collate_fn=ds.collate_fn), model,
                                 crit, 0, DEV, stream='temporal')
            assert not any(log["stamped"][first:]) and set(log["calls"][first:]) == {"resident_gather"}
    assert losses["none"] == losses["host"]
    assert losses["aug"] == losses["aug_again"] and losses["aug"] != losses["none"] and losses["aug"] != losses["aug_epoch5"]
