"""The affine resident gather on the GPU (egz_resident_gather_affine, hipops.resident_gather_aug with scale / rotate; DESIGN.md
section 21) against the numpy restatement tests/augment_affine_ref.py, bit for bit: explicit rows at the ends of both ranges with
flips and shifts, identity rows against egz_resident_gather_aug, the device-side draw, status bit 3, and SP.trainSP on a
resident dataset."""
import numpy as np
import pytest
import torch

import augment_affine_ref as R
import augment_ref as A
from test_hip_augment import _bits, _capture, _dev_same, _launch as _launch_aug, _new_sp, _refill, _same_bits, _spy
from test_hip_resident import DEV, _Arena, _case, _consts, _planes
from test_resident_host import resident_tree

pytestmark = pytest.mark.gpu
F = np.float32
ONE, ZERO = F(1.0), F(0.0)
TOP = np.nextafter(F(1.5), F(0))                          # the float just below 1.5
NAMED = [(ONE, ZERO), (ONE, R.QUARTER_PI), (ONE, -R.QUARTER_PI), (F(0.5), ZERO), (TOP, ZERO)]
RR10 = R.rotate_rad(10)


def _launch(pool, table, idx, H, W, image=None, flow=None, gt=None, nhwc=None, absmax=None, raw=None, raw_fields=7,
            params=None, params_out=None, epoch=0, seed=0, flip_thr=0, shift=0, contrast=0.0, brightness=0.0, scale=0.0,
            rot_rad=0.0):
    """egz_resident_gather_affine through the C ABI -> the status word."""
    from egaze_amd import hipops as Hp
    from egaze_amd._lib import check
    mean, std = (t.to(DEV) for t in _consts())
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    check(Hp.LIB.egz_resident_gather_affine(pool.data_ptr(), pool.shape[0], table.data_ptr(), table.shape[0], idx.data_ptr(),
                                            idx.numel(), H, W, mean.data_ptr(), std.data_ptr(), p(image), p(flow), p(gt),
                                            p(nhwc), p(absmax), p(raw), raw_fields, status.data_ptr(), seed, epoch, flip_thr,
                                            shift, contrast, brightness, p(params), p(params_out), scale, float(rot_rad),
                                            Hp._stream()), "egz_resident_gather_affine")
    torch.cuda.synchronize()
    return int(status.item())


def _padded(pool_h):
    """The pool on the device with two sentinel planes on each side: a read outside it shows in the result, not as a fault."""
    P, H, W = pool_h.shape
    big = torch.full((P + 4, H, W), 0x5A, dtype=torch.uint8, device=DEV)
    big[2:P + 2] = pool_h.to(DEV)
    return big[2:P + 2]


def _expected(pool_h, table_h, idx_h, params):
    """The restatement on the torch-gathered bytes -> (raw u8 (B,24,H,W), fp32 (B,24,H,W), nhwc (B,H,W,32), max |flow|)."""
    mean, std = _consts()
    u8 = pool_h[_planes(table_h, idx_h)].numpy()
    raw, f32 = R.batch(u8, params, mean.numpy(), std.numpy())
    B, _, H, W = f32.shape
    nhwc = np.zeros((B, H, W, 32), dtype=np.float32)
    nhwc[..., :20] = f32[:, 3:23].transpose(0, 2, 3, 1)
    return raw, f32, nhwc, np.abs(f32[:, 3:23]).max()


def _rows(H, W):
    """Identity, theta = +-pi/4, g = 0.5 and just below 1.5, each with and without a flip, unshifted and at every dy, dx of
    +-{1, size - 1, size + 3}; three mixed (g, theta) at the end.  The (g, theta) vary fastest, so a chunk of 3 holds identity
    and warped rows together."""
    dys = (0, 1, -1, H - 1, -(H - 1), H + 3, -(H + 3))
    dxs = (0, W - 1, -(W + 3), 1, W + 3, -1, -(W - 1))
    gain, bias = F(1.25), F(-0.1)
    rows = []
    for flip in (0, 1):
        for k, (dy, dx) in enumerate(zip(dys, dxs)):
            for g, t in NAMED:
                rows.append((flip, dy, dx, gain if k % 2 else ONE, bias if k % 3 == 1 else ZERO, g, t))
        for g, t in ((F(0.5), R.QUARTER_PI), (TOP, -R.QUARTER_PI), (F(0.9), F(0.2))):
            rows.append((flip, 2, -1, ONE, ZERO, g, t))
    return rows


SHAPES = [(H, W, B) for (H, W) in ((2, 4), (3, 8), (5, 12), (16, 16), (30, 36)) for B in (1, 3)] + [(16, 16, 32), (224, 224, 3)]


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_explicit_rows_bit_identical_with_the_restatement(H, W, B):
    """Every output form -- image, flow, ground truth, NHWC-32 with its abs-max, raw -- cut from sentinel-filled arenas, the
    pool between sentinel planes.  At 224 x 224 every fourth row of the list (the reference is the slow side)."""
    from egaze_amd import hipops as Hp
    P, N, HW = 11, 5, H * W
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=H * 1000 + W * 10 + B)
    pool, table, idx = _padded(pool_h), table_h.to(DEV), idx_h.to(DEV)
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
    pa = _Arena(torch.int32, -77, [B * 7])
    image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
    nhwc, raw, used = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W)), pa.cut(0, (B, 7))
    rows = _rows(H, W)[::4 if H == 224 else 1]
    rows += [R.IDENTITY] * (-len(rows) % B)
    for k in range(0, len(rows), B):
        chunk = rows[k:k + B]
        for a in (fa, ra, pa):
            _refill(a)
        am = Hp._new_absmax(torch.device(DEV))
        params = torch.from_numpy(R.rows(chunk)).to(DEV)
        assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params=params, params_out=used) == 0, chunk
        assert fa.sentinels_intact() and ra.sentinels_intact() and pa.sentinels_intact(), chunk
        want_raw, want, want_nhwc, want_am = _expected(pool_h, table_h, idx_h, chunk)
        assert torch.equal(raw.cpu(), torch.from_numpy(want_raw)), chunk
        assert _same_bits(image, want[:, :3]) and _same_bits(flow, want[:, 3:23]) and _same_bits(gt, want[:, 23:]), chunk
        assert _same_bits(nhwc, want_nhwc), chunk
        assert float(Hp.absmax_value(am)) == float(want_am), chunk
        assert torch.equal(used.cpu(), params.cpu()), chunk


@pytest.mark.parametrize("fields", [("image", "gt"), ("flow", "gt"), ("flow",), ("gt",)])
def test_field_subsets_write_only_their_fields(fields):
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 5, 12, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=5)
    if "image" not in fields:
        table_h[:, 0] = -1                                # what plan() leaves for a field not in use: never read
    if "flow" not in fields:
        table_h[:, 1:21] = -1
    if "gt" not in fields:
        table_h[:, 21] = -1
    chunk = [(1, 1, -2, F(0.75), F(0.125), F(0.8), F(0.3)), R.IDENTITY, (0, -2, 5, ONE, ZERO, F(1.3), -R.QUARTER_PI)]
    params = torch.from_numpy(R.rows(chunk)).to(DEV)
    pool, table, idx = _padded(pool_h), table_h.to(DEV), idx_h.to(DEV)
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
    # the wrapper: (B, 7) rows go to the affine entry; fp32 outputs of the fields asked for, None for the rest
    got, used = Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, fields=fields, params=params, want_params=True)
    assert used.shape == (B, 7) and torch.equal(used, params)
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


@pytest.mark.parametrize("H,W,B", [(2, 4, 1), (5, 12, 3), (30, 36, 3), (224, 224, 3), (16, 16, 32)])
def test_identity_rows_reproduce_the_integer_kernel(H, W, B):
    """g = 1, theta = 0 with flips, shifts, gains and biases -- as explicit rows and as the draw of a spec without scale and
    rotate -- against egz_resident_gather_aug on the same inputs: every output bit-identical, the abs-max included."""
    from egaze_amd import hipops as Hp
    HW = H * W
    pool_h, table_h, idx_h = _case(11, 5, B, H, W, seed=H + W + B)
    pool, table, idx = _padded(pool_h), table_h.to(DEV), idx_h.to(DEV)
    five = [(b % 2, (1, -(H - 1), H + 3, 0)[b % 4], (-(W + 3), 2, W - 1, -5)[b % 4], F(1.1), F(0.05)) for b in range(B)]
    drawn = dict(seed=3, epoch=4, flip_thr=1 << 31, shift=W + 3, contrast=0.2, brightness=0.1)
    for mode in ("explicit", "drawn"):
        outs = []
        for kernel in ("aug", "affine"):
            fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
            ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
            image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
            nhwc, raw = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W))
            am = Hp._new_absmax(torch.device(DEV))
            n = 5 if kernel == "aug" else 7
            used = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            kw = dict(drawn)
            if mode == "explicit":
                table7 = R.rows([f + (ONE, ZERO) for f in five])
                kw = dict(params=torch.from_numpy(np.ascontiguousarray(table7[:, :n])).to(DEV))
            launch = _launch_aug if kernel == "aug" else _launch
            assert launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params_out=used, **kw) == 0
            assert fa.sentinels_intact() and ra.sentinels_intact()
            outs.append((fa.buf, ra.buf, Hp.absmax_value(am).clone(), used))
        assert all(_dev_same(a, b) for a, b in zip(outs[0][:3], outs[1][:3])), mode
        assert torch.equal(outs[0][3], outs[1][3][:, :5]) and (outs[1][3][:, 5] == 0x3f800000).all(), mode
        assert ((outs[1][3][:, 6] & 0x7fffffff) == 0).all(), mode


@pytest.mark.parametrize("H,W", [(16, 16), (224, 224)])
def test_device_draw_equals_the_restatement_and_the_explicit_mode(H, W):
    """params_out for sample numbers that include 0 and a repeat, under the known answers' setting and two epochs; the outputs of
    the drawn mode equal the explicit mode fed with params_out; a second launch gives the same bits."""
    from egaze_amd import hipops as Hp
    P, N, HW = 11, 8, H * W
    pool_h, table_h, _ = _case(P, N, 6, H, W, seed=H)
    idx_h = torch.tensor([6, 0, 1, 6, 7, 3, 0], dtype=torch.int64)
    B = idx_h.numel()
    pool, table, idx = _padded(pool_h), table_h.to(DEV), idx_h.to(DEV)
    spec = Hp.AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=1, scale=0.15, rotate=10)
    assert _bits(torch.tensor([spec.rotate_rad])).item() == 0x3e32b8c2
    for epoch in (0, 3):
        want_rows = R.draw_rows(1, epoch, idx_h.tolist(), 1 << 31, 16, 0.2, 0.1, 0.15, RR10)
        if epoch == 0:                                    # the known answers of samples 6, 0, 1 (tests/test_augment_affine_host.py)
            assert np.ascontiguousarray(want_rows[:3, 5:]).view(np.uint32).tolist() == \
                [[0x3f7c35d8, 0x3df2ba26], [0x3f8f3a4f, 0x3d9b67d2], [0x3f5fb78d, 0xbdd4d9b6]]
        runs = []
        for mode in ("drawn", "drawn", "explicit"):
            fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
            ra = _Arena(torch.uint8, 0xA5, [B * 24 * HW])
            pa = _Arena(torch.int32, -77, [B * 7])
            image, flow, gt = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W))
            nhwc, raw, used = fa.cut(3, (B, H, W, 32)), ra.cut(0, (B, 24, H, W)), pa.cut(0, (B, 7))
            am = Hp._new_absmax(torch.device(DEV))
            kw = dict(params=runs[0][2].clone()) if mode == "explicit" else \
                dict(seed=1, flip_thr=1 << 31, shift=16, contrast=0.2, brightness=0.1, scale=0.15, rot_rad=RR10)
            assert _launch(pool, table, idx, H, W, image, flow, gt, nhwc, am, raw, params_out=used, epoch=epoch, **kw) == 0
            assert fa.sentinels_intact() and ra.sentinels_intact() and pa.sentinels_intact()
            assert torch.equal(used.cpu(), torch.from_numpy(want_rows)), (epoch, mode)
            assert torch.equal(used[0], used[3]) and torch.equal(used[1], used[6])       # the same sample, the same row
            runs.append((fa.buf, ra.buf, used, Hp.absmax_value(am).clone()))
        for other in runs[1:]:
            assert all(_dev_same(a, b) for a, b in zip(runs[0], other))
        want_raw, want, want_nhwc, _ = _expected(pool_h, table_h, idx_h, R.unrows(want_rows))
        assert torch.equal(raw.cpu(), torch.from_numpy(want_raw)) and _same_bits(nhwc, want_nhwc)
        assert _same_bits(torch.cat([image, flow, gt], dim=1), want)
    # the wrapper draws the same rows, whatever the batch around a sample; without scale / rotate it keeps its (B, 5) rows
    (_, _, _), rows_a = Hp.resident_gather_aug(pool, table, idx, spec, 3, want_params=True)
    (_, _, _), rows_b = Hp.resident_gather_aug(pool, table, idx[2:5].contiguous(), spec, 3, want_params=True)
    assert torch.equal(rows_a.cpu(), torch.from_numpy(want_rows)) and torch.equal(rows_b, rows_a[2:5])
    old = Hp.AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=1)
    (_, _, _), rows_c = Hp.resident_gather_aug(pool, table, idx, old, 3, want_params=True)
    assert rows_c.shape == (B, 5) and torch.equal(rows_c, rows_a[:, :5])


# ----------------------------------------------------------------------------- status
INF, NAN = 0x7f800000, 0x7fc00000
BAD_ROWS = {"g_low": (5, int(np.nextafter(F(0.5), F(0)).view(np.int32))), "g_high": (5, int(np.nextafter(F(1.5), F(2)).view(np.int32))),
            "g_negative": (5, int(F(-1.0).view(np.int32))), "g_inf": (5, INF), "g_nan": (5, NAN),
            "theta_high": (6, int(np.nextafter(R.QUARTER_PI, F(1)).view(np.int32))),
            "theta_low": (6, int(np.nextafter(-R.QUARTER_PI, F(-1)).view(np.int32))),
            "theta_minus_inf": (6, int(np.array([0xff800000], dtype=np.uint32).view(np.int32)[0])), "theta_nan": (6, NAN)}


@pytest.mark.parametrize("what", list(BAD_ROWS) + ["with_bit_0", "with_bit_1", "with_bit_2", "both_in_one_row"])
def test_bad_rows_are_refused_by_value(what):
    """Bit 3 for each cause, alone and together with bits 0 .. 2: the sample is skipped (its outputs keep the arena's fill), the
    others are right, the wrapper raises with the words of the status value."""
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 5, 12, 3, 11, 5
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=11)
    chunk = [(1, 1, -2, F(1.1), F(0.05), F(0.5), R.QUARTER_PI), (0, 2, 1, ONE, ZERO, F(1.2), F(-0.3)),
             (1, 0, 3, F(0.9), ZERO, F(1.5), -R.QUARTER_PI)]                     # both ends of both ranges are good rows
    rows = R.rows(chunk)
    bad, want = [1], 8
    if what == "with_bit_0":
        idx_h[0], want, bad = N + 5, 9, [0, 1]
        rows[1, 5] = INF
    elif what == "with_bit_1":
        idx_h[0], want, bad = 3, 10, [0, 1]
        table_h[3, 7] = P
        rows[1, 6] = NAN
    elif what == "with_bit_2":
        want, bad = 12, [0, 1]
        rows[0, 0] = 7
        rows[1, 5] = 0
    elif what == "both_in_one_row":
        want = 12
        rows[1, 1], rows[1, 6] = 40000, INF
    else:
        col, val = BAD_ROWS[what]
        rows[1, col] = val
    pool, table, idx = _padded(pool_h), table_h.to(DEV), idx_h.to(DEV)
    params = torch.from_numpy(rows).to(DEV)
    HW = H * W
    fa = _Arena(torch.float32, None, [B * 3 * HW, B * 20 * HW, B * HW, B * HW * 32])
    pa = _Arena(torch.int32, -77, [B * 7])
    image, flow, gt, nhwc = fa.cut(0, (B, 3, H, W)), fa.cut(1, (B, 20, H, W)), fa.cut(2, (B, 1, H, W)), fa.cut(3, (B, H, W, 32))
    used = pa.cut(0, (B, 7))
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
    assert Hp.AFFINE_STATUS[want] in str(e.value)


def test_the_wrapper_refuses_rows_that_do_not_fit_the_spec():
    from egaze_amd import hipops as Hp
    pool_h, table_h, idx_h = _case(11, 5, 3, 6, 12, seed=1)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    five = torch.from_numpy(A.rows([A.IDENTITY] * 3)).to(DEV)
    with pytest.raises(ValueError, match=r"\(3, 7\)"):
        Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(scale=0.1), 0, params=five)
    with pytest.raises(ValueError, match="params"):
        Hp.resident_gather_aug(pool, table, idx, Hp.AugSpec(), 0, params=torch.zeros((3, 6), dtype=torch.int32, device=DEV))
    pool_h, table_h, idx_h = _case(11, 5, 3, 6, 10, seed=1)
    with pytest.raises(RuntimeError, match="egz_resident_gather_affine: W = 10 must be a multiple of 4"):
        Hp.resident_gather_aug(pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV), Hp.AugSpec(rotate=5), 0)


# ----------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return resident_tree(tmp_path_factory.mktemp("augment_affine"))


@pytest.fixture(scope="module")
def host_bytes(tree):
    """(7, 24, H, W) uint8: the host dataset's planes of every sample."""
    from egaze_amd.data.STdatas import STDataset
    host = STDataset(*tree, raw_u8=True)
    return np.stack([np.concatenate([host[i][k].numpy() for k in ("image", "flow", "gt")]) for i in range(len(host))])


def test_sp_trainsp_with_scale_and_rotate(tree, host_bytes, tmp_path, monkeypatch):
    """One epoch of SP.trainSP with scale=0.2,rotate=10 on top of the other four: the batches the loop saw equal the
    restatement applied to the host dataset's bytes; validation afterwards is the unaugmented run's; augment=None still goes
    through the plain gather and gives the loss of an SP built the way it was before the argument existed."""
    from egaze_amd import hipops as Hp
    from egaze_amd.data.resident import ResidentSTDataset
    from test_hip_jpeg import _sp
    mean, std = (t.numpy() for t in _consts())
    ds = ResidentSTDataset(*tree, raw_u8=True, decode="gpu").fill(DEV)
    log = _spy(ds, monkeypatch)
    spec = Hp.AugSpec.parse("flip=0.5,shift=16,contrast=0.2,brightness=0.1,seed=1,scale=0.2,rotate=10")
    losses, state = {}, {}
    for mode in ("plain", "none", "aug"):
        sp = _sp(ds, str(tmp_path / mode)) if mode == "plain" else _new_sp(ds, str(tmp_path / mode), spec if mode == "aug" else None)
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
        if mode == "none":
            state["none"] = {k: v.clone() for k, v in sp.model.state_dict().items()}
            state["val"] = sp.testSP()
        if mode != "aug":
            continue
        assert all(stamped) and calls == ["resident_gather_aug"] * 3 and ds._augment is None
        warped = 0
        for idxs, (im, fl), gt in zip(order, seen_in, seen_gt):
            params = [R.draw(1, 3, i, 1 << 31, 16, 0.2, 0.1, 0.2, RR10) for i in idxs]
            warped += sum(R.matrices(p[5], p[6]) != (65536, 0, 65536, 0) for p in params)
            _, want = R.batch(host_bytes[idxs], params, mean, std)
            assert _same_bits(im, want[:, :3]) and _same_bits(fl, want[:, 3:23])
            assert _same_bits(gt.reshape(len(idxs), 1, 224, 224), want[:, 23:])
        assert warped == 7
        sp.model.load_state_dict(state["none"])
        first = len(log["index"])
        val = sp.testSP()
        assert np.array_equal(np.array([float(v) for v in val]), np.array([float(v) for v in state["val"]]), equal_nan=True)
        assert not any(log["stamped"][first:]) and set(log["calls"][first:]) == {"resident_gather"}
    assert losses["none"] == losses["plain"] and losses["aug"] != losses["none"]
