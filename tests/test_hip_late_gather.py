"""egz_late_gather on the GPU, through the raw C-ABI and through hipops.late_gather: bit-identity with the host expression
``pool[table[idx, c]].float().div(255)``, output subsets, 64-bit plane offsets, the bounds that refuse, the argument checks."""
import pytest
import torch

from test_hip_resident import _Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(P, N, B, H, W, seed):
    """A random pool whose first bytes run through all 256 values, a table with planes shared between samples and between the
    columns of one sample, the first and the last plane in use, and idx unsorted with repeats."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, 256, (P, H, W), dtype=torch.uint8, generator=g)
    n = min(256, pool.numel())
    pool.view(-1)[:n] = torch.arange(n, dtype=torch.int64).to(torch.uint8)
    table = torch.randint(0, P, (N, 3), dtype=torch.int64, generator=g)
    table[0] = torch.tensor([0, 0, P - 1])                             # one plane in both channels of fused
    table[1] = torch.tensor([P - 1, 0, 0])
    table[2] = table[1]                                                # a whole sample repeated
    table[3, 2] = table[3, 0]                                          # gt = pred
    head = [2] if B == 1 else [4, 1, 1] if B == 3 else [4, 1, 1, 0, 3]
    idx = torch.tensor(head + torch.randint(0, N, (B - len(head),), generator=g).tolist(), dtype=torch.int64)
    assert idx.numel() == B
    return pool, table, idx


def _reference(pool, table, idx):
    """-> (fused, gt, raw) on the host: the torch expression, channel 0 of fused the feat column, channel 1 the pred column."""
    col = lambda c: pool[table[idx, c]].float().div(255)
    raw = torch.stack([pool[table[idx, c]] for c in range(3)], dim=1)
    return torch.stack([col(1), col(0)], dim=1), col(2).unsqueeze(1), raw


def _launch(pool, table, idx, H, W, fused=None, gt=None, raw=None, B=None, P=None):
    """The raw entry point -> (return code, status word)."""
    from egaze_amd import hipops as Hp
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    rc = Hp._RAW_LIB.egz_late_gather(p(pool), pool.shape[0] if P is None else P, p(table), table.shape[0], p(idx),
                                     idx.numel() if B is None else B, H, W, p(fused), p(gt), p(raw), status.data_ptr(),
                                     Hp._stream())
    torch.cuda.synchronize()
    return rc, int(status.item())


def _arenas(B, HW):
    return _Arena(torch.float32, None, [B * 2 * HW, B * HW]), _Arena(torch.uint8, 0xA5, [B * 3 * HW])


# (H, W, B): one 4-byte group; a tail inside one block; two blocks per sample with a tail and more samples than a wave has
# lanes / 2; the training geometry
SHAPES = [(2, 2, 1), (6, 10, 3), (16, 68, 33), (224, 224, 5)]


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_gather_bit_identical_with_the_host_expression(H, W, B):
    P, N, HW = 11, 6, H * W
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=H * 1000 + W * 10 + B)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa, ra = _arenas(B, HW)
    fused, gt, raw = fa.cut(0, (B, 2, H, W)), fa.cut(1, (B, 1, H, W)), ra.cut(0, (B, 3, H, W))
    assert _launch(pool, table, idx, H, W, fused, gt, raw) == (0, 0)
    assert fa.sentinels_intact() and ra.sentinels_intact()
    want_fused, want_gt, want_raw = _reference(pool_h, table_h, idx_h)
    assert torch.equal(raw.cpu(), want_raw)
    assert torch.equal(fused.cpu(), want_fused) and torch.equal(gt.cpu(), want_gt)
    # the wrapper: the same tensors, contiguous, the order LF passes to late_fusion
    from egaze_amd import hipops as Hp
    f2, g2 = Hp.late_gather(pool, table, idx)
    assert f2.shape == (B, 2, H, W) and g2.shape == (B, 1, H, W) and f2.is_contiguous() and g2.is_contiguous()
    assert torch.equal(f2, fused) and torch.equal(g2, gt)
    assert torch.equal(Hp.late_gather(pool, table, idx, raw=True).cpu(), want_raw)
    assert torch.equal(f2, Hp.cat2_planes(f2[:, 0:1].contiguous(), f2[:, 1:2].contiguous()))


def test_every_byte_value_is_the_correctly_rounded_quotient():
    """One plane with all 256 byte values in all three columns: the division, not a multiply by the reciprocal (which differs at
    126 of the 256 values)."""
    from egaze_amd import hipops as Hp
    plane = torch.arange(256, dtype=torch.int64).to(torch.uint8).view(1, 16, 16)
    table = torch.zeros((1, 3), dtype=torch.int64)
    fused, gt = Hp.late_gather(plane.to(DEV), table.to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    want = plane.float().div(255)
    assert torch.equal(fused[0, 0].cpu(), want[0]) and torch.equal(fused[0, 1].cpu(), want[0])
    assert torch.equal(gt[0, 0].cpu(), want[0])
    recip = plane.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert int((recip != want).sum()) == 126


@pytest.mark.parametrize("which", ["fused", "gt", "raw"])
def test_output_subsets_write_nothing_else(which):
    """Each output alone: the others are not passed, and their columns of the table are not even looked at."""
    H, W, B, P, N = 6, 10, 3, 11, 6
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=5)
    want = dict(zip(("fused", "gt", "raw"), _reference(pool_h, table_h, idx_h)))
    if which == "fused":
        table_h[:, 2] = -1                                             # never read
    elif which == "gt":
        table_h[:, :2] = P
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa, ra = _arenas(B, H * W)
    outs = {"fused": fa.cut(0, (B, 2, H, W)), "gt": fa.cut(1, (B, 1, H, W)), "raw": ra.cut(0, (B, 3, H, W))}
    assert _launch(pool, table, idx, H, W, **{which: outs[which]}) == (0, 0)
    assert fa.sentinels_intact() and ra.sentinels_intact()
    assert torch.equal(outs[which].cpu(), want[which])
    for other in outs:
        if other == which:
            continue
        o = outs[other]
        assert bool((torch.isnan(o) if o.dtype == torch.float32 else o == 0xA5).all()), other


def test_offsets_above_2_gib_and_4_gib():
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory for a pool above 4 GiB, {free >> 30} GiB are free")
    from egaze_amd import hipops as Hp
    H = W = 16
    P = (1 << 32) // 256 + 24
    flat = torch.empty((1 << 32) + 24 * 256, dtype=torch.uint8, device=DEV)
    pool = flat.view(P, H, W)
    # planes whose byte offsets are just past 2^31, just past 2^32, and the pool's last and first
    planes = [(1 << 31) // 256 + 1, (1 << 32) // 256 + 1, P - 1, 0]
    known = torch.randint(0, 256, (4, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    for k, p in enumerate(planes):
        assert (p * 256 > (1 << 31)) == (k < 3) and (p * 256 > (1 << 32)) == (k in (1, 2))
        pool[p] = known[k].to(DEV)
    table_h = torch.tensor([[planes[0], planes[1], planes[2]], [planes[2], planes[3], planes[0]]], dtype=torch.int64)
    idx_h = torch.tensor([1, 0], dtype=torch.int64)
    where = {p: k for k, p in enumerate(planes)}
    pick = lambda c: known[torch.tensor([where[int(table_h[i, c])] for i in idx_h])]
    fused, gt = Hp.late_gather(pool, table_h.to(DEV), idx_h.to(DEV))
    assert torch.equal(fused[:, 0].cpu(), pick(1).float().div(255))
    assert torch.equal(fused[:, 1].cpu(), pick(0).float().div(255))
    assert torch.equal(gt[:, 0].cpu(), pick(2).float().div(255))
    raw = Hp.late_gather(pool, table_h.to(DEV), idx_h.to(DEV), raw=True)
    assert torch.equal(raw.cpu(), torch.stack([pick(0), pick(1), pick(2)], dim=1))
    del flat, pool


@pytest.mark.parametrize("what", ["idx_high", "idx_negative", "table_high", "table_negative"])
def test_bad_indices_are_refused_not_dereferenced(what):
    """A bounds check that refuses: the bad sample is skipped (its outputs keep the arena's fill), the status word says why,
    the wrapper raises, the other samples of the batch are right."""
    from egaze_amd import hipops as Hp
    H, W, B, P, N = 6, 10, 3, 11, 6
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=11)
    bad, want = 1, 2
    if what == "idx_high":
        idx_h[bad], want = N, 1
    elif what == "idx_negative":
        idx_h[bad], want = -1, 1
    elif what == "table_high":
        idx_h[bad] = 5
        table_h[5, 1] = P
    else:
        idx_h[bad] = 5
        table_h[5, 2] = -(1 << 40)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa, ra = _arenas(B, H * W)
    fused, gt, raw = fa.cut(0, (B, 2, H, W)), fa.cut(1, (B, 1, H, W)), ra.cut(0, (B, 3, H, W))
    assert _launch(pool, table, idx, H, W, fused, gt, raw) == (0, want)
    assert fa.sentinels_intact() and ra.sentinels_intact()
    good = [b for b in range(B) if b != bad]
    want_fused, want_gt, want_raw = _reference(pool_h, table_h, idx_h[good])
    assert torch.equal(fused.cpu()[good], want_fused) and torch.equal(gt.cpu()[good], want_gt)
    assert torch.equal(raw.cpu()[good], want_raw)
    assert bool(torch.isnan(fused[bad]).all()) and bool(torch.isnan(gt[bad]).all()) and bool((raw[bad] == 0xA5).all())
    with pytest.raises(RuntimeError, match="sample was skipped"):
        Hp.late_gather(pool, table, idx)
    sample = {}
    Hp.late_gather(pool, table, idx, status_to=sample)                 # deferred: raised at hand-over
    from egaze_amd.data.STdatas import check_decode_status
    with pytest.raises(RuntimeError, match="sample was skipped"):
        check_decode_status(sample)
    if what == "table_negative":                                       # the ground-truth column is not one of fused's
        fa2, _ = _arenas(B, H * W)
        f2 = fa2.cut(0, (B, 2, H, W))
        assert _launch(pool, table, idx, H, W, fused=f2) == (0, 0)
        assert torch.equal(f2.cpu(), _reference(pool_h, table_h.clamp(min=0), idx_h)[0]) and fa2.sentinels_intact()


def test_both_status_bits_in_one_batch():
    H, W, B, P, N = 6, 10, 3, 11, 6
    pool_h, table_h, idx_h = _case(P, N, B, H, W, seed=13)
    idx_h[0], idx_h[2] = N + 3, 5
    table_h[5, 0] = P + 7
    fa, _ = _arenas(B, H * W)
    fused, gt = fa.cut(0, (B, 2, H, W)), fa.cut(1, (B, 1, H, W))
    assert _launch(pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV), H, W, fused, gt) == (0, 3)
    want_fused, want_gt, _ = _reference(pool_h, table_h, idx_h[1:2])
    assert torch.equal(fused.cpu()[1:2], want_fused) and torch.equal(gt.cpu()[1:2], want_gt)
    assert bool(torch.isnan(fused[[0, 2]]).all()) and bool(torch.isnan(gt[[0, 2]]).all()) and fa.sentinels_intact()


def test_argument_checks_return_errors_and_write_nothing():
    from egaze_amd import hipops as Hp
    H, W, B = 6, 10, 3
    pool_h, table_h, idx_h = _case(11, 6, B, H, W, seed=17)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fa, ra = _arenas(B, H * W)
    fused, gt, raw = fa.cut(0, (B, 2, H, W)), fa.cut(1, (B, 1, H, W)), ra.cut(0, (B, 3, H, W))
    err = lambda: Hp._RAW_LIB.egz_last_error().decode()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = dict(pool=pool.data_ptr(), P=11, table=table.data_ptr(), N=6, idx=idx.data_ptr(), B=B, H=H, W=W,
                fused=fused.data_ptr(), gt=gt.data_ptr(), raw=raw.data_ptr(), status=status.data_ptr(), stream=None)
    for over, word in ((dict(pool=None), "pool"), (dict(table=None), "table"), (dict(idx=None), "idx"),
                       (dict(status=None), "status"), (dict(H=3, W=3), "multiple of 4"), (dict(B=0), "B = 0"),
                       (dict(fused=None, gt=None, raw=None), "no output")):
        rc = Hp._RAW_LIB.egz_late_gather(*{**full, **over}.values())
        assert rc != 0 and err().startswith("egz_late_gather") and word in err(), (over, rc, err())
    torch.cuda.synchronize()
    assert bool(torch.isnan(fused).all()) and bool(torch.isnan(gt).all()) and bool((raw == 0xA5).all())
    assert int(status.item()) == 0
    for bad in (pool[:, :, :5], pool.to(torch.int32), pool.cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            Hp.late_gather(bad, table, idx)
    with pytest.raises(ValueError, match="table"):
        Hp.late_gather(pool, table[:, :2].contiguous(), idx)
    with pytest.raises(ValueError, match="idx"):
        Hp.late_gather(pool, table, idx.to(torch.int32))


@pytest.mark.parametrize("H,W,B", [(6, 10, 3), (224, 224, 5)])
def test_equals_u8_normalize_of_the_gathered_bytes(H, W, B):
    from egaze_amd import hipops as Hp
    pool_h, table_h, idx_h = _case(11, 6, B, H, W, seed=23)
    pool, table, idx = pool_h.to(DEV), table_h.to(DEV), idx_h.to(DEV)
    fused, gt = Hp.late_gather(pool, table, idx)
    raw = Hp.late_gather(pool, table, idx, raw=True)
    norm = Hp.u8_normalize(raw, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))      # columns pred, feat, gt
    assert torch.equal(fused[:, 0], norm[:, 1]) and torch.equal(fused[:, 1], norm[:, 0]) and torch.equal(gt[:, 0], norm[:, 2])
    one = Hp.u8_normalize(raw[:, 2:3].contiguous(), (0.0,), (1.0,))     # lateDataset's map as stage_batch normalises a gt
    assert torch.equal(gt, one)
