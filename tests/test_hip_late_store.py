"""egz_late_store on the GPU, through hipops.late_store: the planes it writes into a late-fusion pool against
hipops.late_input(sp, at, want_u8=True)'s planes and a plain index copy of the ground-truth planes (torch.equal, no
tolerance); scattered destinations into a 0xA5-filled pool (no stray write); skipped planes; plane numbers out of range; values
outside [0, 1]; the argument checks."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5

# (H, W), (h, w): the real geometry; H W no multiple of 4 (the element-wise lanes and the ragged last one); no resize
GEOMETRIES = [((224, 224), (14, 14)), ((6, 7), (3, 2)), ((8, 8), (8, 8))]
NS = (1, 3, 33)


def _map(n, hw, u8, seed):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (n,) + hw, generator=g, dtype=torch.uint8).to(DEV)
    x = torch.rand((n,) + hw, generator=g)
    k = min(x.numel(), 256)
    x.view(-1)[:k] = torch.arange(k, dtype=torch.float32) / 255        # the truncation's own grid points
    return x.to(DEV)


def _dst(n, P, seed, cols=3):
    """(n, 3) distinct plane numbers of a pool of P planes, scattered and non-monotonic."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(P, generator=g)[:cols * n].view(n, cols).to(torch.int64)


def _want(sp, at, dst, pool_before, gt_pool=None, gt_src=None, skip=()):
    """The pool late_store must leave: the reference's planes at the named destinations, everything else as it was."""
    from egaze_amd import hipops as Hp
    _, planes = Hp.late_input(sp, at, want_u8=True, status_to={})      # (n, 2, H, W): channel 0 the AT plane, 1 the SP plane
    want = pool_before.clone()
    for i in range(dst.shape[0]):
        if i in skip:
            continue
        for c, src in ((0, planes[i, 1]), (1, planes[i, 0]), (2, None if gt_pool is None else gt_pool[int(gt_src[i])])):
            if src is not None and int(dst[i, c]) != -1:
                want[int(dst[i, c])] = src
    return want


def _status(st):
    from egaze_amd import hipops as Hp
    return Hp.late_store_status(st['_late_store_status'])


@pytest.mark.parametrize("HW,hw", GEOMETRIES)
@pytest.mark.parametrize("n", NS)
def test_planes_equal_late_inputs_and_nothing_else_is_written(HW, hw, n):
    """All four dtype combinations per geometry and n; dst scattered into a 0xA5 pool; the ground truth from a second pool
    through non-monotonic, repeating source numbers; a device dst and a host dst."""
    from egaze_amd import hipops as Hp
    P, Q = 3 * n + 5, n + 2
    g = torch.Generator().manual_seed(n)
    gt_pool = torch.randint(0, 256, (Q,) + HW, generator=g, dtype=torch.uint8).to(DEV)
    gt_src = torch.randint(0, Q, (n,), generator=g, dtype=torch.int64)
    for k, (sp_u8, at_u8) in enumerate(itertools.product((False, True), repeat=2)):
        sp, at = _map(n, HW, sp_u8, 10 + k), _map(n, hw, at_u8, 20 + k)
        dst = _dst(n, P, 30 + k)
        pool = torch.full((P,) + HW, FILL, dtype=torch.uint8, device=DEV)
        want = _want(sp, at, dst, pool, gt_pool, gt_src)
        st = {}
        out = Hp.late_store(sp, at, pool, dst if k % 2 else dst.to(DEV), gt_pool=gt_pool, gt_src=gt_src.to(DEV), status_to=st)
        assert out is pool and _status(st) == 0
        assert torch.equal(pool, want), (sp_u8, at_u8)
        named = set(dst.flatten().tolist())
        assert all(bool((pool[p] == FILL).all()) for p in range(P) if p not in named)


@pytest.mark.parametrize("HW,hw", GEOMETRIES)
def test_an_unaligned_pool_takes_the_element_wise_path(HW, hw):
    """A pool that starts one byte into its buffer: no 4-byte store may be used, the bytes are the same."""
    from egaze_amd import hipops as Hp
    n, P = 3, 10
    sp, at = _map(n, HW, False, 1), _map(n, hw, False, 2)
    dst = _dst(n, P, 3)
    buf = torch.full((P * HW[0] * HW[1] + 1,), FILL, dtype=torch.uint8, device=DEV)
    pool = buf[1:].view((P,) + HW)
    gt_pool = torch.randint(0, 256, (n,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(DEV)
    gt_src = torch.arange(n, dtype=torch.int64, device=DEV)
    want = _want(sp, at, dst, pool, gt_pool, gt_src.cpu())
    st = {}
    Hp.late_store(sp, at, pool, dst, gt_pool=gt_pool, gt_src=gt_src, status_to=st)
    assert _status(st) == 0 and torch.equal(pool, want) and int(buf[0]) == FILL


@pytest.mark.parametrize("HW,hw", GEOMETRIES)
def test_minus_one_and_a_call_without_gt_pool_leave_their_planes_untouched(HW, hw):
    from egaze_amd import hipops as Hp
    n, P = 3, 12
    sp, at = _map(n, HW, False, 5), _map(n, hw, False, 6)
    gt_pool = torch.randint(0, 256, (n,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).to(DEV)
    gt_src = torch.tensor([2, 0, 1], dtype=torch.int64)
    dst = _dst(n, P, 8)
    dst[0, 0] = dst[1, 1] = dst[2, 2] = -1
    dst[1, 2] = -1
    pool = torch.full((P,) + HW, FILL, dtype=torch.uint8, device=DEV)
    want = _want(sp, at, dst, pool, gt_pool, gt_src)
    st = {}
    Hp.late_store(sp, at, pool, dst, gt_pool=gt_pool, gt_src=gt_src.to(DEV), status_to=st)
    assert _status(st) == 0 and torch.equal(pool, want)
    assert int((pool != FILL).flatten(1).any(1).sum()) <= 5            # 9 entries, 4 of them -1
    # a skipped map is not judged either: NaN behind a -1 raises no bit
    bad = sp.clone()
    bad[0] = float("nan")
    pool.fill_(FILL)
    Hp.late_store(bad, at, pool, dst, gt_pool=gt_pool, gt_src=gt_src.to(DEV), status_to=st)
    assert _status(st) == 0 and torch.equal(pool, want)
    # no gt_pool: the whole third column is skipped, whatever it holds
    dst = _dst(n, P, 9)
    dst[0, 2], dst[1, 2] = 10 ** 12, -7
    pool.fill_(FILL)
    want = _want(sp, at, dst, pool)
    Hp.late_store(sp, at, pool, dst, status_to=st)
    assert _status(st) == 0 and torch.equal(pool, want)
    assert int((pool != FILL).flatten(1).any(1).sum()) <= 2 * n


@pytest.mark.parametrize("where,value", [("dst0", "P"), ("dst1", "P+"), ("dst2", "P"), ("dst0", -2), ("dst1", -(2 ** 40)),
                                         ("dst2", -2), ("gt_src", "Q"), ("gt_src", -1), ("gt_src", -2), ("gt_src", 2 ** 40)])
def test_a_plane_number_out_of_range_skips_its_sample_and_raises_bit_2(where, value):
    from egaze_amd import hipops as Hp
    HW, hw, n, P, Q = (224, 224), (14, 14), 3, 9, 4
    value = {"P": P, "P+": P + 2 ** 33, "Q": Q}.get(value, value)
    sp, at = _map(n, HW, False, 11), _map(n, hw, False, 12)
    gt_pool = torch.randint(0, 256, (Q,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(13)).to(DEV)
    gt_src = torch.tensor([3, 1, 0], dtype=torch.int64)
    dst = _dst(n, P, 14)
    if where == "gt_src":
        gt_src[1] = value
    else:
        dst[1, int(where[-1])] = value
    pool = torch.full((P,) + HW, FILL, dtype=torch.uint8, device=DEV)
    want = _want(sp, at, dst, pool, gt_pool, gt_src, skip=(1,))
    st = {}
    Hp.late_store(sp, at, pool, dst, gt_pool=gt_pool, gt_src=gt_src.to(DEV), status_to=st)
    assert _status(st) == 4
    assert torch.equal(pool, want)
    for p in dst[1].tolist():                                           # the sample's three planes are untouched
        if 0 <= p < P:
            assert bool((pool[p] == FILL).all())
    with pytest.raises(RuntimeError, match="plane number"):             # without status_to the word is read at once
        Hp.late_store(sp, at, pool, dst, gt_pool=gt_pool, gt_src=gt_src.to(DEV))


def test_values_outside_the_domain_take_late_inputs_values_and_bits():
    from egaze_amd import hipops as Hp
    nan = float("nan")

    def both(sp, at):
        n = sp.shape[0]
        st_in, st = {}, {}
        _, planes = Hp.late_input(sp, at, want_u8=True, status_to=st_in)
        pool = torch.full((2 * n,) + tuple(sp.shape[1:]), FILL, dtype=torch.uint8, device=DEV)
        dst = torch.stack((torch.arange(n), n + torch.arange(n), torch.full((n,), -1)), 1)
        Hp.late_store(sp, at, pool, dst, status_to=st)
        assert torch.equal(pool[:n], planes[:, 1]) and torch.equal(pool[n:], planes[:, 0])
        status = _status(st)
        assert status == Hp.late_input_status(st_in['_late_input_status'])
        return pool, status

    clean = torch.full((1, 2, 2), 0.5, device=DEV)
    bad = torch.tensor([[[nan, -0.5], [1.5, float("inf")]]], device=DEV)
    pool, status = both(bad, clean)
    assert pool[0].flatten().tolist() == [0, 0, 255, 255] and pool[1].flatten().tolist() == [127] * 4 and status == 3
    pool, status = both(clean, bad)
    assert pool[1].flatten().tolist() == [0, 0, 255, 255] and status == 3
    for v, q, bit in ((nan, 0, 1), (-0.5, 0, 2), (1.5, 255, 2), (1.0, 255, 0)):
        for as_sp in (True, False):
            x = torch.full((1, 2, 2), v, device=DEV)
            pool, status = both(x, clean) if as_sp else both(clean, x)
            assert pool[0 if as_sp else 1].flatten().tolist() == [q] * 4 and status == bit, (v, as_sp)
    # through the resize: a NaN AT map is a zero plane (bit 0); one element out of range is judged at the map's own resolution
    sp = torch.full((2, 224, 224), 0.5, device=DEV)
    at = torch.full((2, 14, 14), 0.5, device=DEV)
    at[1] = nan
    pool, status = both(sp, at)
    assert status == 1 and bool((pool[3] == 0).all()) and bool((pool[2] == 127).all())
    at[1] = 0.5
    at[1, 13, 13] = -0.5
    assert both(sp, at)[1] == 2
    at[1, 13, 13] = 1.5
    pool, status = both(sp, at)
    assert status == 2 and int(pool[3, 223, 223]) == 255
    with pytest.warns(RuntimeWarning, match="NaN"):                      # read at once: bits 0 / 1 warn
        Hp.late_store(torch.full((1, 2, 2), nan, device=DEV), clean, torch.zeros((2, 2, 2), dtype=torch.uint8, device=DEV),
                      torch.tensor([[0, 1, -1]]))


def test_value_errors():
    from egaze_amd import hipops as Hp
    n, HW = 2, (8, 8)
    sp, at = torch.rand((n,) + HW, device=DEV), torch.rand((n,) + HW, device=DEV)
    pool = torch.zeros((8,) + HW, dtype=torch.uint8, device=DEV)
    gt_pool = torch.zeros((3,) + HW, dtype=torch.uint8, device=DEV)
    gt_src = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    dst = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64)
    ok = dict(sp=sp, at=at, late_pool=pool, dst=dst, gt_pool=gt_pool, gt_src=gt_src)
    Hp.late_store(**ok)
    assert not bool(pool[6:].any())
    bad = [
        ("float32 or uint8", dict(sp=sp.double())),
        ("float32 or uint8", dict(at=at.half())),
        ("uint8", dict(late_pool=pool.float())),                                     # wrong dtype
        ("uint8", dict(gt_pool=gt_pool.to(torch.int8))),
        ("int64", dict(dst=dst.to(torch.int32))),
        ("int64", dict(gt_src=gt_src.to(torch.int32))),
        ("HIP", dict(sp=sp.cpu())),                                                  # wrong device
        ("device", dict(late_pool=pool.cpu())),
        ("device", dict(gt_pool=gt_pool.cpu())),
        ("gt_src", dict(gt_src=gt_src.cpu())),
        ("contiguous", dict(late_pool=torch.zeros((8, 8, 16), dtype=torch.uint8, device=DEV)[:, :, ::2])),
        ("contiguous", dict(gt_pool=torch.zeros((3, 16, 8), dtype=torch.uint8, device=DEV)[:, ::2])),
        ("planes of", dict(late_pool=torch.zeros((8, 8, 4), dtype=torch.uint8, device=DEV))),    # another H x W than sp
        ("planes of", dict(gt_pool=torch.zeros((3, 4, 8), dtype=torch.uint8, device=DEV))),
        ("twice", dict(dst=torch.tensor([[0, 1, 2], [3, 1, 5]]))),                   # a plane named twice, across samples
        ("twice", dict(dst=torch.tensor([[0, 0, 2], [3, 4, 5]]).to(DEV))),           # ... within one, in a device dst
        ("twice", dict(dst=torch.tensor([[0, 1, 2], [3, 4, 2]]))),                   # ... in the ground-truth column
        ("go together", dict(gt_pool=None)),                                         # gt_src without gt_pool
        ("go together", dict(gt_src=None)),
        (r"\(2, 3\)", dict(dst=dst[:1])),
        ("gt_src", dict(gt_src=gt_src[:1])),
        ("overlaps", dict(gt_pool=pool[:3])),
        ("AT maps", dict(at=at[:1])),
    ]
    before = pool.clone()
    for match, over in bad:
        with pytest.raises(ValueError, match=match):
            Hp.late_store(**{**ok, **over})
    assert torch.equal(pool, before)
    # the ground-truth column is not read without gt_pool: the same plane there twice is no refusal
    Hp.late_store(sp, at, pool, torch.tensor([[0, 1, 7], [3, 4, 7]]))
    # -1 may repeat
    Hp.late_store(sp, at, pool, torch.tensor([[0, -1, -1], [-1, -1, -1]]), gt_pool=gt_pool, gt_src=gt_src)
