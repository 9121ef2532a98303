"""egz_late_input and egz_draw_ring on the GPU: the device hand-over against the composition it replaces ((255 * x).to(uint8) ->
resize_linear_u8 -> .float().div(255) -> cat((at, sp), 1)), against late_gather of the same planes, its defined behaviour
outside [0, 1]; the ring against the integer inequality in numpy; the argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64

# (h, w) -> (H, W): the predictor's geometry; odd sizes with H W no multiple of 4 (the element-wise lanes); no resize
GEOMETRIES = [((14, 14), (224, 224)), ((5, 7), (37, 50)), ((224, 224), (224, 224))]


def _specials():
    """Every k / 255 with its two fp32 neighbours (the truncation flips there), 0 and 1."""
    k = (torch.arange(256, dtype=torch.float32) / 255).numpy()
    vals = np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2)), np.float32([0.0, 1.0])])
    return torch.from_numpy(vals.astype(np.float32))


def _maps(B, hw, seed, lo=0):
    """(B, h, w) fp32 in [0, 1]: the special values from position ``lo`` on (as many as fit), then seeded uniform values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B,) + tuple(hw), generator=g)
    s = _specials()[lo:]
    n = min(s.numel(), x.numel())
    x.view(-1)[:n] = s[:n]
    return x


def _quant(x):
    return (255 * x).to(torch.uint8)


def _reference(sp, at, HW):
    """The hand-over as the stages do it today -> (fused, planes) on the device."""
    from egaze_amd import hipops as Hp
    q_sp, q_at = _quant(sp).to(DEV), _quant(at).to(DEV)
    if tuple(q_at.shape[1:]) != tuple(HW):
        q_at = Hp.resize_linear_u8(q_at, HW)
    planes = torch.stack((q_at, q_sp), 1)
    # the division on the host, where data.lateDataset does it (a true division; a device-side div by a scalar may multiply by
    # the reciprocal)
    q_at, q_sp = q_at.cpu(), q_sp.cpu()
    return torch.cat((q_at.unsqueeze(1).float().div(255), q_sp.unsqueeze(1).float().div(255)), 1).to(DEV), planes


def _launch_into_guarded(sp, at):
    """The raw entry point writing into NaN / 0xA5-filled buffers with guards -> (fused, planes, status)."""
    from egaze_amd import hipops as Hp
    B, H, W = sp.shape
    h, w = at.shape[1:]
    n = B * 2 * H * W
    fbuf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    pbuf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    fused, planes = fbuf[GUARD:GUARD + n].view(B, 2, H, W), pbuf[GUARD:GUARD + n].view(B, 2, H, W)
    tabs = (None,) * 4 if (h, w) == (H, W) else Hp._linear_tables(sp.device, (h, w), (H, W), "test")
    p = lambda t: None if t is None else t.data_ptr()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = Hp._RAW_LIB.egz_late_input(sp.data_ptr(), int(sp.dtype == torch.uint8), at.data_ptr(), int(at.dtype == torch.uint8), B, H,
                                    W, h, w, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(tabs[3]), fused.data_ptr(), planes.data_ptr(),
                                    status.data_ptr(), Hp._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(fbuf[:GUARD]).all()) and bool(torch.isnan(fbuf[GUARD + n:]).all())
    assert bool((pbuf[:GUARD] == 0xA5).all()) and bool((pbuf[GUARD + n:] == 0xA5).all())
    assert not bool(torch.isnan(fused).any())                                  # written in full
    return fused, planes, int(status.item())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw,HW", GEOMETRIES)
def test_equals_todays_hand_over(hw, HW, B):
    from egaze_amd import hipops as Hp
    seed = 100 * hw[0] + 10 * HW[1] + B
    sp_h = _maps(B, HW, seed)
    at_h = _maps(B, hw, seed + 1, lo=(37 * seed) % 500)
    # (the lower neighbour of 0 / 255 is a negative denormal: it truncates to 0 either way, and is counted: status bit 1)
    sp, at = sp_h.to(DEV), at_h.to(DEV)
    want_fused, want_planes = _reference(sp_h, at_h, HW)
    fused, planes, status = _launch_into_guarded(sp, at)
    assert torch.equal(planes, want_planes), (planes != want_planes).nonzero()[:8].tolist()
    assert torch.equal(fused, want_fused), (fused != want_fused).nonzero()[:8].tolist()
    assert status == (2 if bool((sp_h < 0).any() or (at_h < 0).any()) else 0)
    st = {}
    f2, p2 = Hp.late_input(sp, at, want_u8=True, status_to=st)
    assert f2.shape == (B, 2) + tuple(HW) and f2.is_contiguous() and p2.is_contiguous()
    assert torch.equal(f2, want_fused) and torch.equal(p2, want_planes)
    assert Hp.late_input_status(st['_late_input_status']) == status
    assert torch.equal(Hp.late_input(sp, at, status_to={}), want_fused)         # without the planes
    # uint8 inputs: the same fused as the fp32 maps they were quantised from, resized or not, mixed or both
    q_sp, q_at = _quant(sp_h).to(DEV), _quant(at_h).to(DEV)
    for a, b in ((q_sp, q_at), (sp, q_at), (q_sp, at)):
        f3, p3 = Hp.late_input(a, b, want_u8=True, status_to={})
        assert torch.equal(f3, want_fused) and torch.equal(p3, want_planes)


def test_every_special_value_through_the_resized_at_plane():
    """4 x 14 x 14 = 784 elements hold all 770 special values: the AT plane is quantised at its source resolution."""
    from egaze_amd import hipops as Hp
    at_h = _maps(4, (14, 14), 5)
    assert _specials().numel() <= at_h.numel()
    sp_h = _maps(4, (224, 224), 6, lo=3)
    want_fused, want_planes = _reference(sp_h, at_h, (224, 224))
    fused, planes = Hp.late_input(sp_h.to(DEV), at_h.to(DEV), want_u8=True, status_to={})
    assert torch.equal(fused, want_fused) and torch.equal(planes, want_planes)


def test_channel_order():
    """Channel 0 is the AT map, channel 1 the SP map: late_fusion's order as LF.trainLate passes it."""
    from egaze_amd import hipops as Hp
    sp = torch.full((2, 224, 224), 0.25, device=DEV)
    at = torch.full((2, 14, 14), 0.75, device=DEV)
    fused, planes = Hp.late_input(sp, at, want_u8=True)
    assert bool((planes[:, 0] == 191).all()) and bool((planes[:, 1] == 63).all())
    assert bool((fused[:, 0] == torch.tensor(191.0) / 255).all()) and bool((fused[:, 1] == torch.tensor(63.0) / 255).all())


@pytest.mark.parametrize("hw,HW,B", [((14, 14), (224, 224), 3), ((8, 12), (8, 12), 2)])
def test_bit_identical_with_late_gather_of_the_same_planes(hw, HW, B):
    """The predictor's LF input is the tensor LF trains on: late_gather over a pool of the hand-over planes."""
    from egaze_amd import hipops as Hp
    sp, at = _maps(B, HW, 11).to(DEV), _maps(B, hw, 12, lo=100).to(DEV)
    fused, planes = Hp.late_input(sp, at, want_u8=True, status_to={})
    pool = planes.view(2 * B, *HW)
    # table columns: SP prediction, AT map, ground truth (any plane)
    table = torch.tensor([[2 * b + 1, 2 * b, 0] for b in range(B)], dtype=torch.int64, device=DEV)
    gathered, _ = Hp.late_gather(pool, table, torch.arange(B, dtype=torch.int64, device=DEV))
    assert torch.equal(gathered, fused)


def test_values_outside_the_domain_are_defined_and_counted():
    from egaze_amd import hipops as Hp
    nan, inf = float("nan"), float("inf")
    clean = torch.full((1, 2, 2), 0.5, device=DEV)

    def run(sp, at):
        st = {}
        fused, planes = Hp.late_input(sp, at, want_u8=True, status_to=st)
        return planes, fused, Hp.late_input_status(st['_late_input_status'])

    bad = torch.tensor([[[nan, -0.5], [1.5, inf]]], device=DEV)
    for as_sp in (True, False):                       # through the SP path and through the unresized AT path
        planes, fused, status = run(bad, clean) if as_sp else run(clean, bad)
        assert planes[0, 1 if as_sp else 0].flatten().tolist() == [0, 0, 255, 255] and status == 3
        assert planes[0, 0 if as_sp else 1].flatten().tolist() == [127] * 4
        assert torch.equal(fused.cpu(), planes.cpu().float().div(255))
    for v, q, bit in ((nan, 0, 1), (-0.5, 0, 2), (-inf, 0, 2), (1.5, 255, 2), (inf, 255, 2), (1.01, 255, 2),
                      (1.003, 255, 0), (1.0, 255, 0), (-0.0, 0, 0)):
        planes, _, status = run(torch.full((1, 2, 2), v, device=DEV), clean)
        assert planes[0, 1].flatten().tolist() == [q] * 4 and status == bit, v
    # a NaN AT map (weighted_minmax of a constant feature map: 0 / 0) through the resize: a zero plane, bit 0
    sp = torch.full((2, 224, 224), 0.5, device=DEV)
    at = torch.full((2, 14, 14), 0.5, device=DEV)
    at[1] = nan
    planes, fused, status = run(sp, at)
    assert status == 1 and bool((planes[1, 0] == 0).all()) and bool((planes[0, 0] == 127).all())
    assert not bool(torch.isnan(fused).any())
    at[1] = 0.5
    at[1, 13, 13] = 7.0                               # one element out of range, in the last corner of the source
    planes, _, status = run(sp, at)
    assert status == 2 and int(planes[1, 0, 223, 223]) == 255
    assert run(sp, torch.full((2, 14, 14), 0.5, device=DEV))[2] == 0
    # without status_to the word is read at once and a non-zero one warns
    with pytest.warns(RuntimeWarning, match="NaN"):
        Hp.late_input(torch.full((1, 2, 2), nan, device=DEV), clean)


# ----------------------------------------------------------------------------- draw_ring
def _ring_numpy(images, centers, r_in, r_out, colour):
    out = images.copy()
    M, H, W, _ = out.shape
    yy, xx = np.mgrid[:H, :W].astype(np.int64)
    for m in range(M):
        d2 = (yy - int(centers[m][0])) ** 2 + (xx - int(centers[m][1])) ** 2
        out[m][(d2 >= r_in * r_in) & (d2 <= r_out * r_out)] = colour
    return out


@pytest.mark.parametrize("H,W", [(40, 56), (224, 224)])
@pytest.mark.parametrize("r_in,r_out", [(6, 9), (0, 5), (0, 0), (3, 3)])
def test_draw_ring_against_numpy(H, W, r_in, r_out):
    from egaze_amd import hipops as Hp
    rng = np.random.RandomState(H + r_out)
    colour = (10, 200, 255)
    sets = [[(H // 2, W // 3), (0, W - 1), (H + 4, -3)],                         # inside, on a border / corner, outside: partly clipped
            [(H - 1, 7), (-r_out, W // 2), (5, W + r_out)],                      # border; outside, touching in one pixel each
            [(-100, -100), (H + 50, W // 2), (2 ** 30, -2 ** 30)]]               # wholly clipped, also far away
    for k, centers in enumerate(sets):
        images = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
        want = _ring_numpy(images, centers, r_in, r_out, colour)
        if k == 2:
            assert np.array_equal(want, images)
        else:
            assert not np.array_equal(want[0], images[0])
        dev = torch.from_numpy(images).to(DEV)
        got = Hp.draw_ring(dev, torch.tensor(centers, dtype=torch.int32, device=DEV), r_in, r_out, colour)
        assert got is dev and np.array_equal(dev.cpu().numpy(), want), (k, centers)
    one = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=DEV)
    Hp.draw_ring(one, torch.tensor([[H // 2, W // 2]], dtype=torch.int32, device=DEV), r_in, r_out)
    assert np.array_equal(one.cpu().numpy(), _ring_numpy(np.zeros((1, H, W, 3), np.uint8), [(H // 2, W // 2)], r_in, r_out,
                                                         (255, 255, 255)))


# ----------------------------------------------------------------------------- refusals
class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_refusals_launch_nothing(monkeypatch):
    import importlib
    from egaze_amd import hipops as Hp
    sp, at = torch.zeros((2, 8, 8), device=DEV), torch.zeros((2, 4, 4), device=DEV)
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    cen = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    Hp.late_input(sp, at)
    Hp.draw_ring(img, cen, 1, 2)                                                  # the good calls pass
    monkeypatch.setattr(importlib.import_module("egaze_amd.hipops.handover"), "LIB", _NoLaunch())
    bad_inputs = [
        (sp.cpu(), at), (sp, at.cpu()),                                           # CPU tensors
        (sp.double(), at), (sp, at.to(torch.int32)), (sp.half(), at),             # wrong dtypes
        (sp, at[:1]), (sp[:1], at),                                               # mismatched batch sizes
        (sp.transpose(1, 2), at), (sp, torch.zeros((2, 4, 8), device=DEV)[:, :, ::2]),     # non-contiguous
        (sp[0], at), (sp, at.unsqueeze(1)), (sp, torch.zeros((2, 0, 4), device=DEV)),       # wrong rank, empty
    ]
    for a, b in bad_inputs:
        with pytest.raises(ValueError):
            Hp.late_input(a, b)
    with pytest.raises(ValueError, match="2x decimation"):
        Hp.late_input(torch.zeros((1, 4, 4), device=DEV), torch.zeros((1, 8, 8), device=DEV))
    bad_rings = [
        (img.cpu(), cen, 1, 2, (0, 0, 0)), (img, cen.cpu(), 1, 2, (0, 0, 0)),
        (img.float(), cen, 1, 2, (0, 0, 0)), (img, cen.long(), 1, 2, (0, 0, 0)), (img, cen.float(), 1, 2, (0, 0, 0)),
        (img, cen[:1], 1, 2, (0, 0, 0)), (img[:1], cen, 1, 2, (0, 0, 0)),
        (img.permute(0, 2, 1, 3), cen, 1, 2, (0, 0, 0)), (img, torch.zeros((2, 4), dtype=torch.int32, device=DEV)[:, ::2], 1, 2, (0, 0, 0)),
        (img[..., 0], cen, 1, 2, (0, 0, 0)),
        (img, cen, 3, 2, (0, 0, 0)), (img, cen, -1, 2, (0, 0, 0)), (img, cen, 1.5, 2, (0, 0, 0)),
        (img, cen, 1, 2, (0, 0, 256)), (img, cen, 1, 2, (0, 0)),
    ]
    for args in bad_rings:
        with pytest.raises(ValueError):
            Hp.draw_ring(*args)
