"""The AT / late-fusion glue kernels of csrc/glue.hip one by one: crop_mean, window_mean, pixel_weighted_sum, weighted_minmax,
u8_center_of_mass, bilinear_up, cat2_planes, u8_normalize.

The tests that ran them so far use B = 2 .. 4, C = 512, 14 x 14 maps and three or four hand-picked gaze points against fp32 host
code at 1e-6-class tolerances; the capped grids of bilinear_up / cat2_planes / u8_normalize never took a second pass of their
loops, weighted_minmax never saw C % 64 != 0 or HW around 256, u8_center_of_mass never needed its 64-bit totals.

References are fp64 (numpy / torch-double on the CPU, scipy for the centre of mass) from the same fp32 operands.
* The three window sums are compared element by element with a DERIVED bar: the standard bound of recursive summation,
  (n + 1) 2^-24 sum |terms| (divided by n for a mean), which holds with or without a fused multiply-add; on the test's inputs
  (features |N(0,1)| + 0.1) one dropped term moves a result by at least 10 bounds (asserted).
* weighted_minmax and bilinear_up: 4 x the run-time distance of the host fp32 formulation from fp64 (the project's allowance
  for another valid fp32 order), max |got - ref| over max |ref|.
* The centre of mass, the concatenation, the normalisation and every min / max / NaN statement are bit for bit.
Figures: profiles/b1_glue_tests.txt."""
import gc
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
FACTOR = 4
AXIS = [v for k in range(14) for v in (16 * k, 16 * k + 15)]            # both ends of every 16-pixel cell: 28 values
OUTSIDE = [-17, -16, -1, 224, 239, 1000]


def H():
    import egaze_amd.hipops as h
    return h


@pytest.fixture(autouse=True)
def cpu_threads():
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        torch.set_num_threads(keep)
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


def features(shape, seed):
    """|N(0,1)| + 0.1: every term of a window sum is at least 0.1"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).abs() + 0.1


def within_bound(tag, got, ref, bound, smallest_term):
    """|got - ref| <= bound element by element; ``smallest_term``: the least any dropped term would move a result."""
    err = (got.double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"\n{tag}: worst error {err.max().item():.2e} = {worst:.3f} bounds; largest bound {bound.max().item():.2e}; "
          f"a dropped term moves a result by >= {smallest_term:.2e} = {smallest_term / bound.max().item():.0f} bounds")
    assert smallest_term >= 10 * bound.max().item(), f"{tag}: a dropped term is not 10 bounds"
    assert worst <= 1.0, f"{tag}: {int((err > bound).sum())} results outside the summation bound, worst {worst:.2f} bounds"


# ---------------------------------------------------------------------------------------------- crop_mean
def crop_points(axis):
    return [[y, x] for y in axis for x in axis]


def crop_ref64(base, pts, size, crop):
    """fp64 mean and sum |terms| of the host crop of sample b = map b % len(base) around pts[b] -> (mean (B, C), sum |.| (B, C))"""
    nb = base.shape[0]
    mean = torch.empty(len(pts), base.shape[1], dtype=torch.float64)
    for r in range(nb):
        idx = list(range(r, len(pts), nb))
        c = crop(base[r:r + 1].expand(len(idx), -1, -1, -1), [pts[i] for i in idx], size).double()
        assert tuple(c.shape[2:]) == (size, size)
        mean[idx] = c.mean((2, 3))
    return mean, mean * size * size                       # (positive features: sum |terms| = sum)


@pytest.mark.parametrize("C", [512, 5])
def test_crop_mean_every_cell_edge_and_size(C):
    """A square 14 x 14 map, gaze points = all 28 x 28 combinations of {16 k, 16 k + 15} plus rows and columns outside the image
    ({-17, -16, -1, 224, 239, 1000}: 34 x 34 = 1156 points in one batch), sizes 1, 2, 3, 4, 5, 13, 14, against the fp64 mean of
    AT.crop_feature's crop.  B C = 5780 at C = 5 is no multiple of the 256-thread block (at C = 512 every B C is).  Gaze points
    that are already an int32 device tensor give the same bits as host lists."""
    h = H()
    from egaze_amd.AT import crop_feature
    pts = crop_points(AXIS + OUTSIDE)
    B, nb = len(pts), 8
    base = features((nb, C, 14, 14), seed=31 + C)
    fd = base.permute(0, 2, 3, 1).contiguous().to(DEV)[torch.arange(B, device=DEV) % nb].contiguous()
    assert (B * C) % 256 != 0 or C == 512
    gp_dev = torch.tensor(pts, dtype=torch.int32, device=DEV)
    for size in (1, 2, 3, 4, 5, 13, 14):
        got = h.crop_mean(fd, pts, size)
        assert torch.equal(h.crop_mean(fd, gp_dev, size), got)
        ref, sabs = crop_ref64(base, pts, size, crop_feature)
        n = size * size
        within_bound(f"crop_mean C={C} size={size}", got.cpu(), ref, (n + 1) * U * sabs / n, base.min().item() / n)


def test_crop_mean_rectangular_map_and_refusals():
    """A 9 x 14 map against the C-ABI's documented rule (rows clipped by H, columns by W; AT.crop_feature clips both by H, its
    maps are square); a window larger than the map is refused."""
    h = H()
    from egaze_amd._lib import EgazeHipError
    Hh, Ww, C = 9, 14, 5

    def crop(feature, maxind, size):
        lo, hi = size // 2, int(math.ceil(size / 2.0))
        out = []
        for b in range(feature.size(0)):
            fy = min(max(maxind[b][0] // 16, lo), Hh - hi)
            fx = min(max(maxind[b][1] // 16, lo), Ww - hi)
            out.append(feature[b:b + 1, :, fy - lo:fy + hi, fx - lo:fx + hi])
        return torch.cat(out, 0)
    pts = crop_points(AXIS + OUTSIDE)
    B, nb = len(pts), 8
    base = features((nb, C, Hh, Ww), seed=77)
    fd = base.permute(0, 2, 3, 1).contiguous().to(DEV)[torch.arange(B, device=DEV) % nb].contiguous()
    for size in (1, 2, 3, 4, 5, 8, 9):
        ref, sabs = crop_ref64(base, pts, size, crop)
        n = size * size
        within_bound(f"crop_mean 9x14 size={size}", h.crop_mean(fd, pts, size).cpu(), ref, (n + 1) * U * sabs / n,
                     base.min().item() / n)
    for size in (10, 14, 0):
        with pytest.raises(EgazeHipError):
            h.crop_mean(fd, pts, size)
    sq = features((2, 14, 14, 5), seed=1).to(DEV)
    with pytest.raises(EgazeHipError):
        h.crop_mean(sq, [[0, 0], [5, 5]], 15)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- window_mean
def test_window_mean_every_window_of_the_map():
    """All 105 x 105 half-open windows of a 14 x 14 map in one batch (C = 8, B C = 88200: no multiple of 256) against fp64."""
    h = H()
    spans = [(a, b) for a in range(14) for b in range(a + 1, 15)]
    wins = [(y0, y1, x0, x1) for y0, y1 in spans for x0, x1 in spans]
    B, nb, C = len(wins), 16, 8
    assert B == 105 * 105 and (B * C) % 256 != 0
    base = features((nb, 14, 14, C), seed=5)
    fd = base.to(DEV)[torch.arange(B, device=DEV) % nb].contiguous()
    got = h.window_mean(fd, wins).cpu()
    S = torch.zeros(nb, 15, 15, C, dtype=torch.float64)                 # integral image: exact to 1e-16 of the sum in fp64
    S[:, 1:, 1:] = base.double().cumsum(1).cumsum(2)
    w = torch.tensor(wins)
    r = torch.arange(B) % nb
    y0, y1, x0, x1 = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
    tot = S[r, y1, x1] - S[r, y0, x1] - S[r, y1, x0] + S[r, y0, x0]
    n = ((y1 - y0) * (x1 - x0)).double()[:, None]
    # (the bound is per window; the smallest dropped term against the LARGEST bound of its own window size)
    ratio = (base.min().item() / n) / ((n + 1) * U * tot / n)
    print(f"\nwindow_mean: a dropped term is >= {ratio.min().item():.0f} bounds")
    assert ratio.min().item() >= 10
    err = (got.double() - tot / n).abs() / ((n + 1) * U * tot / n)
    print(f"window_mean 11025 windows x 8 channels: worst error {err.max().item():.3f} bounds")
    assert err.max().item() <= 1.0, f"{int((err > 1).sum())} results outside the summation bound"


def test_window_mean_wrapper_validation():
    h = H()
    fd = features((2, 14, 14, 8), seed=2).to(DEV)
    for bad in ([(0, 0, 0, 1), (0, 1, 0, 1)], [(0, 1, 3, 3), (0, 1, 0, 1)],            # empty
                [(0, 15, 0, 1), (0, 1, 0, 1)], [(0, 1, -1, 1), (0, 1, 0, 1)], [(0, 1, 0, 15), (0, 1, 0, 1)],   # out of range
                [(5, 4, 0, 1), (0, 1, 0, 1)],                                          # reversed
                [(0, 1, 0, 1)], [(0, 1, 0, 1)] * 3):                                   # wrong count
        with pytest.raises(ValueError):
            h.window_mean(fd, bad)
    assert tuple(h.window_mean(fd, [(0, 14, 0, 14), (13, 14, 13, 14)]).shape) == (2, 8)


# ---------------------------------------------------------------------------------------------- pixel_weighted_sum
ALIGN_POINTS = [[0, 0], [0, 223], [223, 0], [223, 223], [112, 112], [111, 113], [5, 220], [23, 24], [24, 23], [199, 200],
                [200, 199], [-40, 300], [1000, -1], [117, 60]]


@pytest.mark.parametrize("C", [512, 5])
def test_pixel_weighted_sum_against_fp64(C):
    """HW = 196 with the weights of AT.align_window_weights (sizes 1, 3, 5) at the four corners, the centre and points that are
    clipped, against the fp64 dot product of the same fp32 operands; one dropped term of the window's interior (a cell with at
    least a quarter of the largest weight; the cells on the window's rim can weigh 1e-6 of that) is 10 bounds or more.  Then
    maps with zero and negative weights, where only the bound is asserted."""
    h = H()
    from egaze_amd.AT import align_window_weights
    wm = torch.tensor(np.stack([align_window_weights(p, s) for s in (1, 3, 5) for p in ALIGN_POINTS]), dtype=torch.float32)
    B = wm.shape[0]
    g = torch.Generator().manual_seed(8)
    signed = torch.randn(B, 14, 14, generator=g) * (torch.rand(B, 14, 14, generator=g) < 0.5)
    assert bool((signed == 0).any()) and bool((signed < 0).any())
    feat = features((B, 14, 14, C), seed=40 + C)
    fd = feat.to(DEV)
    for tag, w in (("align weights", wm), ("zeros and negative weights", signed)):
        got = h.pixel_weighted_sum(fd, w).cpu()
        terms = w.double().view(B, 196, 1) * feat.double().view(B, 196, C)
        bound = (196 + 1) * U * terms.abs().sum(1)
        if w is wm:
            assert abs(w.double().sum((1, 2)) - 1).max().item() < 1e-6
            inner = (w >= 0.25 * w.amax((1, 2), keepdim=True)).view(B, 196, 1)
            smallest = torch.where(inner, terms.abs(), torch.full_like(terms, float("inf"))).amin(1)
            assert bool((smallest >= 10 * bound).all()), "a dropped interior term is not 10 bounds"
        within_bound(f"pixel_weighted_sum C={C} {tag}", got, terms.sum(1), bound, float("inf"))


def test_pixel_weighted_sum_is_the_aligned_crop_mean():
    """End to end: the device sum with align_window_weights' fp64 weights (rounded to fp32 by the wrapper: one more rounding per
    term, (n + 2) 2^-24 sum |terms|) against fp64 interpolate(align_corners=True) + crop + mean, AT.crop_align_feature."""
    h = H()
    from egaze_amd.AT import align_window_weights, crop_align_feature
    B, C = len(ALIGN_POINTS), 24
    feat = features((B, C, 14, 14), seed=91)
    pts = ALIGN_POINTS
    for size in (1, 3, 5):
        wm = np.stack([align_window_weights(p, size) for p in pts])
        got = h.pixel_weighted_sum(feat.permute(0, 2, 3, 1).contiguous().to(DEV), wm).cpu()
        ref = crop_align_feature(feat.double(), pts, size).mean((2, 3))
        sabs = (torch.tensor(wm).view(B, 1, 196) * feat.double().view(B, C, 196)).abs().sum(2)
        bound = (196 + 2) * U * sabs + 1e-13 * sabs              # (+ the fp64 reference's own interpolation rounding)
        within_bound(f"aligned crop mean size={size}", got, ref, bound, float("inf"))


# ---------------------------------------------------------------------------------------------- weighted_minmax
MINMAX_SHAPES = [(1, 196, 512), (33, 196, 512), (3, 196, 5), (3, 196, 64), (3, 196, 65), (3, 196, 130), (2, 3, 512), (2, 255, 8),
                 (2, 256, 8), (2, 257, 8), (1, 4096, 4)]


def minmax_host(w, feat_nchw):
    from egaze_amd.AT import get_weighted_batch
    assert not feat_nchw.is_cuda
    return get_weighted_batch(w, feat_nchw)


def minmax_dev(h, w, feat_nchw):
    return h.weighted_minmax(feat_nchw.permute(0, 2, 3, 1).contiguous().to(DEV), w.to(DEV)).cpu()


@pytest.mark.parametrize("B,HW,C", MINMAX_SHAPES)
def test_weighted_minmax_against_fp64(B, HW, C):
    """Non-negative features and weights at every (B, HW, C) that takes another path (C % 64, HW around the 256-thread block, the
    4096 limit) against the fp64 of AT.get_weighted_batch's host lines; bar = 4 x the distance of the host fp32 branch, at least
    10 x below the loss of one 64-channel pass of the channel sum; min exactly 0, max exactly 1 in every map, also with weights
    of either sign."""
    h = H()
    g = torch.Generator().manual_seed(B * 100000 + HW * 10 + C)
    feat = features((B, C, HW, 1), seed=B + HW + C)
    w = torch.rand(B, C, generator=g) + 0.05
    got = minmax_dev(h, w, feat)
    ref = minmax_host(w.double(), feat.double())
    cpu32 = minmax_host(w, feat)
    err, dc = (got.double() - ref).abs().max().item(), (cpu32.double() - ref).abs().max().item()       # (max |ref| is 1)
    bar = FACTOR * dc
    s = (feat.double() * w.double().view(B, C, 1, 1))
    defects = []
    for c0 in range(0, C, 64) if C > 64 else ():
        f = s.sum(1) - s[:, c0:c0 + 64].sum(1)
        f = f - f.flatten(1).min(1)[0].view(-1, 1, 1)
        defects.append((f / f.flatten(1).max(1)[0].view(-1, 1, 1) - ref).abs().flatten(1).max(1)[0].min().item())
    defect = min(defects) if defects else float("inf")
    print(f"\nweighted_minmax B={B} HW={HW} C={C}: error {err:.2e}, host fp32 {dc:.2e}, bar {bar:.2e}, one 64-channel pass lost {defect:.1e}")
    assert defect >= 10 * bar
    flat = got.flatten(1)
    assert bool((flat.min(1)[0] == 0.0).all()) and bool((flat.max(1)[0] == 1.0).all())
    assert err <= bar, f"error {err:.3e} above the bar {bar:.3e}"
    ws = w * torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
    flat = minmax_dev(h, ws, feat).flatten(1)
    assert bool((flat.min(1)[0] == 0.0).all()) and bool((flat.max(1)[0] == 1.0).all())


def test_weighted_minmax_degenerate_maps_and_refusal():
    """A constant map (weights k / 8 and features 0.75: every partial sum is exact, so all sums are equal in any order) is
    0 / 0 = NaN everywhere, like the reference; a one-pixel map too; 4097 pixels do not fit the LDS stage."""
    h = H()
    from egaze_amd._lib import EgazeHipError
    feat = torch.full((2, 8, 14, 14), 0.75)
    w = torch.stack((torch.arange(1, 9) / 8.0, torch.arange(8, 0, -1) / 4.0))
    got = minmax_dev(h, w, feat)
    assert bool(torch.isnan(got).all()) and bool(torch.isnan(minmax_host(w, feat)).all())
    one = features((3, 8, 1, 1), seed=4)
    assert bool(torch.isnan(minmax_dev(h, torch.ones(3, 8), one)).all()) and bool(torch.isnan(minmax_host(torch.ones(3, 8), one)).all())
    with pytest.raises(EgazeHipError):
        minmax_dev(h, torch.ones(1, 4), features((1, 4, 4097, 1), seed=5))
    torch.cuda.synchronize()


@pytest.mark.parametrize("HW,C", [(196, 512), (257, 8), (3, 65)])
def test_weighted_minmax_nonfinite_features_follow_torch_min_max(HW, C):
    """The expectation is the host branch on the same values, i.e. torch.min / torch.max, which PROPAGATE a NaN: one NaN feature
    makes that pixel's sum NaN, the minimum NaN and with it the whole map; +inf leaves 0 everywhere and NaN at its own pixel;
    -inf (and both) make everything NaN.  Maps without a non-finite value in the same batch are untouched."""
    h = H()
    nan, inf = float("nan"), float("inf")
    plant = [[(0, nan)], [(HW - 1, nan)], [(HW // 2, nan)], [(1, inf)], [(HW - 2, -inf)], [(0, inf), (HW - 1, -inf)],
             [(0, inf), (1, inf)], [(2, nan), (0, inf)], []]
    B = len(plant)
    feat = features((B, C, HW, 1), seed=HW + C)
    for b, spots in enumerate(plant):
        for k, (p, v) in enumerate(spots):
            feat[b, (7 * p + k) % C, p, 0] = v
    w = torch.rand(B, C, generator=torch.Generator().manual_seed(3)) + 0.05
    want = minmax_host(w, feat)
    got = minmax_dev(h, w, feat)
    for b in (0, 1, 2, 4, 5, 7):
        assert bool(torch.isnan(want[b]).all()), b
    assert int(torch.isnan(want[3]).sum()) == 1 and int(torch.isnan(want[6]).sum()) == 2 and not bool(torch.isnan(want[8]).any())
    bad = [b for b in range(B) if not torch.equal(torch.isnan(got[b]), torch.isnan(want[b]))]
    assert not bad, f"maps {bad}: NaN pattern differs from torch.min / torch.max: " + \
        ", ".join(f"map {b}: {int(torch.isnan(got[b]).sum())} NaN, reference {int(torch.isnan(want[b]).sum())}" for b in bad)
    assert bool((got[3][~torch.isnan(got[3])] == 0).all()) and bool((got[6][~torch.isnan(got[6])] == 0).all())
    assert torch.equal(got[8], minmax_dev(h, w[8:9], feat[8:9])[0]), "a clean map changes with its neighbours in the batch"
    ref8 = minmax_host(w[8:9].double(), feat[8:9].double())[0]                  # and the clean map against fp64, as above
    err, dc = (got[8].double() - ref8).abs().max().item(), (want[8].double() - ref8).abs().max().item()
    print(f"\nweighted_minmax HW={HW} C={C}, the clean map beside non-finite ones: error {err:.2e}, host fp32 {dc:.2e}")
    assert err <= FACTOR * dc


# ---------------------------------------------------------------------------------------------- u8_center_of_mass
def com_maps(Hh, Ww, seed):
    """name -> (Hh, Ww) fp32 map in [0, 1]"""
    n = Hh * Ww
    maps = {"ones": torch.ones(Hh, Ww), "zeros": torch.zeros(Hh, Ww)}
    for name, p in (("corner00", 0), ("corner0W", Ww - 1), ("cornerH0", n - Ww), ("last", n - 1), ("flat255", 255 % n),
                    ("flat256", 256 % n)):
        m = torch.zeros(n)
        m[p] = 1.0 if p % 2 else 0.5
        maps[name] = m.view(Hh, Ww)
    m = torch.zeros(Hh, Ww)
    m[1, 2] = m[Hh - 2, Ww - 3] = 0.6                                    # symmetric about the centre: an exact (half-)integer
    maps["symmetric"] = m
    lv = np.arange(256, dtype=np.float32) / np.float32(255)
    lv = np.clip(np.concatenate([lv, np.nextafter(lv, np.float32(-1)), np.nextafter(lv, np.float32(2))]), 0, 1).astype(np.float32)
    m = torch.zeros(n)
    pos = (torch.arange(lv.size) * 61) % n                               # 768 levels spread over the map
    m[pos] = torch.from_numpy(lv)
    maps["levels"] = m.view(Hh, Ww)
    g = torch.Generator().manual_seed(seed)
    maps["random"] = torch.rand(Hh, Ww, generator=g)
    maps["dim"] = torch.rand(Hh, Ww, generator=g) * 0.02
    return maps


def scipy_com(m):
    from scipy import ndimage
    q = (m.numpy() * 255).astype(np.uint8)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        com = np.array(ndimage.center_of_mass(q), dtype=np.float64)
    gp = np.where(np.isnan(com), 0, np.floor(np.nan_to_num(com))).astype(np.int32)
    return com, gp, q


@pytest.mark.parametrize("Hh,Ww", [(224, 224), (448, 448), (13, 7)])
def test_u8_center_of_mass_bit_for_bit_with_scipy(Hh, Ww):
    """com, gp and q8 equal scipy.ndimage.center_of_mass((m * 255).astype(uint8)) bit for bit: all ones (com exactly
    (111.5, 111.5) at 224 x 224), all zero (NaN, gp 0), one lit pixel at each corner and at flat indices 255 / 256 / last, two
    symmetric pixels, every float32(k / 255) with both neighbours, random and nearly black maps; each alone (B = 1) and all in a
    batch of 33; 13 x 7: H W % 256 != 0 and W no power of two.
    The all-ones row total at 224 x 224 is 255 x 224 x sum(0 .. 223) = 1,426,629,120: it still fits 32 bits.  448 x 448 is the
    size at which the 64-bit totals are needed (11,436,779,520 > 2^32, com exactly (223.5, 223.5)); the random map there
    (5.7e9) needs them too."""
    h = H()
    maps = com_maps(Hh, Ww, seed=Hh)
    want = {k: scipy_com(m) for k, m in maps.items()}
    if (Hh, Ww) == (224, 224):
        assert want["ones"][0].tolist() == [111.5, 111.5]
    if (Hh, Ww) == (448, 448):
        assert want["ones"][0].tolist() == [223.5, 223.5] and 255 * 448 * sum(range(448)) > 2 ** 32
        q = want["random"][2].astype(np.int64)
        assert (q * np.arange(448)[:, None]).sum() > 2 ** 32 and (q * np.arange(448)[None, :]).sum() > 2 ** 32
    assert np.isnan(want["zeros"][0]).all() and want["symmetric"][0].tolist() == [(Hh - 1) / 2, (Ww - 1) / 2]

    def check(tag, maps_b, names):
        d = maps_b.to(DEV)
        com, gp, q = h.u8_center_of_mass(d, want_u8=True)
        com2, gp2 = h.u8_center_of_mass(d)
        com, gp, q, com2, gp2 = (t.cpu().numpy() for t in (com, gp, q, com2, gp2))
        assert np.array_equal(com, com2, equal_nan=True) and np.array_equal(gp, gp2), tag
        for b, k in enumerate(names):
            wc, wg, wq = want[k]
            assert np.array_equal(q[b], wq), (tag, k)
            assert np.array_equal(com[b].view(np.int64), wc.view(np.int64)) or (np.isnan(wc).all() and np.isnan(com[b]).all()), (tag, k, com[b], wc)
            assert np.array_equal(gp[b], wg), (tag, k, gp[b], wg)
    for k, m in maps.items():
        check("B=1", m[None], [k])
    order = [list(maps)[i % len(maps)] for i in range(33)]
    check("B=33", torch.stack([maps[k] for k in order]), order)


# ---------------------------------------------------------------------------------------------- bilinear_up
@pytest.mark.parametrize("align", [False, True], ids=["half-pixel", "align-corners"])
@pytest.mark.parametrize("h_,w_,scale,B", [(14, 14, 16, 3), (14, 14, 16, 33), (7, 5, 3, 3), (1, 9, 2, 3), (9, 1, 2, 3), (4, 4, 1, 3)])
def test_bilinear_up_against_fp64(h_, w_, scale, B, align):
    """fp64 interpolate, bar = 4 x the distance of torch's CPU fp32 interpolate, max |got - ref| over the maps' max.  B = 33 at
    14 x 14 x 16: 1,655,808 outputs, the 4096 x 256 grid takes a second pass.  Then into a strided destination: plane 1 of a
    (B, 2, H, W) buffer with a pad between the samples, everything NaN before; plane 0 and the pad stay NaN, plane 1 has the
    dense result's bits."""
    h = H()
    src = torch.rand(B, h_, w_, generator=torch.Generator().manual_seed(h_ * 100 + w_ + B))
    kw = dict(scale_factor=scale, mode="bilinear", align_corners=align)
    ref = torch.nn.functional.interpolate(src.double()[:, None], **kw)[:, 0]
    cpu32 = torch.nn.functional.interpolate(src[:, None], **kw)[:, 0]
    got = h.bilinear_up(src.to(DEV), scale, align_corners=align)
    Hh, Ww = h_ * scale, w_ * scale
    assert tuple(got.shape) == (B, Hh, Ww)
    if B * Hh * Ww > 4096 * 256:
        assert B == 33
    scale_ = ref.abs().max().item()
    err, dc = (got.cpu().double() - ref).abs().max().item() / scale_, (cpu32.double() - ref).abs().max().item() / scale_
    print(f"\nbilinear_up {h_}x{w_} x{scale} B={B} align={align}: error {err:.2e}, torch CPU fp32 {dc:.2e}, bar {FACTOR * dc:.2e}")
    assert err <= FACTOR * dc
    pad = 12
    buf = torch.full((B, 2 * Hh * Ww + pad), float("nan"), device=DEV)
    dst = torch.as_strided(buf, (B, Hh, Ww), (2 * Hh * Ww + pad, Ww, 1), Hh * Ww)
    out = h.bilinear_up(src.to(DEV), scale, align_corners=align, out=dst)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    assert torch.equal(buf[:, Hh * Ww:2 * Hh * Ww].reshape(B, Hh, Ww), got)
    assert bool(torch.isnan(buf[:, :Hh * Ww]).all()) and bool(torch.isnan(buf[:, 2 * Hh * Ww:]).all())


# ---------------------------------------------------------------------------------------------- cat2_planes, u8_normalize
def test_cat2_planes_past_the_grid_cap_and_scalar_route():
    """B = 96 at 224 x 224: 1,204,224 float4 items, past the 4096 x 256 of the capped grid; an odd-size plane (13 x 7, B = 5)
    through the one-float kernel.  Bit for bit torch.cat."""
    h = H()
    g = torch.Generator(device=DEV).manual_seed(6)
    for B, Hh, Ww in ((96, 224, 224), (5, 13, 7)):
        f = torch.randn(B, 1, Hh, Ww, generator=g, device=DEV)
        w = torch.randn(B, 1, Hh, Ww, generator=g, device=DEV)
        if Hh * Ww % 4 == 0:
            assert B * Hh * Ww // 4 > 4096 * 256
        got = h.cat2_planes(f, w)
        assert torch.equal(got.cpu(), torch.cat((f.cpu(), w.cpu()), dim=1)), (B, Hh, Ww)


def test_u8_normalize_past_the_grid_cap():
    """(9, 20, 224, 224) bytes: 2,257,920 quads, just past the 8192 x 256 of the capped grid, so the loop and the channel index
    run at a wrapped position; 20 different (mean, std) pairs; bit for bit the torch expression on the CPU."""
    h = H()
    src = torch.randint(0, 256, (9, 20, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(12))
    assert src.numel() // 4 > 8192 * 256
    mean = [0.30 + 0.017 * c for c in range(20)]
    std = [0.20 + 0.013 * c for c in range(20)]
    got = h.u8_normalize(src.to(DEV), mean, std).cpu()
    m = torch.tensor(mean, dtype=torch.float32).view(20, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(20, 1, 1)
    want = (src.float().div(255) - m) / s
    assert torch.equal(got, want), f"{int((got != want).sum())} values differ"
