"""Host-side pieces of the feature visualisation (vis_features.py): the numpy restatements the GPU kernels are checked against
(OpenCV's 8-bit INTER_LINEAR resize from hipops.linear_table, the float64 blend of the overlay, the reference's crop window),
their properties, the argument checks that need no device, and -- where cv2 is importable -- the restatements against cv2
itself.  Also the seeded synthetic inputs that tests/golden/make_golden_vis.py and tests/test_hip_vis.py share."""
import hashlib

import numpy as np
import pytest
import torch

from egaze_amd import hipops as H
from egaze_amd.vis_features import crop_window

FRAME = 224


# ----------------------------------------------------------------------------- restatements
def resize_linear(img, out_hw):
    """cv2.resize(img, (W', H')) with INTER_LINEAR for uint8 (H, W) or (H, W, C) images: the tables of hipops.linear_table,
    then OpenCV's integer passes (HResizeLinear, the uchar VResizeLinear)."""
    img = np.asarray(img, dtype=np.uint8)
    sh, sw = img.shape[:2]
    dh, dw = out_hw
    xo, xa = H.linear_table(sw, dw, "x")
    yo, ya = H.linear_table(sh, dh, "y")
    a0, a1 = xa[0::2].astype(np.int64), xa[1::2].astype(np.int64)
    b0, b1 = ya[0::2].astype(np.int64), ya[1::2].astype(np.int64)
    x1 = np.minimum(xo + 1, sw - 1)
    src = img.astype(np.int64)
    if src.ndim == 2:
        src = src[:, :, None]
    rows = (src[:, xo] * a0[None, :, None] + src[:, x1] * a1[None, :, None])        # (sh, dw, C): S of every source row
    r0, r1 = np.clip(yo, 0, sh - 1), np.clip(yo + 1, 0, sh - 1)
    S0, S1 = rows[r0], rows[r1]
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    out = out.astype(np.uint8)
    return out[:, :, 0] if img.ndim == 2 else out


def blend(heat, img):
    """numpy's ``heatmap * 0.3 + img * 0.5`` in float64, then OpenCV's convertTo(CV_8U): round half to even, saturated."""
    v = np.asarray(heat, dtype=np.uint8) * 0.3 + np.asarray(img, dtype=np.uint8) * 0.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def overlay(map_u8, frame_chw, lut):
    """The reference's resize -> applyColorMap -> blend of one map over one (3, H, W) BGR frame -> (H, W, 3) BGR uint8."""
    frame = np.asarray(frame_chw).transpose(1, 2, 0)
    heat = np.asarray(lut)[resize_linear(map_u8, frame.shape[:2])]
    return blend(heat, frame)


def cell_argmax(gt_hw, cell=16):
    """First arg-max of the exact integer cell sums of a (H, W) uint8 map (row-major, numpy's tie rule)."""
    g = np.asarray(gt_hw, dtype=np.int64)
    ch, cw = g.shape[0] // cell, g.shape[1] // cell
    s = g[:ch * cell, :cw * cell].reshape(ch, cell, cw, cell).sum((1, 3))
    return int(np.argmax(s.reshape(-1)))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ----------------------------------------------------------------------------- seeded synthetic inputs
def synth_inputs(seed, n, hw=FRAME):
    """n frames of the raw_u8 loader: 'image' (n, 3, hw, hw) BGR bytes, 'flow' (n, 20, hw, hw) bytes, 'gt' (n, 1, hw, hw) bytes
    holding one Gaussian blob centred in a cell whose row and column lie in 3 .. hw / 16 - 3 (so every crop window has 6 x 6
    cells and the cell is the unique arg-max), and the chosen cells."""
    rs = np.random.RandomState(seed)
    image = rs.randint(0, 256, size=(n, 3, hw, hw)).astype(np.uint8)
    flow = rs.randint(0, 256, size=(n, 20, hw, hw)).astype(np.uint8)
    nc = hw // 16
    cells = rs.randint(3, nc - 2, size=(n, 2))
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64)
    gt = np.empty((n, 1, hw, hw), np.uint8)
    for k, (r, c) in enumerate(cells):
        d2 = (yy - (16 * r + 7.5)) ** 2 + (xx - (16 * c + 7.5)) ** 2
        gt[k, 0] = np.floor(255 * np.exp(-d2 / (2 * 18.0 ** 2))).astype(np.uint8)
    return {'image': image, 'flow': flow, 'gt': gt, 'cells': cells[:, 0] * nc + cells[:, 1]}


def random_lut(seed):
    return np.random.RandomState(seed).randint(0, 256, size=(256, 3)).astype(np.uint8)


# ----------------------------------------------------------------------------- tables and integer passes
def test_linear_table_14_to_224_by_hand():
    xo, xa = H.linear_table(14, 224, "x")
    yo, ya = H.linear_table(14, 224, "y")
    # d = 0: f = 0.5 / 16 - 0.5 = -0.46875 -> floor -1, f = 0.53125; x clamps to (0, 0), y keeps the coefficients
    assert (xo[0], xa[0], xa[1]) == (0, 2048, 0)
    assert (yo[0], ya[0], ya[1]) == (-1, 960, 1088)
    # d = 8: f = 8.5 / 16 - 0.5 = 0.03125 -> (0, 1984, 64)
    assert (xo[8], xa[16], xa[17]) == (0, 1984, 64)
    # the right edge: d = 223 -> f = 13.46875, s = 13 = ssize - 1 -> x clamps (13, f = 0)
    assert (xo[223], xa[446], xa[447]) == (13, 2048, 0)
    assert (yo[223], ya[446], ya[447]) == (13, 1088, 960)
    assert np.all(xa[0::2].astype(int) + xa[1::2] == 2048)


def test_linear_table_rounds_half_to_even():
    # 3 -> 2: f = (d + 0.5) * 1.5 - 0.5 = 0.25, 2.75 -> coefficients 1536 / 512 exactly; 5 -> 3: f = 1/3 steps
    _, a = H.linear_table(5, 3, "y")
    f = np.float32((np.arange(3) + 0.5) * (5 / 3) - 0.5)
    f = np.float32(f - np.floor(f))
    assert np.array_equal(a[1::2], np.rint(f * np.float32(2048)).astype(np.int16))


@pytest.mark.parametrize("shape", [(14, 14), (1, 1), (7, 5), (30, 17, 3)])
def test_identity_size_returns_input(shape):
    img = np.random.RandomState(1).randint(0, 256, size=shape).astype(np.uint8)
    assert np.array_equal(resize_linear(img, shape[:2]), img)


@pytest.mark.parametrize("src,dst", [((14, 14), (224, 224)), ((224, 224), (14, 14)), ((5, 9), (11, 3)), ((1, 1), (7, 4))])
def test_constant_image_stays_constant(src, dst):
    for v in (0, 1, 127, 254, 255):
        assert np.all(resize_linear(np.full(src, v, np.uint8), dst) == v)


def test_edge_clamps():
    img = np.random.RandomState(2).randint(0, 256, size=(14, 14)).astype(np.uint8)
    out = resize_linear(img, (224, 224))
    # the first 8 output columns sit left of source column 0's centre: clamped to column 0 (and likewise for rows, where
    # both clamped source rows are row 0, so b0 + b1 = 2048 weights the same value)
    assert np.array_equal(out[:8, :8], np.broadcast_to(img[0, 0], (8, 8)))
    assert np.array_equal(out[-8:, -8:], np.broadcast_to(img[-1, -1], (8, 8)))
    # a single source pixel fills the whole output
    assert np.all(resize_linear(np.array([[77]], np.uint8), (5, 9)) == 77)


def test_vertical_pass_rounding():
    # one step of the vertical pass by hand: S = 2048 v for a constant row, so dst = ((b0 (128 v) >> 16) + ... + 2) >> 2
    img = np.array([[10, 10], [11, 11]], np.uint8)
    out = resize_linear(img, (3, 2))
    _, ya = H.linear_table(2, 3, "y")
    yo, _ = H.linear_table(2, 3, "y")
    for d in range(3):
        r0, r1 = min(max(yo[d], 0), 1), min(max(yo[d] + 1, 0), 1)
        S0, S1 = int(img[r0, 0]) * 2048, int(img[r1, 0]) * 2048
        want = (((int(ya[2 * d]) * (S0 >> 4)) >> 16) + ((int(ya[2 * d + 1]) * (S1 >> 4)) >> 16) + 2) >> 2
        assert out[d, 0] == want


def test_blend_ties_round_half_to_even():
    # h = 5, i = 0: 5 * 0.3 = 1.5 exactly in float64 -> 2; h = 0, i = 1: 0.5 -> 0; h = 0, i = 3: 1.5 -> 2; i = 5: 2.5 -> 2
    assert blend([5], [0])[0] == 2
    assert blend([0, 0, 0], [1, 3, 5]).tolist() == [0, 2, 2]
    assert 5 * 0.3 == 1.5
    h, i = np.meshgrid(np.arange(256), np.arange(256))
    v = h * 0.3 + i * 0.5
    assert np.array_equal(blend(h, i), np.rint(v).astype(np.uint8))
    assert blend([255], [255])[0] == 204


@pytest.mark.parametrize("idx", range(14))
def test_window_rule_every_clipped_index(idx):
    # the reference: fmax clipped to [2, 11] as integers, rows int(f - 2.5) : f + 3
    y0, y1, x0, x1 = crop_window(idx * 14 + (13 - idx), 14, 14, 5)
    for lo, hi, v in ((y0, y1, idx), (x0, x1, 13 - idx)):
        f = min(max(v, 2), 11)
        assert (lo, hi) == (int(f - 2.5), f + 3)
        assert hi - lo == (5 if f == 2 else 6)
        assert 0 <= lo < hi <= 14


def test_cell_argmax_first_of_ties():
    g = np.zeros((224, 224), np.uint8)
    g[16 * 5, 16 * 7] = 9                   # cell (5, 7)
    g[16 * 2 + 3, 16 * 9 + 1] = 9           # cell (2, 9): same sum, earlier in row-major order
    assert cell_argmax(g) == 2 * 14 + 9


def test_synth_inputs_are_seeded_and_cells_unique():
    a, b = synth_inputs(5, 3), synth_inputs(5, 3)
    for k in ('image', 'flow', 'gt', 'cells'):
        assert np.array_equal(a[k], b[k])
    for k in range(3):
        assert cell_argmax(a['gt'][k, 0]) == a['cells'][k]
        r, c = divmod(int(a['cells'][k]), 14)
        y0, y1, x0, x1 = crop_window(a['cells'][k], 14, 14, 5)
        assert (y1 - y0, x1 - x0) == (6, 6) and 3 <= r <= 11 and 3 <= c <= 11


def test_overlay_restatement_shape_and_lut_use():
    lut = random_lut(3)
    m = np.full((14, 14), 200, np.uint8)
    fr = np.zeros((3, 224, 224), np.uint8)
    out = overlay(m, fr, lut)
    assert out.shape == (224, 224, 3)
    assert np.array_equal(out[0, 0], blend(lut[200], [0, 0, 0]))


def test_jet_table_restated_shape():
    t = H.jet_table_restated()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    # JET runs from dark blue (B high, R low) to dark red
    assert t[0, 0] > 100 and t[0, 2] == 0 and t[255, 2] > 100 and t[255, 0] == 0


# ----------------------------------------------------------------------------- argument checks (no device needed)
def test_linear_table_rejects_bad_sizes():
    with pytest.raises(ValueError):
        H.linear_table(0, 5)
    with pytest.raises(ValueError):
        H.linear_table(5, -1)
    with pytest.raises(ValueError):
        H.linear_table(5, 5, axis="z")


def test_wrappers_reject_host_and_wrong_dtype():
    u8 = torch.zeros((2, 14, 14), dtype=torch.uint8)
    with pytest.raises(ValueError, match="HIP"):
        H.resize_linear_u8(u8, (224, 224))
    with pytest.raises(ValueError, match="uint8"):
        H.resize_linear_u8(u8.float(), (224, 224))
    with pytest.raises(ValueError, match="HIP"):
        H.heatmap_overlay(u8, torch.zeros((2, 3, 224, 224), dtype=torch.uint8), [0, 1],
                          torch.zeros((256, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        H.cell_argmax_u8(torch.zeros((2, 224, 224)))
    with pytest.raises(ValueError, match="tensor"):
        H.cell_argmax_u8(np.zeros((2, 224, 224), np.uint8))


# ----------------------------------------------------------------------------- against cv2 itself, where it exists
@pytest.mark.parametrize("src,dst", [((14, 14), (224, 224)), ((224, 224), (14, 14)), ((720, 1280), (224, 224)),
                                     ((224, 224), (720, 1280)), ((1, 1), (5, 7)), ((13, 29), (31, 11))])
@pytest.mark.parametrize("C", [1, 3])
def test_resize_matches_cv2(src, dst, C):
    cv2 = pytest.importorskip("cv2")
    img = np.random.RandomState(4).randint(0, 256, size=src + ((C,) if C == 3 else ())).astype(np.uint8)
    assert np.array_equal(resize_linear(img, dst), cv2.resize(img, (dst[1], dst[0])))


def test_jet_table_matches_cv2():
    cv2 = pytest.importorskip("cv2")
    ref = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET).reshape(256, 3)
    assert np.array_equal(H.jet_table_restated(), ref)


def test_overlay_matches_cv2():
    cv2 = pytest.importorskip("cv2")
    rs = np.random.RandomState(6)
    m = rs.randint(0, 256, size=(14, 14)).astype(np.uint8)
    fr = rs.randint(0, 256, size=(3, 224, 224)).astype(np.uint8)
    lut = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET).reshape(256, 3)
    res = cv2.applyColorMap(cv2.resize(m, (224, 224)), cv2.COLORMAP_JET) * 0.3 + fr.transpose(1, 2, 0) * 0.5
    # what cv2.imwrite stores for the float64 image: its own conversion to 8 bits, through a lossless encoder
    want = cv2.imdecode(cv2.imencode(".png", res)[1], cv2.IMREAD_COLOR)
    assert np.array_equal(overlay(m, fr, lut), want)
