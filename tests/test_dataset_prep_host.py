"""Dataset preparation on the host (egaze_amd.data.dataset_preprocessing, egaze_amd.misc.gazedataset_gt): label files
against what the reference scripts wrote (tests/golden/make_golden_prep.py), impulse indices, OpenCV's INTER_AREA tables,
and a numpy restatement of the whole ground-truth map render -- the construction csrc/gaze_gt.hip evaluates -- against
scipy.ndimage.gaussian_filter plus the reference's normalisation.  The GPU tests (test_hip_gt_maps.py) import the
restatement from here.  cv2 is not installed in the build image: the INTER_AREA restatement is checked against cv2.resize
only where cv2 can be imported."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dataset_prep.npz")

GPLUS = ((960, 1280), 70.0, 0)       # (H, W), sigma, mode: data/dataset_preprocessing.py (GTEA Gaze+)
GAZE = ((480, 640), 35.0, 1)         # misc/gazedataset_gt.py (GTEA Gaze)


def _golden():
    return np.load(GOLDEN)


def _text(a):
    return a.tobytes().decode()


# ----------------------------------------------------------------------------- numpy restatement of the render
def scipy_weights(sigma, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d (order 0): radius int(truncate * sigma + 0.5), phi / phi.sum()."""
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def _reflect(q, n):
    return np.where(q < 0, -q - 1, np.where(q >= n, 2 * n - 1 - q, q))


def line_response(v, c, n, w, R):
    """scipy's correlate1d ('reflect') along the last axis of lines that hold v (one value per line) at index c and 0
    elsewhere, in scipy's order: centre tap, then |k| = R .. 1 adding (in[p - k] + in[p + k]) * w[k].  Only the (at most
    three) taps that hit c are added -- the others add exact zeros."""
    v = np.atleast_1d(np.asarray(v, np.float64))[:, None]     # -> (len(v), n)
    p = np.arange(n)
    out = np.where(p == c, v, 0.0) * w[R]
    for k in range(R, 0, -1):
        a, b = _reflect(p + k, n) == c, _reflect(p - k, n) == c
        hit = a | b
        if hit.any():
            va = np.where(a[hit], v, 0.0)
            vb = np.where(b[hit], v, 0.0)
            out[..., hit] += (va + vb) * w[R + k]
    return out


def render_full(r, c, hw, sigma):
    """-> (M, G): the filtered impulse (== gaussian_filter) and the reference's normalised map G = (M - min) / max * 255,
    built separably: the axis-0 response gy, then per row the axis-1 response of a line holding gy[i] at column c."""
    H, W = hw
    w, R = scipy_weights(sigma)
    gy = line_response(1.0, r, H, w, R)[0]
    M = line_response(gy, c, W, w, R)
    G = M - np.min(M)
    G /= np.max(G)
    G *= 255
    return M, G


def area_resize(S, out_hw, mode):
    """OpenCV's generic INTER_AREA (ResizeArea_Invoker) on one single-channel image, in its accumulation order.
    mode 0: S float64, double accumulation; mode 1: S uint8, float accumulation.  -> (sum as float64, uint8)."""
    from egaze_amd.hipops import area_table
    wt = np.float64 if mode == 0 else np.float32
    H, W = S.shape
    (yo, ys, ya), (xo, xs, xa) = area_table(H, out_hw[0]), area_table(W, out_hw[1])
    S = S.astype(wt)
    buf = np.zeros((H, out_hw[1]), wt)           # buf of every source row at once: per column, x entries in table order
    for dx in range(out_hw[1]):
        for k in range(xo[dx], xo[dx + 1]):
            buf[:, dx] += S[:, xs[k]] * wt(xa[k])
    out = np.zeros(out_hw, wt)
    for dy in range(out_hw[0]):
        for e in range(yo[dy], yo[dy + 1]):
            t = wt(ya[e]) * buf[ys[e]]
            out[dy] = t if e == yo[dy] else out[dy] + t
    u8 = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out.astype(np.float64), u8


def render(r, c, hw, sigma, mode, out_hw=(224, 224)):
    """The reference's gt map at impulse (r, c): mode 0 resizes G, mode 1 resizes np.uint8(G)."""
    _, G = render_full(r, c, hw, sigma)
    return area_resize(G if mode == 0 else G.astype(np.uint8), out_hw, mode)


def positions(hw, sigma):
    """>= 12 impulse positions: the four corners, the -1 wraps, the centre, and rows / columns whose response has two and
    three non-zero taps (a reflection within reach, and the p + c = n - 1 tap hit from both sides)."""
    H, W = hw
    R = int(4.0 * sigma + 0.5)
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, 17), (5, W - 1), (H // 2, W // 2),
            (R // 3, W - R // 2), (H - R // 2, R // 4), ((H - 1) // 2, (W - 1) // 2), (H // 2 - 1, 3), (R - 1, R + 1),
            (1, W - 2)]


# ----------------------------------------------------------------------------- golden label files
def test_parsetxt_matches_reference(tmp_path):
    from egaze_amd.data.dataset_preprocessing import parsetxt
    g = _golden()
    for video in _text(g["gplus_videos"]).split("\n"):
        p = tmp_path / (video + "_gaze.txt")
        p.write_bytes(g[f"gplus_{video}_log"].tobytes())
        gx, gy, nf, fs = parsetxt(str(p))
        assert nf == g[f"gplus_{video}_nframe"].tolist()
        assert fs == g[f"gplus_{video}_fixsac_list"].tolist()
        assert np.array_equal(np.array(gx), g[f"gplus_{video}_gazex"])
        assert np.array_equal(np.array(gy), g[f"gplus_{video}_gazey"])


def test_fixsac_files_match_reference_bytes(tmp_path):
    from egaze_amd.data import dataset_preprocessing as D
    g = _golden()
    (tmp_path / "gtea_gaze").mkdir()
    videos = _text(g["gplus_videos"]).split("\n")
    for video in videos:
        (tmp_path / "gtea_gaze" / (video + "_gaze.txt")).write_bytes(g[f"gplus_{video}_log"].tobytes())
    D.main(["--gazePath", str(tmp_path / "gtea_gaze"), "--fixsacPath", str(tmp_path / "fixsac"), "--fixsac-only"])
    for video in videos:
        assert (tmp_path / "fixsac" / (video + ".txt")).read_bytes() == g[f"gplus_{video}_fixsac"].tobytes()


def test_fixation_files_match_reference_bytes(tmp_path):
    from egaze_amd.misc import gazedataset_gt as M
    g = _golden()
    (tmp_path / "gp").mkdir()
    names = _text(g["gaze_names"]).split("\n")
    for name in names:
        (tmp_path / "gp" / (name + ".txt")).write_bytes(g[f"gaze_{name}_track"].tobytes())
    M.main(["--gazePath", str(tmp_path / "gp"), "--fixationPath", str(tmp_path / "fix")])
    for name in names:
        assert (tmp_path / "fix" / (name + "_fixation.txt")).read_bytes() == g[f"gaze_{name}_fixation"].tobytes()
    assert not (tmp_path / names[0]).exists()                # no maps without --gt


def test_parsetxt_frame_before_first_raises(tmp_path):
    from egaze_amd.data.dataset_preprocessing import parsetxt
    p = tmp_path / "v_gaze.txt"
    p.write_text("0\tSMP\t1\t10.0\t10.0\t5\tFixation\n0\tSMP\t1\t12.0\t10.0\t6\tFixation\n"
                 "0\tSMP\t1\t12.0\t10.0\t4\tFixation\n")
    with pytest.raises(ValueError, match="precedes the first frame"):
        parsetxt(str(p))


def test_missing_frames_stop_with_video_name(tmp_path):
    from egaze_amd.data import dataset_preprocessing as D
    (tmp_path / "gaze").mkdir(); (tmp_path / "flow" / "Vid_One").mkdir(parents=True)
    (tmp_path / "gaze" / "Vid_One_gaze.txt").write_text("".join(f"0\tSMP\t1\t10.0\t10.0\t{n}\tFixation\n" for n in range(4)))
    for n in range(1, 3):
        (tmp_path / "flow" / "Vid_One" / f"img_{n:05d}.jpg").write_bytes(b"")
    with pytest.raises(SystemExit, match="Vid_One"):
        D.main(["--gazePath", str(tmp_path / "gaze"), "--flowPath", str(tmp_path / "flow"), "--imagePath",
                str(tmp_path / "img"), "--gtPath", str(tmp_path / "gt"), "--fixsacPath", str(tmp_path / "fs")])


# ----------------------------------------------------------------------------- impulse indices and area tables
def test_impulse_index_mapping():
    from egaze_amd.data.dataset_preprocessing import impulse_index
    from egaze_amd.misc.gazedataset_gt import impulse_indices
    # the reference's gazemap[int(round(y)) - 1][int(round(x)) - 1] on a numpy array
    for v, size in ((0.5, 960), (-0.5, 960), (0.0, 960), (1.5, 960), (2.5, 1280), (959.4, 960), (1279.4, 1280),
                    (640.5, 1280), (1.0, 1280)):
        ref = np.zeros(size); ref[int(round(v)) - 1] = 1
        assert impulse_index(v, size) == int(np.argmax(ref)), v
    assert impulse_index(0.5, 960) == 959 and impulse_index(0.5, 1280) == 1279 and impulse_index(2.5, 960) == 1
    with pytest.raises(ValueError):
        impulse_index(962.0, 960)
    x = np.array([0.0, 0.5, 1.5, 2.5, 640.0, 639.5, 320.5])
    y = np.array([480.0, 479.5, 0.5, 1.5, 0.0, 2.5, 240.5])
    rows, cols = impulse_indices(x, y)
    assert rows.tolist() == [479, 479, 479, 1, 479, 1, 239]
    assert cols.tolist() == [639, 639, 1, 1, 639, 639, 319]


@pytest.mark.parametrize("ssize,dsize", [(1280, 224), (960, 224), (640, 224), (480, 224), (100, 7), (37, 36)])
def test_area_tables(ssize, dsize):
    from egaze_amd.hipops import area_table
    ofs, si, alpha = area_table(ssize, dsize)
    assert ofs.dtype == np.int32 and si.dtype == np.int32 and alpha.dtype == np.float32
    assert ofs[0] == 0 and ofs[-1] == len(si) == len(alpha) and len(ofs) == dsize + 1
    assert np.all(np.diff(ofs) >= 1) and si.min() >= 0 and si.max() == ssize - 1
    sums = np.add.reduceat(alpha.astype(np.float64), ofs[:-1])
    assert np.abs(sums - 1.0).max() < 1e-6
    scale = ssize / dsize
    assert np.diff(ofs).max() <= int(np.ceil(scale)) + 1
    assert np.all(np.diff(si) >= -1)                      # consecutive outputs share at most one boundary column
    # every source index is covered, in order within each output
    assert set(si.tolist()) == set(range(ssize))
    for d in range(dsize):
        seg = si[ofs[d]:ofs[d + 1]]
        assert np.all(np.diff(seg) == 1)
        assert abs(seg[0] - d * scale) <= 1 and abs(seg[-1] + 1 - (d + 1) * scale) <= 1
    # one entry per source column, plus one per interior cell boundary that falls inside a source column
    assert len(si) == ssize + sum(1 for d in range(1, dsize) if (d * ssize) % dsize)
    if ssize == 1280:
        assert len(si) == 1472 and np.diff(ofs).max() == 7


# ----------------------------------------------------------------------------- the restatement against scipy
@pytest.mark.parametrize("geom", [GPLUS, GAZE], ids=["gplus", "gaze"])
def test_render_restatement_matches_scipy(geom):
    from scipy import ndimage
    hw, sigma, _ = geom
    for r, c in positions(hw, sigma)[:8]:
        M, G = render_full(r, c, hw, sigma)
        imp = np.zeros(hw); imp[r, c] = 1
        ref = ndimage.gaussian_filter(imp, sigma)
        assert np.array_equal(M, ref), (r, c)
        ref -= np.min(ref); ref /= np.max(ref); ref *= 255
        assert np.array_equal(G, ref), (r, c)


def test_area_restatement_basic():
    # a constant image stays constant (up to the float32 rounding of the table weights)
    out, u8 = area_resize(np.full((960, 1280), 200.0), (224, 224), 0)
    assert np.abs(out - 200.0).max() < 1e-3 and np.all(u8 == 200)
    out, u8 = area_resize(np.full((480, 640), 77, np.uint8), (224, 224), 1)
    assert out.dtype == np.float64 and np.abs(out - 77.0).max() < 1e-3 and np.all(u8 == 77)


def test_restatement_matches_cv2_resize():
    cv2 = pytest.importorskip("cv2")
    for hw, sigma, mode in (GPLUS, GAZE):
        for r, c in positions(hw, sigma)[:4]:
            _, G = render_full(r, c, hw, sigma)
            S = G if mode == 0 else G.astype(np.uint8)
            ref = cv2.resize(S, (224, 224), interpolation=cv2.INTER_AREA)
            out, u8 = area_resize(S, (224, 224), mode)
            if mode == 0:
                assert np.array_equal(out, ref)
            else:
                assert np.array_equal(u8, ref)
