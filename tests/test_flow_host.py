"""The definition of the TV-L1 flow (tests/flow_ref.py, the numpy restatement of DESIGN.md "TV-L1 optical flow") tested on its
own, without a GPU: known translations of analytic textures, the pyramid's level sizes (the 16-pixel clamp and the 16-level cap,
in both Python statements and in the library's workspace size), the quantiser, the grey rule, and the file naming and chunking
of data/extract_flow.py with its device calls stubbed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as R  # noqa: E402

# (shift x, shift y), (H, W): the translations of the issue; 3 scales, 5 warps, 30 iterations
TRANSLATIONS = [((1.5, -0.75), (64, 80)), ((3.25, 2.0), (96, 128)), ((-2.5, 0.5), (50, 70))]
MEAN_EPE, MAX_EPE = 0.05, 0.25


def translation_pair(shift, hw):
    return np.stack([R.texture(*hw), R.texture(*hw, shift=shift)])


@pytest.mark.parametrize("shift,hw", TRANSLATIONS)
def test_fp64_definition_recovers_a_translation(shift, hw):
    u1, u2 = R.tvl1_flow(translation_pair(shift, hw), np.float64, nscales=3, warps=5, iterations=30)
    mean, mx = R.endpoint_error(u1, u2, shift, trim=8)
    print(f"{hw} shift {shift}: endpoint error mean {mean:.4f} max {mx:.4f} px")
    assert mean <= MEAN_EPE and mx <= MAX_EPE, (mean, mx)


def test_level_sizes_clamp_to_16_pixels():
    assert R.level_sizes(224, 224, 5, 0.5) == [(224, 224), (112, 112), (56, 56), (28, 28)]        # 14 x 14 would be too small
    assert R.level_sizes(33, 47, 5, 0.5) == [(33, 47), (17, 24)]
    assert R.level_sizes(16, 16, 5, 0.5) == [(16, 16)]
    assert R.level_sizes(256, 512, 3, 0.5) == [(256, 512), (128, 256), (64, 128)]


def test_level_sizes_stop_at_16_levels_in_both_statements():
    """The device carves its workspace for at most 16 levels (MAX_LEVELS of csrc/flow_tvl1.hip): the definition says so too."""
    from egaze_amd import hipops as H
    chain = [100, 90, 81, 73, 66, 59, 53, 48, 43, 39, 35, 32, 29, 26, 23, 21, 19, 17]     # 18 levels keep 16 pixels; 15 follows
    for nscales in (15, 16, 17, 20, 1000):
        want = [(v, v) for v in chain[:min(nscales, 16)]]
        assert R.level_sizes(100, 100, nscales, 0.9) == H.flow_level_sizes(100, 100, nscales, 0.9) == want
    assert R.MAX_LEVELS == H.FLOW_MAX_LEVELS == 16 == len(R.level_sizes(100, 100, 20, 0.9))
    frames = np.zeros((2, 100, 100), np.uint8)
    assert [p.shape[-2:] for p in R.build_pyramid(frames, 20, 0.9, np.float32)] == R.level_sizes(100, 100, 20, 0.9)
    for args in ((224, 224, 5, 0.5), (33, 47, 5, 0.5), (16, 16, 5, 0.5), (256, 512, 3, 0.5), (273, 310, 5, 0.5), (65, 290, 5, 0.5),
                 (64, 80, 10, 0.8), (96, 300, 5, 0.3), (2048, 2048, 20, 0.5)):
        assert R.level_sizes(*args) == H.flow_level_sizes(*args), args
    assert R.level_sizes(273, 310, 5, 0.5) == [(273, 310), (137, 155), (69, 78), (35, 39), (18, 20)]
    assert len(R.level_sizes(64, 80, 10, 0.8)) == 7 and R.level_sizes(96, 300, 5, 0.3) == [(96, 300), (29, 90)]


def test_workspace_size_counts_the_levels_of_the_definition():
    """egz_tvl1_flow_ws_bytes is host code: its pyramid term is F floats per pixel of every level the definition lists, so the
    library's own level_sizes agrees with the two Python ones, the 16-level cap included."""
    from egaze_amd import _lib
    for F, H, W, nscales, z in ((3, 100, 100, 20, 0.9), (3, 100, 100, 16, 0.9), (3, 100, 100, 15, 0.9), (3, 273, 310, 5, 0.5),
                                (2, 65, 290, 5, 0.5), (3, 64, 80, 10, 0.8), (3, 96, 300, 5, 0.3), (35, 16, 272, 5, 0.5),
                                (3, 64, 80, 1, 0.5), (3, 64, 80, 3, 0.5)):
        pyr = sum(h * w for h, w in R.level_sizes(H, W, nscales, z))
        assert _lib.LIB.egz_tvl1_flow_ws_bytes(F, H, W, nscales, z) == 4 * (F * H * W + F * pyr + 18 * (F - 1) * H * W)
    assert _lib.LIB.egz_tvl1_flow_ws_bytes(3, 100, 100, 20, 0.9) == _lib.LIB.egz_tvl1_flow_ws_bytes(3, 100, 100, 16, 0.9)
    assert _lib.LIB.egz_tvl1_flow_ws_bytes(3, 100, 100, 16, 0.9) > _lib.LIB.egz_tvl1_flow_ws_bytes(3, 100, 100, 15, 0.9)


def test_pyramid_filter_radius_follows_zfactor():
    """The radii the wide device tests rely on: 4 at zfactor 0.5, 2 at 0.8, 8 at 0.3; and the wrapper's sigma is the definition's."""
    from egaze_amd import hipops as H
    for z, radius in ((0.5, 4), (0.8, 2), (0.3, 8)):
        assert H.flow_pyramid_sigma(z) == R.pyramid_sigma(z)
        assert R.gauss_weights(R.pyramid_sigma(z))[1] == radius


def test_quantiser_branches_and_ties():
    v = np.array([20.0, 20.000002, 25.0, np.inf, -20.0, -20.000002, -25.0, -np.inf, 0.0], np.float32)
    assert R.flow_to_u8(v, 20.0).tolist() == [255, 255, 255, 255, 0, 0, 0, 0, 128]       # 127.5 -> 128 (even)
    # bound 127.5 makes the mapping v + 127.5: every integer v is a tie, and ties go to the even neighbour
    ints = np.arange(-127, 128).astype(np.float32)
    q = R.flow_to_u8(ints, 127.5)
    want = np.array([int(x + 127.5) + (int(x + 127.5) & 1) for x in ints.tolist()])
    assert (q % 2 == 0).all() and np.array_equal(q, want)
    assert R.flow_to_u8(np.float32(-127.0), 127.5) == 0 and R.flow_to_u8(np.float32(127.0), 127.5) == 254
    # away from ties: the nearest integer
    x = np.linspace(-19.9, 19.9, 1001).astype(np.float32)
    exact = 255.0 * (x.astype(np.float64) + 20.0) / 40.0
    assert np.abs(R.flow_to_u8(x).astype(np.float64) - exact).max() <= 0.5


def test_grey_rule_on_channel_extremes():
    for b in (0, 255):
        for g in (0, 255):
            for r in (0, 255):
                want = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
                assert R.bgr_to_gray(np.array([[[b, g, r]]], np.uint8))[0, 0] == want
    assert R.bgr_to_gray(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255          # the weights sum to 2^14
    assert R.bgr_to_gray(np.array([[[255, 0, 0]], [[0, 255, 0]], [[0, 0, 255]]], np.uint8))[:, 0].tolist() == [29, 150, 76]


class _Stubs:
    """Host stand-ins for extract_flow's three device steps: a frame is its number, a flow plane is its pair's two numbers."""

    def __init__(self, mod, monkeypatch):
        self.decoded = []
        monkeypatch.setattr(mod, "decode_frames", self.decode_frames)
        monkeypatch.setattr(mod, "flow_images", self.flow_images)
        monkeypatch.setattr(mod, "encode_gray", self.encode_gray)

    def decode_frames(self, paths, size, device):
        nums = [int(os.path.basename(p)[4:9]) for p in paths]
        self.decoded.append(nums)
        return np.array(nums)

    def flow_images(self, frames, bound, params):
        pairs = np.stack([frames[:-1], frames[1:]], 1)                      # (F - 1, 2)
        return np.stack([pairs, pairs + 100])[:, :, None, :]               # (2, F - 1, 1, 2): x, then y

    def encode_gray(self, u8, quality):
        return [bytes(int(v) for v in plane.ravel()) for plane in u8]


def _frames_folder(tmp_path, n):
    src = tmp_path / "frames" / "vid"
    src.mkdir(parents=True)
    for i in range(1, n + 1):
        (src / ("img_%05d.jpg" % i)).write_bytes(b"")
    (src / "notes.txt").write_bytes(b"")
    return tmp_path / "frames", tmp_path / "flow"


def test_extract_flow_naming_and_chunk_overlap(tmp_path, monkeypatch):
    from egaze_amd.data import extract_flow as X
    assert X.chunk_ranges(7, 3) == [(0, 3), (3, 6)] and X.chunk_ranges(8, 3) == [(0, 3), (3, 6), (6, 7)]
    assert X.chunk_ranges(2, 32) == [(0, 1)] and X.chunk_ranges(1, 32) == []
    stubs = _Stubs(X, monkeypatch)
    src, dst = _frames_folder(tmp_path, 7)
    argv = ["--framePath", str(src), "--flowPath", str(dst), "--chunk", "3"]
    assert X.main(argv) == 12
    assert stubs.decoded == [[1, 2, 3, 4], [4, 5, 6, 7]]                    # consecutive chunks share one frame
    assert sorted(os.listdir(dst / "vid")) == sorted(f % n for f in X.FLOW_NAMES for n in range(1, 7))   # none for frame 7
    for n in range(1, 7):                                                   # number n: the flow from frame n to frame n + 1
        assert (dst / "vid" / ("flow_x_%05d.jpg" % n)).read_bytes() == bytes([n, n + 1])
        assert (dst / "vid" / ("flow_y_%05d.jpg" % n)).read_bytes() == bytes([n + 100, n + 101])
    # existing files are kept, and a chunk that is complete is not even decoded
    (dst / "vid" / "flow_y_00005.jpg").unlink()
    (dst / "vid" / "flow_x_00004.jpg").write_bytes(b"kept")
    stubs.decoded.clear()
    assert X.main(argv) == 1
    assert stubs.decoded == [[4, 5, 6, 7]]
    assert (dst / "vid" / "flow_x_00004.jpg").read_bytes() == b"kept"
    assert (dst / "vid" / "flow_y_00005.jpg").read_bytes() == bytes([105, 106])
    stubs.decoded.clear()
    assert X.main(argv + ["--overwrite"]) == 12
    assert (dst / "vid" / "flow_x_00004.jpg").read_bytes() == bytes([4, 5])


def test_extract_flow_short_folders_and_arguments(tmp_path, monkeypatch):
    from egaze_amd.data import extract_flow as X
    _Stubs(X, monkeypatch)
    src, dst = _frames_folder(tmp_path, 1)
    assert X.main(["--framePath", str(src), "--flowPath", str(dst)]) == 0          # one frame: no pair, no file
    for bad in (["--chunk", "0"], ["--quality", "0"], ["--bound", "0"], ["--folders", "missing"]):
        with pytest.raises(SystemExit):
            X.main(["--framePath", str(src), "--flowPath", str(dst)] + bad)
