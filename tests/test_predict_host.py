"""Host logic of egaze_amd.predict: which frames get a prediction, the chunk plan and its plane table, the fixation flags
(file and online rule), the coordinate mapping and the parser.  No GPU needed: nothing is launched."""
import numpy as np
import pytest


def P():
    from egaze_amd import predict
    return predict


# ----------------------------------------------------------------------------- frames, chunks, plane table
@pytest.mark.parametrize("F", [10, 11, 14, 40])
def test_predictable_range(F):
    p = P()
    if F < 11:
        with pytest.raises(ValueError, match="at least 11 frames"):
            p.predictable_frames(F)
        with pytest.raises(ValueError):
            p.chunk_plan(F, 4)
        return
    r = p.predictable_frames(F)
    assert list(r) == [k for k in range(F) if 9 <= k <= F - 2] and len(r) == F - 10


def test_plane_table_written_out_for_eleven_frames():
    p = P()
    plan = p.chunk_plan(11, 32)
    assert plan == [{'frames': (9, 10), 'decode': (0, 11), 'flows': (0, 10), 'carried': (0, 0)}]
    # pool: planes 0 .. 2 = B, G, R of frame 9; then flow 0 x, flow 0 y, flow 1 x, ... flow 9 y at 3 .. 22
    by_hand = [[0,
                21, 22,      # m = 0: flow 9
                19, 20,      # m = 1: flow 8
                17, 18, 15, 16, 13, 14, 11, 12, 9, 10, 7, 8, 5, 6,
                3, 4,        # m = 9: flow 0
                -1]]
    t = p.plane_table(1)
    assert t.dtype == np.int64 and t.tolist() == by_hand


@pytest.mark.parametrize("F, chunk", [(11, 1), (14, 3), (14, 32), (40, 7), (40, 30), (40, 1)])
def test_chunks_carry_nine_flows_and_request_nothing_twice(F, chunk):
    p = P()
    plan = p.chunk_plan(F, chunk)
    frames = [k for c in plan for k in range(*c['frames'])]
    assert frames == list(range(9, F - 1))
    assert all(0 < c['frames'][1] - c['frames'][0] <= chunk for c in plan)
    flows = [i for c in plan for i in range(*c['flows'])]
    decoded = [i for c in plan for i in range(*c['decode'])]
    assert flows == list(range(F - 1))                       # each flow once, in order, none missing
    assert decoded == list(range(F))                         # each frame decoded once
    have = set()
    for n, c in enumerate(plan):
        k0, k1 = c['frames']
        carried = set(range(*c['carried']))
        assert carried <= have                               # only what an earlier chunk computed is carried
        assert len(carried) == (0 if n == 0 else 9)
        if n:
            assert c['carried'] == (k0 - 9, k0) and plan[n - 1]['flows'][1] == k0
            assert c['decode'][0] == k0 + 1                  # frame k0 itself comes over from the chunk before
        pool = sorted(carried | set(range(*c['flows'])))
        assert pool == list(range(k0 - 9, k1))               # the chunk's pool: flows k0 - 9 .. k1 - 1
        have |= set(range(*c['flows']))
        # the table addresses, for frame k and m = 0 .. 9, flow k - m of that pool
        t = p.plane_table(k1 - k0)
        base = 3 * (k1 - k0)
        for i in range(k1 - k0):
            assert t[i, 0] == 3 * i and t[i, 21] == -1
            for m in range(10):
                j = (k0 + i - m) - (k0 - 9)                  # position of flow k - m in the pool
                assert (t[i, 1 + 2 * m], t[i, 2 + 2 * m]) == (base + 2 * j, base + 2 * j + 1)
        assert t[:, :21].min() >= 0 and t[:, :21].max() == base + 2 * (k1 - k0 + 9) - 1


# ----------------------------------------------------------------------------- fixation flags
def test_file_flags_are_dilated_like_stdataset(tmp_path):
    p = P()
    rng = np.random.RandomState(3)
    for n in (1, 2, 11, 57):
        for _ in range(5):
            a = (rng.rand(n) < 0.3).astype(float)
            want = (np.convolve(a, np.array([1, 1, 1]))[1:-1] > 0).astype(float)        # STDataset.__init__
            assert np.array_equal(p.dilate_fixsac(a), want)
            path = tmp_path / "f.txt"
            np.savetxt(path, a)
            assert np.array_equal(p.load_fixsac(str(path), n), want)
    a = np.zeros(14)
    a[[8, 13]] = 1                                                                     # -> frames 9 .. 12: 1, 0, 0, 1
    assert p.dilate_fixsac(a)[9:13].tolist() == [1.0, 0.0, 0.0, 1.0]


def test_short_flag_file_is_refused(tmp_path):
    p = P()
    path = tmp_path / "f.txt"
    np.savetxt(path, np.ones(13))
    with pytest.raises(ValueError, match="13 fixation flags for 14 frames"):
        p.load_fixsac(str(path), 14)
    assert p.load_fixsac(str(path), 13).shape == (13,)
    np.savetxt(path, np.ones(20))                            # longer: the first F lines count
    assert p.load_fixsac(str(path), 14).shape == (14,)


def _rule_restated(xs, ys, r2):
    """misc/gazedataset_gt.py's loop without the retroactive clearing, written out."""
    flags = [0]
    cx, cy, fix_num = xs[0], ys[0], 0
    for i in range(1, len(xs)):
        if (cx - xs[i]) ** 2 + (cy - ys[i]) ** 2 < r2:
            flags.append(1)
            fix_num += 1
            cx, cy = cx * fix_num, cy * fix_num
            cx, cy = cx + xs[i], cy + ys[i]
            cx, cy = cx / (fix_num + 1), cy / (fix_num + 1)
        else:
            flags.append(0)
            fix_num = 0
            cx, cy = xs[i], ys[i]
    return flags


TRACKS = {
    "stationary": ([100.0] * 6, [50.0] * 6, [0, 1, 1, 1, 1, 1]),
    "jump": ([100.0, 101.0, 102.0, 180.0, 181.0, 181.5], [50.0, 50.5, 50.0, 120.0, 120.0, 121.0], [0, 1, 1, 0, 1, 1]),
    # one frame near the start point, then away: the reference would clear that one-frame fixation afterwards; online it stays
    "one-frame dwell": ([10.0, 11.0, 100.0, 200.0], [10.0, 10.0, 100.0, 200.0], [0, 1, 0, 0]),
    # 17.5 away exactly: the comparison is strict, so it is a saccade; a hair inside is a fixation
    "on the radius": ([0.0, 17.5, 17.5, 17.5 + 17.4999], [0.0, 0.0, 17.5, 17.5], [0, 0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(TRACKS))
def test_online_rule_equals_the_restated_rule(name):
    p = P()
    xs, ys, want = TRACKS[name]
    rule = p.OnlineFixation(17.5)
    got = [rule.step(x, y) for x, y in zip(xs, ys)]
    assert got == _rule_restated(xs, ys, 17.5 ** 2) == want
    from egaze_amd.misc.gazedataset_gt import fixation_state
    ref = fixation_state(np.array(xs) * 50 / 17.5, np.array(ys) * 50 / 17.5).astype(int).tolist()   # the rule at its own 50 px
    if name == "one-frame dwell":
        assert ref == [0, 0, 0, 0]                           # the retroactive clearing, left out online
    elif name != "on the radius":                            # (scaling moves a point that sits exactly on the radius)
        assert ref == want


def test_online_rule_treats_nan_as_a_saccade():
    rule = P().OnlineFixation(17.5)
    assert [rule.step(*pt) for pt in [(5.0, 5.0), (5.0, 6.0), (float("nan"), float("nan")), (5.0, 5.0), (5.0, 5.5)]] == \
        [0, 1, 0, 0, 1]


# ----------------------------------------------------------------------------- coordinates
@pytest.mark.parametrize("H0, W0", [(224, 224), (720, 1280), (96, 128)])
def test_coordinate_mapping(H0, W0):
    p = P()
    x, y = p.map_to_frame(111.5, 111.5, (H0, W0))            # the map's centre
    assert (x, y) == ((W0 - 1) / 2, (H0 - 1) / 2)
    x, y = p.map_to_frame(0.0, 0.0, (H0, W0))
    assert (x, y) == (W0 / 448 - 0.5, H0 / 448 - 0.5)
    x, y = p.map_to_frame(223.0, 223.0, (H0, W0))            # the last pixel's centre: as far from the far edge
    assert x == pytest.approx(W0 - 1 - (W0 / 448 - 0.5)) and y == pytest.approx(H0 - 1 - (H0 / 448 - 0.5))
    if (H0, W0) == (224, 224):
        assert p.map_to_frame(37.25, 180.5, (H0, W0)) == (180.5, 37.25)
    r_in, r_out = p.ring_radii(H0)
    assert (r_in, r_out) == {224: (6, 9), 720: (19, 29), 96: (3, 4)}[H0]


# ----------------------------------------------------------------------------- parser
BASE = ["--framePath", "v", "--trained_model", "sp", "--trained_late", "lf", "--out", "o"]


@pytest.mark.parametrize("extra", [["--chunk", "0"], ["--flow_jpeg", "101"], ["--flow_jpeg", "-1"], ["--handover_jpeg", "101"],
                                   ["--fix_radius", "-1"], ["--fixsac", "auto"], ["--fixsac", "flags.txt"]])
def test_parser_refuses(extra, capsys):
    with pytest.raises(SystemExit) as e:
        P().parse_args(BASE + extra)
    assert e.value.code == 2
    assert extra[0] in capsys.readouterr().err


def test_parser_defaults_and_accepts():
    p = P()
    a = p.parse_args(BASE)
    assert (a.fixsac, a.fix_radius, a.chunk, a.crop_size, a.flow_jpeg, a.handover_jpeg) == ('all', 17.5, 32, 3, 95, 0)
    assert not a.overlay and not a.save_maps and a.device == '0' and a.bound == 20.0 and a.trained_lstm is None
    assert a.params == dict(tau=0.25, lam=0.15, theta=0.3, nscales=5, zfactor=0.5, warps=5, iterations=30)
    a = p.parse_args(BASE + ["--fixsac", "auto", "--trained_lstm", "l", "--flow_jpeg", "0", "--fix_radius", "0", "--overlay"])
    assert a.fixsac == 'auto' and a.flow_jpeg == 0 and a.overlay
    assert p.CSV_HEADER == "frame,row,col,x,y,fixation,sp_row,sp_col"
