"""Host side of the affine resident gather (tests/augment_affine_ref.py, hipops.AugSpec's scale / rotate,
egz_resident_gather_affine's argument checks).  No GPU: nothing is launched."""
import numpy as np
import pytest

import augment_affine_ref as R
import augment_ref as A

F = np.float32
SETTING = dict(flip_thr=1 << 31, shift=16, contrast=0.2, brightness=0.1)
RR10 = R.rotate_rad(10)


# ----------------------------------------------------------------------------- the draw and the matrices
# computed once on a CPU with the definition of DESIGN.md section 21 (seed 1, scale 0.15, rotate 10 degrees); pinned so that
# restatement and kernel cannot drift together
KNOWN = [
    # epoch, sample, bits(g), bits(theta), M00, M01, A00, A10, word[5]
    (0, 0, 0x3f8f3a4f, 0x3d9b67d2, 58400, 4440, 73122, 5559, 0xe584b6528d0bb3f8),
    (0, 1, 0x3f5fb78d, 0xbdd4d9b6, 74588, -7780, 56963, -5942, 0x1463d7a3d38e838e),
    (0, 6, 0x3f7c35d8, 0x3df2ba26, 66054, 7866, 64113, 7634, 0x735e27d8822f9f17),
    (0, (1 << 33) + 5, 0x3f8d19be, 0x3deaab42, 59061, 6797, 71770, 8260, 0xd756484f86480f80),
    (3, 1, 0x3f5d41b8, 0xbdeffe83, 75307, -8865, 56253, -6622, 0x0c3066b0bbfea1c5),
]


def _bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("epoch,sample,g,theta,M00,M01,A00,A10,word5", KNOWN)
def test_known_answers(epoch, sample, g, theta, M00, M01, A00, A10, word5):
    assert _bits(RR10) == 0x3e32b8c2
    got = R.draw(1, epoch, sample, **SETTING, scale=0.15, rot_rad=RR10)
    assert got[5].dtype == np.float32 and got[6].dtype == np.float32
    assert (_bits(got[5]), _bits(got[6])) == (g, theta)
    assert R.matrices(got[5], got[6]) == (M00, M01, A00, A10)
    assert R.words(1, epoch, sample)[5] == word5


def test_the_five_old_parameters_do_not_move():
    for epoch, sample in ((0, 0), (0, 6), (3, 1), (7, (1 << 33) + 5), (2, 123456)):
        assert R.words(1, epoch, sample)[:5] == A.words(1, epoch, sample)
        old = A.draw(1, epoch, sample, **SETTING)
        for scale, rot in ((0.0, 0.0), (0.15, RR10), (0.5, R.QUARTER_PI)):
            new = R.draw(1, epoch, sample, **SETTING, scale=scale, rot_rad=rot)
            assert new[:5] == old
    # zero amplitudes: g = 1 exactly, theta = +-0, the identity matrices
    for s in range(200):
        d = R.draw(9, 2, s, 0, 0, 0.0, 0.0, 0.0, F(0.0))
        assert d[5] == F(1.0) and d[6] == F(0.0) and R.matrices(d[5], d[6]) == (65536, 0, 65536, 0)
    gs = np.array([R.draw(9, 2, s, 0, 0, 0.0, 0.0, 0.5, R.QUARTER_PI)[5:] for s in range(400)])
    assert 0.5 <= gs[:, 0].min() < 0.55 and 1.45 < gs[:, 0].max() < 1.5
    assert -R.QUARTER_PI <= gs[:, 1].min() < -0.7 and 0.7 < gs[:, 1].max() < R.QUARTER_PI


def test_rows_round_trip():
    params = [R.draw(1, 0, s, **SETTING, scale=0.15, rot_rad=RR10) for s in range(5)] + [R.IDENTITY]
    r = R.rows(params)
    assert r.dtype == np.int32 and r.shape == (6, 7) and r[5].tolist() == [0, 0, 0, 0x3f800000, 0, 0x3f800000, 0]
    assert R.unrows(r) == params
    assert np.array_equal(r[:, :5], A.rows([p[:5] for p in params]))


def test_polynomial_against_fp64_sine_and_cosine():
    """2,000,001 points of [-pi/4, pi/4], both ends included.  The largest deviation measured with this restatement was 4.6e-8
    for S and 7.4e-8 for C; the bound is that 7.4e-8 plus one fp32 ulp of 1 (2^-23 = 1.2e-7), the spacing of the results
    themselves near 1, so that the last-place rounding of another libm's fp64 reference cannot fail it."""
    th = np.linspace(-np.pi / 4, np.pi / 4, 2000001).astype(np.float32)
    th[0], th[-1] = -R.QUARTER_PI, R.QUARTER_PI
    s, c = R.sincos(th)
    assert s.dtype == np.float32 and c.dtype == np.float32
    bound = 7.4e-8 + 2.0 ** -23
    t64 = th.astype(np.float64)
    es, ec = np.abs(s - np.sin(t64)).max(), np.abs(c - np.cos(t64)).max()
    print(f"max |S - sin| = {es:.3e}, max |C - cos| = {ec:.3e}")
    assert es <= bound and ec <= bound
    assert R.sincos(F(0.0)) == (F(0.0), F(1.0)) and R.matrices(1.0, 0.0) == (65536, 0, 65536, 0)
    assert R.sincos(F(-0.0)) == (F(0.0), F(1.0)) and R.matrices(1.0, -0.0) == (65536, 0, 65536, 0)


def test_forward_times_inverse_is_the_identity():
    """A M / 65536 against 65536 I over 20,000 seeded (g, theta) and the corners.  Bound per entry, in Q16 units:
    every entry of the product is 65536 (a m + a' m') with a = A / 65536 (|.| <= g) and m = M / 65536 (|.| <= q = 1 / g).
      the two rints move each factor by at most 0.5 / 65536:  0.5 (|m00| + |m01| + |a00| + |a10|) <= 0.5 sqrt(2) (q + g)
                                                             <= 0.5 * 1.41422 * 2.5 = 1.768   (g = 0.5; |C| + |S| <= sqrt 2)
      the fp32 steps (1 / g, q C, g C: three roundings of 2^-24 per product of size <= 1):  65536 * 3 * 2^-24   = 0.012
      the polynomial (C^2 + S^2 - 1 <= 2 sqrt(2) * 7.4e-8 on the diagonal; cancels off it):  65536 * 2.1e-7    = 0.014
      the product of two rint errors:  2 * 65536 * (0.5 / 65536)^2                                             < 0.001
    together 1.80.  The largest figure measured with this restatement was 1.55."""
    rng = np.random.default_rng(7)
    pairs = [(F(rng.uniform(0.5, 1.5)), F(np.clip(F(rng.uniform(-np.pi / 4, np.pi / 4)), -R.QUARTER_PI, R.QUARTER_PI)))
             for _ in range(20000)]
    top = np.nextafter(F(1.5), F(0))
    pairs += [(g, t) for g in (F(0.5), F(1.0), top, F(1.5)) for t in (-R.QUARTER_PI, F(0.0), R.QUARTER_PI)]
    worst = 0.0
    for g, t in pairs:
        M00, M01, A00, A10 = R.matrices(g, t)
        diag = (A00 * M00 + A10 * M01) / 65536 - 65536
        off = (A00 * M01 - A10 * M00) / 65536
        worst = max(worst, abs(diag), abs(off))
    print(f"max |A M / 65536 - 65536 I| = {worst:.3f}")
    assert worst <= 1.80


# ----------------------------------------------------------------------------- applying the parameters
def _planes(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (24, H, W), dtype=np.uint8)


@pytest.mark.parametrize("H,W", [(2, 4), (5, 8), (30, 36)])
def test_identity_is_the_integer_gather(H, W):
    """g = 1, theta = 0: both flips; shifts inside, at and beyond the frame, in each direction."""
    p = _planes(H, W, seed=H)
    shifts = lambda n: (0, 1, -1, 2, n - 1, -(n - 1), n, -n, n + 3, -(n + 3))
    for flip in (0, 1):
        for dy in shifts(H):
            for dx in shifts(W):
                assert np.array_equal(R.geometric(p, flip, dy, dx, F(1.0), F(0.0)), A.geometric(p, flip, dy, dx)), (flip, dy, dx)
    assert np.array_equal(R.geometric(p, 1, 2, -1, F(1.0), F(-0.0)), A.geometric(p, 1, 2, -1))


@pytest.mark.parametrize("flip", [0, 1])
def test_a_constant_flow_field_turns_and_scales_with_the_picture(flip):
    """Every flow pair holds one vector; the output holds g R(theta) of it (x negated first under a flip), within 1 byte.  The
    vectors are short enough not to clip at g = 1.5."""
    H, W = 6, 8
    rng = np.random.default_rng(3)
    p = _planes(H, W, seed=1)
    vec = rng.integers(70, 186, (10, 2))
    for k in range(10):
        p[3 + 2 * k], p[4 + 2 * k] = vec[k, 0], vec[k, 1]
    top = np.nextafter(F(1.5), F(0))
    for g, t in ((F(1.0), F(0.3)), (F(0.5), R.QUARTER_PI), (top, -R.QUARTER_PI), (F(1.25), F(-0.1)), (F(0.8), F(0.0))):
        out = R.geometric(p, flip, 1, -2, g, t).astype(np.float64)
        vx, vy = (vec[:, 0] - 127.5) * (-1 if flip else 1), vec[:, 1] - 127.5
        wx = 127.5 + float(g) * (np.cos(float(t)) * vx - np.sin(float(t)) * vy)
        wy = 127.5 + float(g) * (np.sin(float(t)) * vx + np.cos(float(t)) * vy)
        assert wx.min() > 0 and wx.max() < 255 and wy.min() > 0 and wy.max() < 255
        for k in range(10):
            assert np.abs(out[3 + 2 * k] - wx[k]).max() <= 1.0 and np.abs(out[4 + 2 * k] - wy[k]).max() <= 1.0, (g, t, k)


@pytest.mark.parametrize("flip", [0, 1])
def test_a_linear_ramp_comes_out_at_the_analytic_coordinate(flip):
    """byte = 10 + 3 x + 2 y in the (flipped) frame; an output pixel whose source lies inside the frame holds the ramp at
    c + (1 / g) R(-theta) (p - d - c).  Bilinear interpolation is exact on a ramp, so the deviation is the byte's own rounding
    (0.5) plus the slopes (3 + 2) times the coordinate error: 1 / 512 pixel from the Q8 rounding of the coordinate and
    (0.5 + 0.01) (|X2| + |Y2|) / 131072 <= 0.51 (H + W) / 131072 from the rint and the fp32 steps of the Q16 matrix."""
    H, W = 30, 36
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = (10 + 3 * xx + 2 * yy).astype(np.uint8)
    assert 10 + 3 * (W - 1) + 2 * (H - 1) <= 255
    p = np.zeros((24, H, W), dtype=np.uint8)
    p[:] = ramp[:, ::-1] if flip else ramp               # stored so that the flipped frame F is the ramp
    p[A.FLOW_X, :, :] = 255 - p[A.FLOW_X, :, :] if flip else p[A.FLOW_X, :, :]
    bound = 0.5 + 5 * (1 / 512 + 0.51 * (H + W) / 131072)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    for g, t, dy, dx in ((F(1.0), F(0.3), 0, 0), (F(0.5), R.QUARTER_PI, 2, -3), (F(1.4), F(-0.5), -1, 4), (F(0.75), F(0.0), 3, 1)):
        out = R.geometric(p, flip, dy, dx, g, t).astype(np.float64)
        q, c, s = 1 / float(g), np.cos(float(t)), np.sin(float(t))
        ux, uy = xx - dx - cx, yy - dy - cy
        sx, sy = cx + q * (c * ux + s * uy), cy + q * (-s * ux + c * uy)
        inside = (sx >= 0.01) & (sx <= W - 1.01) & (sy >= 0.01) & (sy <= H - 1.01)
        assert inside.sum() > 100
        want = 10 + 3 * sx + 2 * sy
        for plane in (0, 2, 23):                          # colour and ground truth: the same mix, nothing clamped inside
            assert np.abs(out[plane] - want)[inside].max() <= bound, (g, t, plane)
        assert (out[23][(sx < -1.01) | (sx > W + 0.01) | (sy < -1.01) | (sy > H + 0.01)] == 0).all()


def test_the_ground_truth_fades_at_the_frame_and_colour_replicates():
    H, W = 5, 8
    p = np.full((24, H, W), 200, dtype=np.uint8)
    out = R.geometric(p, 0, 0, 0, F(0.5), F(0.0))         # q = 2: the frame shrinks to the middle half
    assert (out[:3] == 200).all() and (out[3:23:2] == 164).all()      # 127.5 + 0.5 (200 - 127.5) = 163.75
    assert out[23, 0, 0] == 0 and out[23].max() == 200 and (out[23, 1:4, 2:6] == 200).all()
    out = R.geometric(p, 0, 0, 0, F(0.75), F(0.3))        # a turned edge: taps on both sides of it, weights in between
    assert (out[:3] == 200).all() and ((out[23] > 0) & (out[23] < 200)).any() and out[23, 0, 0] == 0 and out[23, 2, 4] == 200


# ----------------------------------------------------------------------------- AugSpec
def test_augspec_scale_and_rotate():
    from egaze_amd.hipops import AugSpec
    s = AugSpec.parse("flip=0.5,shift=16,contrast=0.2,brightness=0.1,scale=0.15,rotate=10")
    assert s == AugSpec(0.5, 16, 0.2, 0.1, 0, 0.15, 10.0) == AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, scale=0.15,
                                                                      rotate=10)
    assert str(s).endswith("seed=0,scale=0.15,rotate=10.0") and AugSpec.parse(str(s)) == s and s.affine
    assert _bits(s.rotate_rad) == _bits(RR10) and float(F(s.rotate_rad)) == s.rotate_rad
    assert _bits(AugSpec(rotate=45).rotate_rad) == _bits(R.QUARTER_PI)
    # a spec without the two prints and compares as it always did
    old = AugSpec(0.5, 16, 0.2, 0.1, 3)
    assert str(old) == "flip=0.5,shift=16,contrast=0.2,brightness=0.1,seed=3" and not old.affine
    assert old.scale == 0.0 and old.rotate == 0.0 and old.rotate_rad == 0.0
    for text in ("scale=0.5", "rotate=45", "rotate=7", "scale=0.25,seed=9", "flip,rotate=0.5,scale=0.001"):
        t = AugSpec.parse(text)
        assert AugSpec.parse(str(t)) == t and t.affine and hash(t) == hash(AugSpec.parse(str(t)))
    assert "scale" not in str(AugSpec.parse("rotate=7")) and "rotate" not in str(AugSpec.parse("scale=0.1"))
    assert AugSpec.parse("scale=0.25,seed=9", seed=2) == AugSpec(seed=2, scale=0.25)
    assert isinstance(AugSpec(rotate=10).rotate, float) and isinstance(AugSpec(scale=0).scale, float)


@pytest.mark.parametrize("text", ["scale=0.51", "scale=-0.1", "scale", "scale=x", "scale=nan", "rotate=45.5", "rotate=-1", "rotate",
                                  "rotate=nan", "rotate=inf", "scale=0.1,scale=0.2", "zoom=2", "rotate=10deg"])
def test_augspec_refusals(text):
    from egaze_amd.hipops import AugSpec
    with pytest.raises(ValueError, match="AugSpec"):
        AugSpec.parse(text)


def test_augspec_constructor_refusals():
    from egaze_amd.hipops import AugSpec
    for kw in (dict(scale=0.6), dict(scale=-0.01), dict(scale="0.1"), dict(scale=True), dict(scale=float("nan")),
               dict(rotate=46), dict(rotate=-0.5), dict(rotate="10"), dict(rotate=float("nan"))):
        with pytest.raises(ValueError, match="AugSpec"):
            AugSpec(**kw)


def test_cli_takes_the_two_keys_and_says_so():
    from egaze_amd import gaze_full, streamtrain
    from egaze_amd.hipops import AugSpec
    for parser in (gaze_full.build_parser(), streamtrain.build_parser("spatial"), streamtrain.build_parser("temporal")):
        ns = parser.parse_args(["--gpu_resident", "--augment", "flip,scale=0.2,rotate=10", "--augment_seed", "5"])
        assert streamtrain.augment_spec(ns) == AugSpec(flip=0.5, seed=5, scale=0.2, rotate=10.0)
        text = "".join(parser.format_help().split())     # argparse breaks the long example where it pleases
        assert "scale=0.15,rotate=10" in text


# ----------------------------------------------------------------------------- status words
def test_status_words_name_bit_3():
    from egaze_amd import hipops as Hp
    assert set(Hp.AFFINE_STATUS) == set(range(8, 16)) and not set(Hp.AFFINE_STATUS) & set(Hp.RESIDENT_STATUS)
    for st in range(8, 16):
        assert "magnification" in Hp.AFFINE_STATUS[st]
        if st > 8:
            assert Hp.RESIDENT_STATUS[st - 8] in Hp.AFFINE_STATUS[st]
    import torch

    class _Done:
        def synchronize(self):
            pass
    for st in (4, 8, 13):
        with pytest.raises(RuntimeError, match="resident_gather: .*skipped") as e:
            Hp.check_resident_status((torch.tensor([st], dtype=torch.int32), _Done()))
        assert (Hp.RESIDENT_STATUS.get(st) or Hp.AFFINE_STATUS[st]) in str(e.value)


# ----------------------------------------------------------------------------- C-ABI refusals (nothing is launched)
def _call(**over):
    from egaze_amd import _lib
    a = dict(pool=0x1000, P=60, table=0x2000, N=7, idx=0x3000, B=3, H=224, W=224, mean=0x4000, std=0x5000, image=0x10000,
             flow=0x20000, gt=0x30000, nhwc=None, absmax=None, raw=None, raw_fields=7, status=0x6000, seed=1, epoch=0,
             flip_thr=1 << 31, max_shift=16, contrast=0.2, brightness=0.1, params_in=None, params_out=None, scale=0.15,
             rotate_rad=float(RR10), stream=None)
    a.update(over)
    rc = _lib.LIB.egz_resident_gather_affine(*a.values())
    return rc, _lib.LIB.egz_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(pool=None), "pool"), (dict(table=None), "table"), (dict(idx=None), "idx"), (dict(mean=None), "mean"),
    (dict(std=None), "mean / std"), (dict(B=0), "B"), (dict(B=65536), "B"), (dict(H=0), "H"), (dict(W=-4), "W"),
    (dict(H=6, W=10), "W = 10 must be a multiple of 4"), (dict(H=4, W=3), "multiple of 4"), (dict(H=2, W=2), "multiple of 4"),
    (dict(H=65536, W=32768), "2^31"), (dict(P=0), "P = 0"), (dict(N=0), "N = 0"),
    (dict(image=None, flow=None, gt=None), "no output"), (dict(nhwc=0x40000), "absmax"), (dict(absmax=0x40000), "absmax"),
    (dict(status=None), "status"), (dict(raw=0x70000, raw_fields=8), "raw_fields"), (dict(raw=0x70000, raw_fields=0), "raw_fields"),
    (dict(pool=0x1002), "4-byte"), (dict(raw=0x70001), "4-byte"), (dict(image=0x10004), "16-byte"), (dict(gt=0x30008), "16-byte"),
    (dict(flip_thr=(1 << 32) + 1), "flip_thr"), (dict(max_shift=-1), "max_shift"), (dict(max_shift=32768), "max_shift"),
    (dict(contrast=1.0), "contrast"), (dict(contrast=-0.5), "contrast"), (dict(contrast=float("nan")), "contrast"),
    (dict(brightness=1.5), "brightness"), (dict(brightness=float("nan")), "brightness"),
    (dict(params_in=0x7002), "params_in"), (dict(params_out=0x7001), "params_out"),
    (dict(scale=0.5000001), "scale"), (dict(scale=-0.1), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"), (dict(rotate_rad=0.7853983), "rotate_rad"), (dict(rotate_rad=-0.1), "rotate_rad"),
    (dict(rotate_rad=float("nan")), "rotate_rad"),
])
def test_cabi_refuses_bad_arguments_before_any_launch(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("egz_resident_gather_affine") and word in msg, (rc, msg)


def test_symbol_is_declared_bound_and_exported():
    import test_cabi_symbols as T
    from egaze_amd import _lib
    assert T._declared()["egz_resident_gather_affine"] == len(_lib.SIGNATURES["egz_resident_gather_affine"][1]) == 29
    assert T._declared()["egz_resident_gather_aug"] == 27              # the entry without the affine step keeps its signature
    T.test_header_binding_and_library_agree()
