"""hipops.tvl1_flow and its stages (csrc/flow_tvl1.hip) against tests/flow_ref.py, the numpy restatement of DESIGN.md "TV-L1
optical flow": the whole solver against fp64 within a budget measured from fp32 numpy, every stage against fp32 numpy bit for bit,
the tiled solver against the one-launch-per-iteration form bit for bit, batch invariance, known translations, the quantiser and
the grey rule, data/extract_flow.py end to end, and the refusals."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as R  # noqa: E402
from test_flow_host import MAX_EPE, MEAN_EPE, TRANSLATIONS, translation_pair  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAR3 = dict(nscales=3, warps=5, iterations=30)
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ulps(a, b):
    """Largest distance in units of the last place between two float32 arrays (0 = equal bits, up to the sign of zero)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return int(np.abs(key(a) - key(b)).max())


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def three_frames(hw):
    return np.stack([R.texture(*hw, seed=3), R.texture(*hw, shift=(1.5, -0.75), seed=3), R.texture(*hw, shift=(2.25, 0.5), seed=3)])


_REF = {}


def reference(hw):
    """(frames, fp64 flow, fp32 flow) of the three-frame run at hw, computed once."""
    if hw not in _REF:
        f = three_frames(hw)
        _REF[hw] = (f, np.stack(R.tvl1_flow(f, np.float64, **PAR3)), np.stack(R.tvl1_flow(f, F32, **PAR3)))
    return _REF[hw]


# ------------------------------------------------------------------------------------------------ solver against fp64
@pytest.mark.parametrize("hw", [(50, 70), (64, 80)])
def test_solver_against_fp64(hw):
    """Budget: 8 times the distance of the fp32 numpy restatement from fp64 on the same frames (the device's summation order
    in the 16-tap sampler and a threshold branch flipping on a tie may differ from numpy's, nothing else)."""
    from egaze_amd import hipops as H
    frames, ref64, ref32 = reference(hw)
    got = np.stack([host(u) for u in H.tvl1_flow(dev(frames), **PAR3)]).astype(np.float64)
    d_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    d_dev = float(np.abs(got - ref64).max())
    print(f"tvl1_flow {hw}: fp32 numpy vs fp64 {d_ref:.3e} px, device vs fp64 {d_dev:.3e} px (budget {8 * d_ref:.3e})")
    assert 0 < d_ref < 1e-3
    assert d_dev <= 8 * d_ref, (d_dev, d_ref)


# ------------------------------------------------------------------------------------------------ stage by stage, 33 x 47
HW = (33, 47)


def test_stage_grey_exact():
    from egaze_amd import hipops as H
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (3,) + HW + (3,), dtype=np.uint8)
    x[0, 0, :8] = [[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)]
    want = R.bgr_to_gray(x)
    assert np.array_equal(host(H.bgr_to_gray_u8(dev(x))), want)
    assert np.array_equal(host(H.bgr_to_gray_u8(dev(x.transpose(0, 3, 1, 2)))), want)            # planar


def test_stage_gaussians_bit_for_bit():
    from egaze_amd import hipops as H
    frames = three_frames(HW)
    pre = R.gauss_filter(frames, R.PRESMOOTH_SIGMA, F32)
    assert ulps(host(H.flow_gauss(dev(frames), H.FLOW_PRESMOOTH_SIGMA)), pre) == 0
    sig = R.pyramid_sigma(0.5)
    assert H.flow_pyramid_sigma(0.5) == sig
    assert ulps(host(H.flow_gauss(dev(pre), sig)), R.gauss_filter(pre, sig, F32)) == 0


def test_stage_pyramid_level_and_flow_upsampling_bit_for_bit():
    from egaze_amd import hipops as H
    assert H.flow_level_sizes(*HW, 5, 0.5) == R.level_sizes(*HW, 5, 0.5) == [(33, 47), (17, 24)]
    pre = R.gauss_filter(three_frames(HW), R.PRESMOOTH_SIGMA, F32)
    coarse = R.pyramid_down(pre, 0.5, F32)
    got = H.flow_resample(H.flow_gauss(dev(pre), R.pyramid_sigma(0.5)), (17, 24))
    assert ulps(host(got), coarse) == 0
    u = np.random.default_rng(1).normal(0, 2, (2, 17, 24)).astype(F32)
    scale = F32(47) / F32(24)
    assert ulps(host(H.flow_resample(dev(u), HW, float(scale))), R.resample(u, 33, 47, scale, F32)) == 0


def _warp_inputs():
    img = R.gauss_filter(three_frames(HW), R.PRESMOOTH_SIGMA, F32)
    u = np.random.default_rng(2).normal(0, 3, (2, 2) + HW).astype(F32)
    u[:, :, 0, :] = 40.0                    # far outside: the position clamps
    u[:, :, 1, :] = -40.0
    u[:, :, 2, :5] = [0.0, 1.0, -1.0, 0.5, -0.5]
    return img, u


def test_stage_gradient_and_warp_bit_for_bit():
    from egaze_amd import hipops as H
    img, u = _warp_inputs()
    gx, gy = R.grad_central(img[1:], F32)
    dgx, dgy = H.flow_grad(dev(img[1:]))
    assert ulps(host(dgx), gx) == 0 and ulps(host(dgy), gy) == 0
    want = R.warp(img[:-1], img[1:], gx, gy, u[0], u[1], F32)
    got = host(H.tvl1_warp(dev(img), dgx, dgy, dev(u)))
    for name, g, w in zip(("gx", "gy", "g2", "rc"), got, want):
        assert ulps(g, w) == 0, name


def _random_state(hw, n, seed):
    """A state and constants that take every branch of the threshold step, flat pixels (g2 = 0) included."""
    rng = np.random.default_rng(seed)
    state = rng.normal(0, 1, (6, n) + hw).astype(F32)
    state[2:] *= F32(0.5)
    gx, gy = rng.normal(0, 8, (2, n) + hw).astype(F32)
    flat = rng.random((n,) + hw) < 0.1
    gx[flat] = 0
    gy[flat] = 0
    rc = (rng.normal(0, 1, (n,) + hw) * rng.choice([0.1, 5.0, 200.0], (n,) + hw)).astype(F32)
    return state, np.stack([gx, gy, gx * gx + gy * gy, rc])


@pytest.mark.parametrize("n", [1, 3])
def test_stage_inner_iteration_bit_for_bit(n):
    from egaze_amd import hipops as H
    state, consts = _random_state(HW, 2, 4)
    want = R.iterate(state, consts, n, 0.15, 0.3, 0.25, F32)
    got = host(H.tvl1_iterate(dev(state), dev(consts), n, fused=1))
    for name, g, w in zip(("u1", "u2", "p11", "p12", "p21", "p22"), got, want):
        assert ulps(g, w) == 0, name


# ------------------------------------------------------------------------------------------------ tiling
@pytest.mark.parametrize("hw", [(33, 47), (64, 64), (50, 70)])
@pytest.mark.parametrize("iterations", [7, 30])
def test_tiled_solver_equals_one_launch_per_iteration(hw, iterations):
    """The pair under test sits between two pairs that are NaN in every plane, and the ping-pong buffer starts as NaN: a read
    across the image border, or a pixel left unwritten, would show."""
    from egaze_amd import hipops as H
    assert H.LIB.egz_tvl1_default_k() in H.FLOW_FUSED[1:]
    state, consts = _random_state(hw, 3, 5)
    state[:, 0] = state[:, 2] = np.nan
    consts[:, 0] = consts[:, 2] = np.nan
    s, c = dev(state), dev(consts)
    nan = torch.full_like(s, float("nan"))
    want = H.tvl1_iterate(s, c, iterations, fused=1, scratch=nan.clone())[:, 1]
    assert bool(torch.isfinite(want).all())
    assert not same_bits(want, s[:, 1])
    for k in (None,) + H.FLOW_FUSED[1:]:
        got = H.tvl1_iterate(s, c, iterations, fused=k, scratch=nan.clone())[:, 1]
        for m, name in enumerate(("u1", "u2", "p11", "p12", "p21", "p22")):
            assert same_bits(got[m], want[m]), (k, name)


# ------------------------------------------------------------------------------------------------ batch
def test_a_pair_alone_equals_the_pair_in_a_batch():
    from egaze_amd import hipops as H
    hw = (50, 70)
    frames = np.stack([R.texture(*hw, shift=(0.7 * i, -0.4 * i), seed=6) for i in range(6)])
    x = dev(frames)
    u1, u2 = H.tvl1_flow(x, **PAR3)
    assert u1.shape == u2.shape == (5,) + hw and u1.dtype == torch.float32
    a1, a2 = H.tvl1_flow(x[2:4], **PAR3)                                   # F = 2
    assert a1.shape == (1,) + hw
    assert same_bits(a1[0], u1[2]) and same_bits(a2[0], u2[2])
    f1, f2 = H.tvl1_flow(x, fused=1, **PAR3)                               # and the whole chain does not depend on k
    assert same_bits(f1, u1) and same_bits(f2, u2)


# ------------------------------------------------------------------------------------------------ known motion
@pytest.mark.parametrize("shift,hw", TRANSLATIONS)
def test_device_recovers_a_translation(shift, hw):
    from egaze_amd import hipops as H
    u1, u2 = H.tvl1_flow(dev(translation_pair(shift, hw)), **PAR3)
    mean, mx = R.endpoint_error(host(u1).astype(np.float64), host(u2).astype(np.float64), shift, trim=8)
    print(f"{hw} shift {shift}: endpoint error mean {mean:.4f} max {mx:.4f} px")
    assert mean <= MEAN_EPE and mx <= MAX_EPE, (mean, mx)


# ------------------------------------------------------------------------------------------------ quantiser
def test_quantiser_exact():
    from egaze_amd import hipops as H
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.normal(0, 12, 20000), rng.uniform(-20.001, 20.001, 20000),
                        [20.0, -20.0, 20.000002, -20.000002, 0.0, np.inf, -np.inf]]).astype(F32)
    for bound in (20.0, 15.0):
        assert np.array_equal(host(H.flow_to_u8(dev(v), bound)), R.flow_to_u8(v, bound)), bound
    ties = np.arange(-127, 128).astype(F32).reshape(5, 51)                 # bound 127.5: every integer is a tie
    got = host(H.flow_to_u8(dev(ties), 127.5))
    assert got.shape == ties.shape and (got % 2 == 0).all()
    assert np.array_equal(got, R.flow_to_u8(ties, 127.5))


# ------------------------------------------------------------------------------------------------ end to end
def _pil_jpeg(plane, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(plane).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def test_extract_flow_end_to_end(tmp_path):
    from PIL import Image
    from egaze_amd import hipops as H
    from egaze_amd.data import extract_flow as X
    hw, quality = (64, 80), 90
    src = tmp_path / "frames" / "clip"
    src.mkdir(parents=True)
    for i in range(6):
        rgb = np.stack([R.texture(*hw, shift=(0.5 * i * i, -0.3 * i * i), seed=s) for s in (8, 9, 10)], -1)
        Image.fromarray(rgb).save(src / ("img_%05d.jpg" % (i + 1)), quality=95)
    dst = tmp_path / "flow"
    n = X.main(["--framePath", str(tmp_path / "frames"), "--flowPath", str(dst), "--chunk", "2", "--quality", str(quality),
                "--nscales", "3"])
    assert n == 10
    assert sorted(os.listdir(dst / "clip")) == sorted(f % k for f in X.FLOW_NAMES for k in range(1, 6))
    # the same planes from the public functions, all pairs in one batch
    paths = [str(src / ("img_%05d.jpg" % (i + 1))) for i in range(6)]
    bgr = X.decode_frames(paths, None, DEV)
    want_bgr = np.stack([np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1] for p in paths])
    assert np.array_equal(host(bgr).transpose(0, 2, 3, 1), want_bgr)
    u1, u2 = H.tvl1_flow(H.bgr_to_gray_u8(bgr), nscales=3)
    planes = [host(H.flow_to_u8(u, 20.0)) for u in (u1, u2)]
    assert (np.diff(planes[0].mean(axis=(1, 2))) > 3).all()                 # real flows: 0.5, 1.5 ... 4.5 px, 6.4 levels apart
    for c, fmt in enumerate(X.FLOW_NAMES):
        for k in range(5):
            data = (dst / "clip" / (fmt % (k + 1))).read_bytes()
            assert data == _pil_jpeg(planes[c][k], quality), (fmt, k)
            # ... and the file decodes to that plane up to the JPEG's own loss: at quality 90 the luminance steps are at
            # most 24 (11.5 on average), and a rounding error of q / sqrt(12) per coefficient keeps the pixels within sqrt(mean q^2 / 12) = 3.9 grey levels RMS
            back = np.asarray(Image.open(io.BytesIO(data)))
            assert back.shape == hw
            assert np.sqrt(np.mean((back.astype(np.float64) - planes[c][k]) ** 2)) < 4.0


# ------------------------------------------------------------------------------------------------ refusals
class _Recorder:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            if not name.endswith(("_bytes", "_k")):
                self.calls.append(name)
            return fn(*a)
        return call


def test_refusals_launch_nothing(monkeypatch):
    from egaze_amd import _lib
    from egaze_amd import hipops as H
    import sys
    rec = _Recorder(H.LIB)
    monkeypatch.setattr(H, "LIB", rec)
    for name, mod in list(sys.modules.items()):       # every family module binds the one proxy under its own name
        if name.startswith(H.__name__ + ".") and getattr(mod, "LIB", None) is not None:
            monkeypatch.setattr(mod, "LIB", rec)
    ok = torch.zeros((3, 32, 40), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="expected a HIP"):
        H.tvl1_flow(ok.cpu())
    with pytest.raises(RuntimeError, match="expected a HIP"):
        H.flow_to_u8(torch.zeros(4))
    with pytest.raises(RuntimeError, match="expected a HIP"):
        H.bgr_to_gray_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="frames_gray_u8"):
        H.tvl1_flow(ok.float())
    with pytest.raises(ValueError, match="frames_gray_u8"):
        H.tvl1_flow(ok[:, :15])                                             # H < 16
    with pytest.raises(ValueError, match="frames_gray_u8"):
        H.tvl1_flow(ok[:1])                                                 # F = 1
    with pytest.raises(ValueError, match="frames_gray_u8"):
        H.tvl1_flow(ok[0])
    for name in ("tau", "lam", "theta", "nscales", "zfactor", "warps", "iterations"):
        for bad in (0, -1):
            with pytest.raises(ValueError, match=name):
                H.tvl1_flow(ok, **{name: bad})
    with pytest.raises(ValueError, match="zfactor"):
        H.tvl1_flow(ok, zfactor=1.0)
    with pytest.raises(ValueError, match="fused"):
        H.tvl1_flow(ok, fused=5)
    with pytest.raises(ValueError, match="bound"):
        H.flow_to_u8(torch.zeros(4, device=DEV), bound=0.0)
    with pytest.raises(ValueError, match="u must be float32"):
        H.flow_to_u8(ok)
    with pytest.raises(ValueError, match="frames"):
        H.bgr_to_gray_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=DEV))
    assert rec.calls == []
    # the library refuses what the wrappers would have let through, with its error code, and launches nothing either
    raw = _lib.LIB
    f = torch.zeros(6 * 2 * 32 * 40, device=DEV)
    u = torch.empty((2, 32, 40), device=DEV)
    g, r = H._flow_taps(torch.device(DEV), 0.8)
    nb = raw.egz_tvl1_flow_ws_bytes(3, 32, 40, 3, 0.5)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def flow(F=3, Hh=32, W=40, frames=ok.data_ptr(), tau=0.25, it=30, k=0, wsb=nb):
        return raw.egz_tvl1_flow(frames, F, Hh, W, g.data_ptr(), r, g.data_ptr(), r, tau, 0.15, 0.3, 3, 0.5, 5, it, k,
                                 ws.data_ptr(), wsb, u.data_ptr(), u.data_ptr(), None)
    assert raw.egz_tvl1_flow_ws_bytes(1, 32, 40, 3, 0.5) == 0 and raw.egz_tvl1_flow_ws_bytes(3, 8, 40, 3, 0.5) == 0
    for bad in (dict(F=1), dict(Hh=15), dict(W=2049), dict(frames=None), dict(tau=0.0), dict(it=0), dict(k=5), dict(wsb=nb - 1)):
        assert flow(**bad) != 0, bad
        assert "egz_tvl1_flow" in raw.egz_last_error().decode()
    assert raw.egz_tvl1_iterate(f.data_ptr(), f.data_ptr(), f.data_ptr(), 2, 32, 40, 5, 1, 0.25, 0.15, 0.3, None) != 0
    assert raw.egz_tvl1_iterate(f.data_ptr(), None, f.data_ptr(), 2, 32, 40, 5, 1, 0.25, 0.15, 0.3, None) != 0
    assert raw.egz_flow_to_u8(None, 4, 20.0, None, None) != 0
    assert raw.egz_bgr_to_gray_u8(None, 1, 4, 4, 0, None, None) != 0
    torch.cuda.synchronize()
