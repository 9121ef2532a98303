"""csrc/flow_tvl1.hip where tests/test_hip_flow.py does not reach: rows wider than one 256-thread block (every stage bit for bit
against fp32 numpy at 300 and 513 columns), tiles of the tiled solver that touch no image border and last tiles that are slivers,
the whole chain at four and five levels and at pyramid factors other than 0.5 -- against fp64, against the same chain composed
from the public stage wrappers (bit for bit: the workspace carving and the buffer swaps of egz_tvl1_flow), across every k and
against fp32 numpy --, a batch of 33 pairs, the workspace cache, and the 16-level cap."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as R  # noqa: E402
from test_hip_flow import DEV, F32, _random_state, dev, host, same_bits, three_frames, ulps  # noqa: E402

pytestmark = pytest.mark.gpu
WIDE = [(17, 300), (16, 513)]           # a ragged second x-block; a third x-block of one pixel
SEAM_COLUMNS = (253, 254, 255, 256, 257, 258, 259, 509, 510, 511, 512)
STATE = ("u1", "u2", "p11", "p12", "p21", "p22")


# ------------------------------------------------------------------------------------------------ stages across x-blocks
_PRE = {}


def presmoothed(hw):
    """Three frames at hw after the sigma 0.8 Gaussian, fp32 numpy, computed once."""
    if hw not in _PRE:
        _PRE[hw] = R.gauss_filter(three_frames(hw), R.PRESMOOTH_SIGMA, F32)
    return _PRE[hw]


@pytest.mark.parametrize("hw", WIDE)
def test_wide_gaussians_bit_for_bit(hw):
    from egaze_amd import hipops as H
    frames, pre = three_frames(hw), presmoothed(hw)
    for sigma in (R.PRESMOOTH_SIGMA, R.pyramid_sigma(0.5)):
        assert ulps(host(H.flow_gauss(dev(frames), sigma)), R.gauss_filter(frames, sigma, F32)) == 0, ("uint8", sigma)
    # zfactor 0.3: radius 8, so the taps of columns 248 .. 263 cross the seam between the first two blocks
    for sigma in (R.PRESMOOTH_SIGMA, R.pyramid_sigma(0.5), R.pyramid_sigma(0.3)):
        assert ulps(host(H.flow_gauss(dev(pre), sigma)), R.gauss_filter(pre, sigma, F32)) == 0, ("float", sigma)


@pytest.mark.parametrize("fine,coarse", [((32, 600), (16, 300)), ((33, 513), (17, 257))])
def test_wide_pyramid_level_bit_for_bit(fine, coarse):
    from egaze_amd import hipops as H
    pre = presmoothed(fine)
    want = R.pyramid_down(pre, 0.5, F32)
    assert want.shape == (3,) + coarse
    got = H.flow_resample(H.flow_gauss(dev(pre), R.pyramid_sigma(0.5)), coarse)
    assert ulps(host(got), want) == 0


@pytest.mark.parametrize("coarse,fine", [((17, 257), (33, 513)), ((16, 150), (32, 300))])
def test_wide_flow_upsampling_bit_for_bit(coarse, fine):
    from egaze_amd import hipops as H
    u = np.random.default_rng(11).normal(0, 2, (3,) + coarse).astype(F32)
    scale = F32(fine[1]) / F32(coarse[1])
    assert ulps(host(H.flow_resample(dev(u), fine, float(scale))), R.resample(u, *fine, scale, F32)) == 0


def _wide_warp_inputs(hw):
    """The clamping rows of test_hip_flow._warp_inputs, and displacements that carry the 4 x 4 taps across a block seam."""
    h, w = hw
    u = np.random.default_rng(12).normal(0, 3, (2, 2) + hw).astype(F32)
    u[:, :, 0, :] = 40.0
    u[:, :, 1, :] = -40.0
    u[:, :, 2, :5] = [0.0, 1.0, -1.0, 0.5, -0.5]
    cols = [c for c in SEAM_COLUMNS if c < w]
    assert cols and 3 + 6 <= h
    for r, d in enumerate((1.0, -1.0, 2.5, -2.5, 40.0, -40.0)):
        u[0, :, 3 + r, cols] = d                   # along x, with the random u2 of the row
    return presmoothed(hw), u


@pytest.mark.parametrize("hw", WIDE)
def test_wide_gradient_and_warp_bit_for_bit(hw):
    from egaze_amd import hipops as H
    img, u = _wide_warp_inputs(hw)
    gx, gy = R.grad_central(img[1:], F32)
    dgx, dgy = H.flow_grad(dev(img[1:]))
    assert ulps(host(dgx), gx) == 0 and ulps(host(dgy), gy) == 0
    gx3, gy3 = R.grad_central(img, F32)                                    # three planes
    d3x, d3y = H.flow_grad(dev(img))
    assert ulps(host(d3x), gx3) == 0 and ulps(host(d3y), gy3) == 0
    want = R.warp(img[:-1], img[1:], gx, gy, u[0], u[1], F32)
    got = host(H.tvl1_warp(dev(img), dgx, dgy, dev(u)))
    for name, g, w in zip(("gx", "gy", "g2", "rc"), got, want):
        assert ulps(g, w) == 0, name


@pytest.mark.parametrize("hw", WIDE)
@pytest.mark.parametrize("n", [1, 3])
def test_wide_inner_iteration_bit_for_bit(hw, n):
    from egaze_amd import hipops as H
    state, consts = _random_state(hw, 3, 13)
    want = R.iterate(state, consts, n, 0.15, 0.3, 0.25, F32)
    got = host(H.tvl1_iterate(dev(state), dev(consts), n, fused=1))
    for name, g, w in zip(STATE, got, want):
        assert ulps(g, w) == 0, name


# ------------------------------------------------------------------------------------------------ interior and sliver tiles
# (97, 130): 4 x 5 tiles, tiles interior in both axes for every K, a last tile row 1 pixel high, a last tile column 2 wide
# (70, 104): 3 x 4 tiles, the last tile column 8 wide (the K of the widest form), the last tile row 6 high
# (72, 300): 3 x 10 tiles, and the k = 1 yardstick spans two x-blocks
@pytest.mark.parametrize("hw", [(97, 130), (70, 104), (72, 300)])
@pytest.mark.parametrize("iterations", [7, 30])
def test_tiled_solver_equals_one_launch_per_iteration_on_many_tiles(hw, iterations):
    """As test_hip_flow.test_tiled_solver_equals_one_launch_per_iteration: NaN pairs on both sides, a NaN ping-pong buffer."""
    from egaze_amd import hipops as H
    state, consts = _random_state(hw, 3, 5)
    state[:, 0] = state[:, 2] = np.nan
    consts[:, 0] = consts[:, 2] = np.nan
    s, c = dev(state), dev(consts)
    nan = torch.full_like(s, float("nan"))
    want = H.tvl1_iterate(s, c, iterations, fused=1, scratch=nan.clone())[:, 1]
    assert bool(torch.isfinite(want).all())
    assert not same_bits(want, s[:, 1])
    ref = R.iterate(state[:, 1:2], consts[:, 1:2], iterations, 0.15, 0.3, 0.25, F32)          # the yardstick itself
    for m, name in enumerate(STATE):
        assert ulps(host(want[m]), ref[m][0]) == 0, name
    for k in (None,) + H.FLOW_FUSED[1:]:
        got = H.tvl1_iterate(s, c, iterations, fused=k, scratch=nan.clone())[:, 1]
        for m, name in enumerate(STATE):
            assert same_bits(got[m], want[m]), (k, name)


# ------------------------------------------------------------------------------------------------ the whole chain at depth
DEFAULT = dict(nscales=5, zfactor=0.5)
DEEP = {                                 # id: (hw, parameters, level sizes)
    "273x310": ((273, 310), DEFAULT, [(273, 310), (137, 155), (69, 78), (35, 39), (18, 20)]),
    "65x290": ((65, 290), DEFAULT, [(65, 290), (33, 145), (17, 73)]),
    "64x80-z0.8": ((64, 80), dict(nscales=10, zfactor=0.8), [(64, 80), (51, 64), (41, 51), (33, 41), (26, 33), (21, 26), (17, 21)]),
    "96x300-z0.3": ((96, 300), dict(nscales=5, zfactor=0.3), [(96, 300), (29, 90)]),
}
_DEEP_REF = {}


def deep_reference(case, dtype):
    """(frames, flow (2, 2, H, W)) of a DEEP case in fp64 or fp32 numpy, computed once and left unchanged."""
    if (case, dtype) not in _DEEP_REF:
        hw, par, _ = DEEP[case]
        flow = np.stack(R.tvl1_flow(three_frames(hw), dtype, **par))
        flow.setflags(write=False)
        _DEEP_REF[case, dtype] = flow
    return three_frames(DEEP[case][0]), _DEEP_REF[case, dtype]


def composed_flow(H, frames, nscales, zfactor, warps=5, iterations=30, fused=None):
    """R.tvl1_flow's loop, every step one public stage wrapper: what egz_tvl1_flow launches, each result in a tensor of its own."""
    x = dev(frames)
    n, sigma = x.shape[0] - 1, H.flow_pyramid_sigma(zfactor)
    pyr = [H.flow_gauss(x, H.FLOW_PRESMOOTH_SIGMA)]
    for hw in H.flow_level_sizes(*x.shape[-2:], nscales, zfactor)[1:]:
        pyr.append(H.flow_resample(H.flow_gauss(pyr[-1], sigma), hw))
    state, trace = None, []
    for img in reversed(pyr):
        h, w = img.shape[-2:]
        new = torch.zeros((6, n, h, w), dtype=torch.float32, device=DEV)
        if state is not None:
            hc, wc = state.shape[-2:]
            new[0] = H.flow_resample(state[0], (h, w), float(F32(w) / F32(wc)))
            new[1] = H.flow_resample(state[1], (h, w), float(F32(h) / F32(hc)))
        state = new
        gx, gy = H.flow_grad(img[1:])
        for _ in range(warps):
            consts = H.tvl1_warp(img, gx, gy, state[:2])
            state = H.tvl1_iterate(state, consts, iterations, fused=fused)
            trace.append(((h, w), consts, state))
    return state[0], state[1], trace


@pytest.mark.parametrize("case", list(DEEP))
def test_deep_chain_against_fp64(case):
    """Budget, as in test_hip_flow.test_solver_against_fp64: 8 times the distance of the fp32 numpy restatement from fp64 on the
    same frames (the device's summation order in the 16-tap sampler and a threshold branch flipping on a tie may differ from
    numpy's, nothing else)."""
    from egaze_amd import hipops as H
    hw, par, sizes = DEEP[case]
    assert H.flow_level_sizes(*hw, **par) == R.level_sizes(*hw, **par) == sizes
    frames, ref64 = deep_reference(case, np.float64)
    _, ref32 = deep_reference(case, F32)
    got = np.stack([host(u) for u in H.tvl1_flow(dev(frames), **par)]).astype(np.float64)
    d_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    d_dev = float(np.abs(got - ref64).max())
    print(f"tvl1_flow {hw} {par}: fp32 numpy vs fp64 {d_ref:.3e} px, device vs fp64 {d_dev:.3e} px (budget {8 * d_ref:.3e})")
    assert 0 < d_ref < 1e-3
    assert d_dev <= 8 * d_ref, (d_dev, d_ref)


@pytest.mark.parametrize("case", list(DEEP))
def test_deep_chain_equals_its_stages_composed(case):
    """Both sides launch the same kernels on the same values; only egz_tvl1_flow's carving of one workspace, its plane strides
    per level and its swaps of the two state buffers differ, so the bits must agree."""
    from egaze_amd import hipops as H
    hw, par, sizes = DEEP[case]
    x = dev(three_frames(hw))
    u1, u2 = H.tvl1_flow(x, **par)
    c1, c2, trace = composed_flow(H, three_frames(hw), **par)
    assert [t[0] for t in trace[::5]] == sizes[::-1]
    assert bool(torch.isfinite(u1).all()) and float(u1.abs().max()) > 0.5
    assert same_bits(u1, c1) and same_bits(u2, c2)


@pytest.mark.parametrize("case", ["273x310", "64x80-z0.8"])
def test_deep_chain_does_not_depend_on_k(case):
    """30 iterations are 30, 15, 10, 8, 5, 4 launches per warp for k = 1, 2, 3, 4, 6, 8: the result lands in the second buffer
    for k = 2 and 6 only, and with five and seven levels every k goes through the swap after resampling as well."""
    from egaze_amd import hipops as H
    hw, par, _ = DEEP[case]
    x = dev(three_frames(hw))
    want = H.tvl1_flow(x, fused=1, **par)
    assert {k: -(-30 // k) % 2 for k in H.FLOW_FUSED} == {1: 0, 2: 1, 3: 0, 4: 0, 6: 1, 8: 0}
    differ = []
    for k in (None,) + H.FLOW_FUSED[1:]:
        got = H.tvl1_flow(x, fused=k, **par)
        if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
            differ.append(k)
    assert differ == []
    for iterations, odd in ((7, {1, 3, 8}), (9, {1, 2, 3, 4})):              # other parities: every k is odd once
        assert {k for k in H.FLOW_FUSED if -(-iterations // k) % 2} == odd
        want = H.tvl1_flow(x, fused=1, iterations=iterations, warps=2, **par)
        for k in H.FLOW_FUSED[1:]:
            got = H.tvl1_flow(x, fused=k, iterations=iterations, warps=2, **par)
            if not (same_bits(got[0], want[0]) and same_bits(got[1], want[1])):
                differ.append((iterations, k))
    assert differ == []


@pytest.mark.parametrize("case", ["65x290", "273x310"])
def test_deep_chain_against_fp32_numpy(case):
    """Every stage equals fp32 numpy bit for bit, so the chain does."""
    from egaze_amd import hipops as H
    hw, par, _ = DEEP[case]
    frames, ref32 = deep_reference(case, F32)
    got = np.stack([host(u) for u in H.tvl1_flow(dev(frames), **par)])
    d = ulps(got, ref32)
    print(f"tvl1_flow {hw} {par}: device vs fp32 numpy {d} ulp, {int((got != ref32).sum())} of {got.size} values differ")
    assert d == 0


# ------------------------------------------------------------------------------------------------ batch and cache
def test_long_batch_pairs_alone_and_in_chunks():
    from egaze_amd import hipops as H
    from egaze_amd.data import extract_flow as X
    hw = (16, 272)
    x = dev(np.stack([R.texture(*hw, shift=(0.3 * i, -0.2 * i), seed=6) for i in range(34)]))
    u1, u2 = H.tvl1_flow(x)
    assert u1.shape == u2.shape == (33,) + hw
    assert bool(torch.isfinite(u1).all()) and float(u1[32].abs().max()) > 0.1
    for i in (0, 16, 32):
        a1, a2 = H.tvl1_flow(x[i:i + 2])                                   # F = 2
        assert a1.shape == (1,) + hw
        assert same_bits(a1[0], u1[i]) and same_bits(a2[0], u2[i]), i
    ranges = X.chunk_ranges(34, 8)
    assert ranges == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 33)]
    for first, last in ranges:                                             # consecutive chunks share one frame
        c1, c2 = H.tvl1_flow(x[first:last + 1])
        assert same_bits(c1, u1[first:last]) and same_bits(c2, u2[first:last]), (first, last)


def test_workspace_regrows_and_is_reused_for_a_shallower_pyramid():
    from egaze_amd import hipops as H
    from egaze_amd.hipops import _core
    hw = (64, 80)
    x = dev(three_frames(hw))
    key = (torch.device(DEV).index or 0, _core._stream(), 3, *hw)
    nbytes = {n: H.LIB.egz_tvl1_flow_ws_bytes(3, *hw, n, 0.5) for n in (1, 3)}
    assert 0 < nbytes[1] < nbytes[3]
    fresh = {}
    for n in (1, 3):
        H._FLOW_WS.clear()
        fresh[n] = H.tvl1_flow(x, nscales=n)
        assert [k for k in H._FLOW_WS if k[2:] == key[2:]] == [key] and H._FLOW_WS[key].numel() == nbytes[n]
    assert not same_bits(fresh[1][0], fresh[3][0])
    H._FLOW_WS.clear()
    # small; too small for 3 levels, so regrown; then kept, larger than 1 level needs and full of NaN bit patterns
    for step, (n, size) in enumerate(((1, nbytes[1]), (3, nbytes[3]), (1, nbytes[3]))):
        if step == 2:
            H._FLOW_WS[key].fill_(0xFF)
        got = H.tvl1_flow(x, nscales=n)
        assert [k for k in H._FLOW_WS if k[2:] == key[2:]] == [key], step
        assert H._FLOW_WS[key].numel() == size, step
        assert same_bits(got[0], fresh[n][0]) and same_bits(got[1], fresh[n][1]), step


# ------------------------------------------------------------------------------------------------ the 16-level cap
def test_more_than_16_scales_are_16():
    """100 x 100 at zfactor 0.9 keeps 16 pixels for 18 levels; the definition and the device stop at 16."""
    from egaze_amd import hipops as H
    hw, par = (100, 100), dict(zfactor=0.9)
    assert R.level_sizes(*hw, 20, 0.9) == H.flow_level_sizes(*hw, 20, 0.9) and len(R.level_sizes(*hw, 20, 0.9)) == 16
    frames = three_frames(hw)
    x = dev(frames)
    got20, got16, got15 = (H.tvl1_flow(x, nscales=n, **par) for n in (20, 16, 15))
    assert same_bits(got20[0], got16[0]) and same_bits(got20[1], got16[1])
    assert not same_bits(got16[0], got15[0])                               # the sixteenth level is there
    ref64 = np.stack(R.tvl1_flow(frames, np.float64, nscales=20, **par))
    ref32 = np.stack(R.tvl1_flow(frames, F32, nscales=20, **par))
    got = np.stack([host(u) for u in got20]).astype(np.float64)
    d_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    d_dev = float(np.abs(got - ref64).max())
    print(f"tvl1_flow {hw} nscales 20 zfactor 0.9: fp32 numpy vs fp64 {d_ref:.3e} px, device vs fp64 {d_dev:.3e} px "
          f"(budget {8 * d_ref:.3e})")
    assert 0 < d_ref < 1e-3
    assert d_dev <= 8 * d_ref, (d_dev, d_ref)
