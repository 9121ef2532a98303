"""hipops.jpeg_roundtrip (csrc/jpeg_roundtrip.hip) against the pair it stands for, jpeg_decode(jpeg_encode(x, q)): equal bit
for bit over sizes with partial blocks on either axis, every quality class, four kinds of content, one plane to 66,000;
scatter through plane_index, the out-of-range status, in place, and the wrapper's refusals.  The pair itself is checked
against Pillow / cv2 by test_hip_jpeg_encode.py and test_hip_jpeg_decode.py, the per-block chain against Pillow by
test_jpeg_roundtrip_host.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (7, 9), (8, 8), (9, 17), (33, 250), (64, 64), (224, 224)]
QUALITIES = [1, 50, 75, 95, 100]
KINDS = ["noise", "smooth", "two-level", "near-saturated"]


def content(kind, n, h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * KINDS.index(kind) + h * 7 + w)
    shape = (n, h, w)
    if kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        a = (x * rng.uniform(0, 6, (n, 1, 1)) + y * rng.uniform(0, 6, (n, 1, 1))) + rng.normal(0, 2, shape)
    elif kind == "two-level":
        a = rng.integers(0, 2, shape) * 255
    else:
        a = np.where(rng.random(shape) < 0.5, rng.integers(0, 4, shape), rng.integers(252, 256, shape))
    return torch.from_numpy(np.clip(a, 0, 255).astype(np.uint8)).to(DEV)


def pair(x, q):
    """jpeg_decode(jpeg_encode(x, q)): the reference."""
    from egaze_amd import hipops as H
    n, h, w = x.shape
    data, off, st = H.jpeg_encode(x, quality=q)
    dec, dst = H.jpeg_decode(data, off, (h, w), [1] * n, n3=0)
    assert not int(st.abs().max()) and not int(dst.abs().max())
    return dec.view(n, h, w)


def ok(status, n):
    assert status.dtype == torch.int32 and status.shape == (n,) and not int(status.abs().max())


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equals_encode_then_decode(hw):
    from egaze_amd import hipops as H
    h, w = hw
    for kind in KINDS:
        x = content(kind, 3, h, w)
        for q in QUALITIES:
            got, status = H.jpeg_roundtrip(x, q)
            ok(status, 3)
            want = pair(x, q)
            assert got.shape == x.shape and got.dtype == torch.uint8
            assert torch.equal(got, want), (hw, kind, q, int((got != want).sum()))
            if kind == "noise" and q == 1 and h * w >= 64:
                assert not torch.equal(got, x)             # a lossy step did run


@pytest.mark.parametrize("n", [1, 3, 82])
def test_plane_counts(n):
    from egaze_amd import hipops as H
    x = torch.cat([content(k, (n + 3) // 4, 224, 224, seed=n) for k in KINDS])[:n].contiguous()
    got, status = H.jpeg_roundtrip(x)                      # quality 95, predict's chunk of 32 at n = 82
    ok(status, n)
    assert torch.equal(got, pair(x, 95))


def test_66000_planes_pass_any_grid_limit():
    from egaze_amd import hipops as H
    n = 66000
    x = torch.cat([content(k, n // 4, 8, 8, seed=5) for k in KINDS])
    got, status = H.jpeg_roundtrip(x, 75)
    ok(status, n)
    want = torch.cat([pair(x[:33000], 75), pair(x[33000:], 75)])          # jpeg_encode takes 65,535 images per call
    assert torch.equal(got, want)
    assert torch.equal(got[-1], want[-1]) and torch.equal(got[65535:65537], want[65535:65537])


def test_scatter_into_a_pool_leaves_the_other_planes():
    from egaze_amd import hipops as H
    x = content("smooth", 5, 33, 50)
    want = pair(x, 95)
    pool = torch.full((9, 33, 50), 0xA5, dtype=torch.uint8, device=DEV)
    index = [7, 0, 4, 8, 2]
    for table in (index, torch.tensor(index), torch.tensor(index, device=DEV)):
        pool.fill_(0xA5)
        out, status = H.jpeg_roundtrip(x, 95, out=pool, plane_index=table)
        assert out is pool
        ok(status, 5)
        for i, p in enumerate(index):
            assert torch.equal(pool[p], want[i]), (i, p)
        for p in set(range(9)) - set(index):
            assert bool((pool[p] == 0xA5).all()), p
    flat = torch.full((9 * 33 * 50,), 0xA5, dtype=torch.uint8, device=DEV)     # any shape made of whole planes
    H.jpeg_roundtrip(x, 95, out=flat, plane_index=index)
    assert torch.equal(flat.view(9, 33, 50), pool)


def test_out_of_range_index_is_flagged_and_not_written():
    from egaze_amd import hipops as H
    x = content("noise", 4, 9, 17)
    want = pair(x, 50)
    pool = torch.full((3, 9, 17), 0xA5, dtype=torch.uint8, device=DEV)
    guard = torch.full((4, 9, 17), 0xA5, dtype=torch.uint8, device=DEV)       # allocated right after the pool
    _, status = H.jpeg_roundtrip(x, 50, out=pool, plane_index=[1, 3, -1, 0])
    assert status.cpu().tolist() == [0, 1, 1, 0]
    assert torch.equal(pool[1], want[0]) and torch.equal(pool[0], want[3])
    assert bool((pool[2] == 0xA5).all()) and bool((guard == 0xA5).all())
    assert H.JPEG_ROUNDTRIP_STATUS[1]


@pytest.mark.parametrize("hw", [(9, 17), (224, 224), (33, 250)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place(hw):
    from egaze_amd import hipops as H
    x = content("noise", 6, *hw)
    want, _ = H.jpeg_roundtrip(x, 75)
    assert torch.equal(want, pair(x, 75))
    y = x.clone()
    out, status = H.jpeg_roundtrip(y, 75, out=y)
    ok(status, 6)
    assert out is y and torch.equal(y, want)


def test_refusals():
    from egaze_amd import hipops as H
    x = content("noise", 2, 16, 16)
    with pytest.raises(RuntimeError, match="HIP"):
        H.jpeg_roundtrip(x.cpu())
    with pytest.raises(RuntimeError, match="HIP"):
        H.jpeg_roundtrip(x.cpu().numpy())
    with pytest.raises(ValueError, match="uint8"):
        H.jpeg_roundtrip(x.float())
    for bad in (x[0], x[None]):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            H.jpeg_roundtrip(bad)
    for q in (0, 101, -1, True, 95.0, "95"):
        with pytest.raises(ValueError, match="quality"):
            H.jpeg_roundtrip(x, q)
    with pytest.raises(ValueError, match="no plane"):
        H.jpeg_roundtrip(x[:0])
    with pytest.raises(ValueError, match="plane_index= needs out="):
        H.jpeg_roundtrip(x, plane_index=[0, 1])
    pool = torch.zeros((4, 16, 16), dtype=torch.uint8, device=DEV)
    for table in ([0], [0, 1, 2], torch.zeros((2, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match="plane ind|1-D"):
            H.jpeg_roundtrip(x, out=pool, plane_index=table)
    for out in (torch.zeros(4 * 256 + 1, dtype=torch.uint8, device=DEV), pool.float(), pool.cpu(), pool[:, :, :8],
                torch.zeros(0, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="whole 16 x 16 planes"):
            H.jpeg_roundtrip(x, out=out)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="whole 16 x 16 planes"):
            H.jpeg_roundtrip(x, out=pool.to("cuda:1"))
    big = content("noise", 4, 16, 16)
    with pytest.raises(ValueError, match="overlaps"):       # a permutation inside the source
        H.jpeg_roundtrip(big[:2], out=big, plane_index=[1, 0])
    with pytest.raises(ValueError, match="overlaps"):       # shifted by one plane
        H.jpeg_roundtrip(big[:2], out=big[1:3])
    assert bool((pool == 0).all())
    H.jpeg_roundtrip(big[:2], out=big[2:])                  # disjoint halves of one tensor
