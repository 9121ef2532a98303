"""Host side of the augmented resident gather (tests/augment_ref.py, hipops.AugSpec, data/resident.py's stamp, the CLI flags,
egz_resident_gather_aug's argument checks).  No GPU: nothing is launched."""
import numpy as np
import pytest
import torch

import augment_ref as A
from test_resident_host import resident_tree

SETTING = dict(flip_thr=1 << 31, shift=16, contrast=0.2, brightness=0.1)


# ----------------------------------------------------------------------------- the draw
# computed once on a CPU with the definition of DESIGN.md section 20; pinned so that restatement and kernel cannot drift together
KNOWN = [
    # epoch, sample, flip, dy, dx, a, b, word[0]
    (0, 0, 1, -12, -11, 1.1838943, 0.0065886974, 0x5f47167dab1e6f33),
    (0, 1, 0, -1, 11, 1.1520585, -0.08140608, 0xdb0f9160fb234b5f),
    (0, 6, 1, -11, 1, 1.1332113, -0.057996143, 0x0de2eb6ba2168b85),
    (0, (1 << 33) + 5, 0, -16, -5, 1.0035169, 0.028425122, 0xa8cd0661d78ecc78),
    (3, 1, 0, 1, 7, 0.88284904, 0.07916436, None),
]


@pytest.mark.parametrize("epoch,sample,flip,dy,dx,a,b,word0", KNOWN)
def test_known_answers(epoch, sample, flip, dy, dx, a, b, word0):
    got = A.draw(1, epoch, sample, **SETTING)
    assert got[:3] == (flip, dy, dx)
    assert got[3].dtype == np.float32 and got[3] == np.float32(a) and got[4] == np.float32(b)
    if word0 is not None:
        assert A.words(1, epoch, sample)[0] == word0


def test_draw_depends_on_the_sample_number_not_on_the_batch():
    a = A.draw_rows(1, 0, [4, 1, 1, 0], **SETTING)
    b = A.draw_rows(1, 0, [0, 9, 4, 7, 1], **SETTING)
    assert np.array_equal(a[1], a[2])                                  # a repeat within a batch
    assert np.array_equal(a[0], b[2]) and np.array_equal(a[1], b[4]) and np.array_equal(a[3], b[0])
    assert len({tuple(r) for r in A.draw_rows(1, 0, range(64), **SETTING)}) == 64


def test_epoch_and_seed_change_the_draw():
    base = A.draw_rows(1, 0, range(32), **SETTING)
    for other in (A.draw_rows(1, 1, range(32), **SETTING), A.draw_rows(2, 0, range(32), **SETTING)):
        assert not np.array_equal(base, other)
        assert (base == other).all(axis=1).sum() == 0
    assert np.array_equal(base, A.draw_rows(1, 0, range(32), **SETTING))


def test_flip_threshold_never_and_always():
    assert A.flip_threshold(0.0) == 0 and A.flip_threshold(1.0) == 1 << 32 and A.flip_threshold(0.5) == 1 << 31
    kw = dict(shift=3, contrast=0.0, brightness=0.0)
    assert not any(A.draw(5, 0, s, flip_thr=0, **kw)[0] for s in range(500))
    assert all(A.draw(5, 0, s, flip_thr=1 << 32, **kw)[0] for s in range(500))
    half = sum(A.draw(5, 0, s, flip_thr=1 << 31, **kw)[0] for s in range(2000))
    assert 850 < half < 1150                                           # 1000 +- 6.7 sigma of a fair coin


def test_zero_amplitudes_give_the_neutral_parameters():
    for s in range(200):
        flip, dy, dx, a, b = A.draw(9, 2, s, flip_thr=0, shift=0, contrast=0.0, brightness=0.0)
        assert (flip, dy, dx) == (0, 0, 0) and a == np.float32(1) and b == np.float32(0)
    dys = {A.draw(9, 2, s, flip_thr=0, shift=2, contrast=0.5, brightness=0.5)[1] for s in range(400)}
    assert dys == {-2, -1, 0, 1, 2}
    ab = np.array([A.draw(9, 2, s, flip_thr=0, shift=2, contrast=0.5, brightness=0.25)[3:] for s in range(400)])
    assert 0.5 <= ab[:, 0].min() < 0.6 and 1.4 < ab[:, 0].max() < 1.5 and -0.25 <= ab[:, 1].min() and ab[:, 1].max() < 0.25


# ----------------------------------------------------------------------------- applying the parameters
def _consts():
    from egaze_amd.data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    return IMAGE_MEAN + FLOW_MEAN + (0.0,), IMAGE_STD + FLOW_STD + (1.0,)


def _planes(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (24, H, W), dtype=np.uint8)


def test_identity_is_the_plain_normalisation():
    mean, std = _consts()
    full = np.arange(256, dtype=np.uint8).reshape(1, 16, 16).repeat(24, 0)             # every byte value in every plane
    for planes in (_planes(6, 12), full):
        raw = A.geometric(planes, 0, 0, 0)
        assert np.array_equal(raw, planes)
        t = torch.from_numpy(planes)
        want = (t.float().div(255) - torch.tensor(mean).view(24, 1, 1)) / torch.tensor(std).view(24, 1, 1)
        got = A.normalise(raw, *A.IDENTITY[3:], mean, std)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))


def test_geometry_by_hand():
    H, W = 3, 4
    p = np.zeros((24, H, W), dtype=np.uint8)
    p[:] = np.arange(12, dtype=np.uint8).reshape(H, W) + 1
    out = A.geometric(p, 0, 1, -1)                                     # out(y, x) = src(y - 1, x + 1)
    assert out[0].tolist() == [[2, 3, 4, 4], [2, 3, 4, 4], [6, 7, 8, 8]]            # edge replicate
    assert out[23].tolist() == [[0, 0, 0, 0], [2, 3, 4, 0], [6, 7, 8, 0]]           # the ground truth: 0 outside
    out = A.geometric(p, 1, 0, 1)                                      # out(y, x) = F(y, x - 1), F(y, x) = src(y, 3 - x)
    assert out[1].tolist() == [[4, 4, 3, 2], [8, 8, 7, 6], [12, 12, 11, 10]]
    assert out[3].tolist() == [[251, 251, 252, 253], [247, 247, 248, 249], [243, 243, 244, 245]]  # x-flow: 255 - byte
    assert out[4].tolist() == out[1].tolist()                          # y-flow keeps its bytes
    assert out[23].tolist() == [[0, 4, 3, 2], [0, 8, 7, 6], [0, 12, 11, 10]]
    assert (A.geometric(p, 0, 3, 0)[23] == 0).all() and (A.geometric(p, 1, 0, -4)[23] == 0).all()
    assert (A.geometric(p, 0, -7, 0)[0] == p[0, 2]).all()              # far outside: the last row everywhere


def test_flip_twice_is_the_identity():
    p = _planes(5, 8, seed=3)
    pre = p[:, :, ::-1].copy()
    pre[A.FLOW_X, :, :] = 255 - pre[A.FLOW_X, :, :]                    # a pre-flipped array, its x-planes inverted
    assert np.array_equal(A.geometric(pre, 1, 0, 0), p)
    assert np.array_equal(A.geometric(A.geometric(p, 1, 0, 0), 1, 0, 0), p)
    assert not np.array_equal(A.geometric(p, 1, 0, 0)[3], p[3, :, ::-1])            # the inversion happened


def test_photometric_step_is_on_the_colour_frame_only_and_clamps():
    mean, std = _consts()
    full = np.arange(256, dtype=np.uint8).reshape(1, 16, 16).repeat(24, 0)
    base = A.normalise(full, np.float32(1), np.float32(0), mean, std)
    got = A.normalise(full, np.float32(1.75), np.float32(-0.25), mean, std)
    assert np.array_equal(got[3:], base[3:]) and not np.array_equal(got[:3], base[:3])
    m, s = np.float32(mean[0]), np.float32(std[0])
    assert got[0].min() == (np.float32(0) - m) / s and got[0].max() == (np.float32(1) - m) / s
    x = np.float32(100) / np.float32(255)
    v = np.float32(np.float32(np.float32(1.75) * x) + np.float32(-0.25))
    assert got[0].reshape(-1)[100] == (v - m) / s


def test_rows_round_trip():
    params = [A.draw(1, 0, s, **SETTING) for s in range(5)] + [A.IDENTITY]
    r = A.rows(params)
    assert r.dtype == np.int32 and r.shape == (6, 5) and r[5].tolist() == [0, 0, 0, 0x3f800000, 0]
    assert A.unrows(r) == params


# ----------------------------------------------------------------------------- AugSpec
def test_augspec_parse_round_trips():
    from egaze_amd.hipops import AugSpec
    s = AugSpec.parse("flip=0.5,shift=16,contrast=0.2,brightness=0.1")
    assert s == AugSpec(flip=0.5, shift=16, contrast=0.2, brightness=0.1, seed=0)
    assert s.flip_thr == 1 << 31 == A.flip_threshold(0.5)
    assert AugSpec.parse(str(s)) == s
    assert AugSpec.parse("flip") == AugSpec(flip=0.5) and AugSpec.parse(" shift = 3 , flip ") == AugSpec(flip=0.5, shift=3)
    assert AugSpec.parse("flip=1,seed=7").flip_thr == 1 << 32 and AugSpec.parse("flip=1,seed=7").seed == 7
    assert AugSpec.parse("flip=0.25,seed=7", seed=9) == AugSpec(flip=0.25, seed=9)
    big = AugSpec(flip=0.3, shift=32767, contrast=0.999, brightness=0.5, seed=(1 << 64) - 1)
    assert AugSpec.parse(str(big)) == big
    assert AugSpec() == AugSpec(0.0, 0, 0.0, 0.0, 0) and AugSpec().flip_thr == 0
    with pytest.raises(Exception):
        s.shift = 2                                                    # frozen
    assert hash(s) == hash(AugSpec.parse(str(s)))


@pytest.mark.parametrize("text", ["", "flop=1", "flip=2", "flip=-0.1", "shift", "shift=1.5", "shift=-1", "shift=32768",
                                  "contrast=1", "contrast=-0.1", "brightness=1.0", "brightness=x", "flip,flip=0.2", "seed=-1",
                                  "flip=0.5;shift=2", "flip=nan", "seed=18446744073709551616"])
def test_augspec_refusals(text):
    from egaze_amd.hipops import AugSpec
    with pytest.raises(ValueError, match="AugSpec"):
        AugSpec.parse(text)


def test_augspec_constructor_refusals():
    from egaze_amd.hipops import AugSpec
    for kw in (dict(flip=1.5), dict(shift=1.0), dict(shift=True), dict(contrast="0.1"), dict(brightness=1.0), dict(seed=1 << 64),
               dict(seed=0.5), dict(flip=float("nan"))):
        with pytest.raises(ValueError, match="AugSpec"):
            AugSpec(**kw)


# ----------------------------------------------------------------------------- CLI
def _parsers():
    from egaze_amd import gaze_full, streamtrain
    return gaze_full.build_parser(), streamtrain.build_parser("spatial"), streamtrain.build_parser("temporal")


def test_cli_flags_are_absent_unless_given_and_parse():
    from egaze_amd import streamtrain
    from egaze_amd.hipops import AugSpec
    for parser in _parsers():
        ns = parser.parse_args([])
        assert not hasattr(ns, "augment") and not hasattr(ns, "augment_seed") and streamtrain.augment_spec(ns) is None
        ns = parser.parse_args(["--gpu_resident"])
        assert not hasattr(ns, "augment") and streamtrain.augment_spec(ns) is None
        ns = parser.parse_args(["--gpu_resident", "--augment", "flip,shift=16", "--augment_seed", "5"])
        assert ns.augment == "flip,shift=16" and ns.augment_seed == 5
        assert streamtrain.augment_spec(ns) == AugSpec(flip=0.5, shift=16, seed=5)
        assert streamtrain.augment_spec(parser.parse_args(["--augment", "contrast=0.2", "--gpu_resident"])) == \
            AugSpec(contrast=0.2)


@pytest.mark.parametrize("argv,word", [
    (["--augment", "flip"], "--gpu_resident"),
    (["--augment", "flip", "--gpu_decode"], "host loading path"),
    (["--augment_seed", "3"], "--gpu_resident"),
    (["--gpu_resident", "--augment_seed", "3"], "without --augment"),
    (["--gpu_resident", "--augment", "shift=99999"], "32767"),
    (["--gpu_resident", "--augment", "zoom=2"], "zoom"),
])
def test_cli_refuses_augment_without_gpu_resident_and_bad_specs(argv, word, capsys):
    for parser in _parsers():
        with pytest.raises(SystemExit) as e:
            parser.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err


# ----------------------------------------------------------------------------- the stamp
def test_collate_stamps_only_inside_augmenting(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset, augmenting
    from egaze_amd.hipops import AugSpec
    args = resident_tree(tmp_path)
    ds = ResidentSTDataset(*args, raw_u8=True)
    spec = AugSpec(flip=0.5, shift=4, seed=3)
    assert "augment" not in ds.collate_fn([ds[0], ds[1]])
    with ds.augmenting(spec, 2) as inside:
        assert inside is ds
        b = ds.collate_fn([ds[5], ds[0]])
        assert tuple(b["augment"]) == (spec, 2) and b["index"].tolist() == [5, 0] and b["resident"] is ds
        with ds.augmenting(AugSpec(seed=9), 7):
            assert tuple(ds.collate_fn([ds[1]])["augment"]) == (AugSpec(seed=9), 7)
        assert tuple(ds.collate_fn([ds[1]])["augment"]) == (spec, 2)
    assert "augment" not in ds.collate_fn([ds[0]])
    with pytest.raises(KeyError):                                      # left on the way out of an exception too
        with ds.augmenting(spec, 0):
            raise KeyError("x")
    assert "augment" not in ds.collate_fn([ds[0]])
    with pytest.raises(ValueError, match="AugSpec"):
        with ds.augmenting("flip", 0):
            pass
    # the drivers' helper: a spec and a resident dataset, else nothing happens
    with augmenting(ds, None, 1):
        assert "augment" not in ds.collate_fn([ds[0]])
    with augmenting(ds, spec, 1):
        assert tuple(ds.collate_fn([ds[0]])["augment"]) == (spec, 1)
    with augmenting(STDataset(*args, raw_u8=True), spec, 1), augmenting(None, spec, 1):
        pass


def test_a_seeded_loader_visits_the_same_batches_with_and_without_augmenting(tmp_path):
    """The stamp draws nothing from the host RNG: same samples, same batches, and the generator ends in the same state."""
    from torch.utils.data import DataLoader
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.hipops import AugSpec
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True)
    seen = {}
    for mode in ("plain", "augmented"):
        torch.manual_seed(7)
        loader = DataLoader(ds, batch_size=3, shuffle=True, num_workers=0, pin_memory=False, collate_fn=ds.collate_fn)
        if mode == "plain":
            order = [b["index"].tolist() for b in loader]
        else:
            with ds.augmenting(AugSpec(flip=0.5, shift=8), 0):
                batches = list(loader)
            assert all(tuple(b["augment"]) == (AugSpec(flip=0.5, shift=8), 0) for b in batches)
            order = [b["index"].tolist() for b in batches]
        seen[mode] = (order, torch.rand(1).item())
    assert seen["plain"] == seen["augmented"]


def test_a_stamped_batch_refuses_raw_bytes(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import to_raw_u8
    from egaze_amd.hipops import AugSpec
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True)          # no pool: the refusal comes first
    with ds.augmenting(AugSpec(flip=1.0), 0):
        b = ds.collate_fn([ds[0], ds[1]])
    with pytest.raises(RuntimeError, match="augmenting.*raw"):
        ds.gather(b, "cuda:0", raw=True)
    with pytest.raises(RuntimeError, match="augmenting.*raw"):
        to_raw_u8(b, torch.device("cuda:0"))
    with pytest.raises(RuntimeError, match="fill"):                     # an unstamped one gets as far as the missing pool
        ds.gather(ds.collate_fn([ds[0]]), "cuda:0", raw=True)


# ----------------------------------------------------------------------------- C-ABI refusals (nothing is launched)
def _call(**over):
    from egaze_amd import _lib
    a = dict(pool=0x1000, P=60, table=0x2000, N=7, idx=0x3000, B=3, H=224, W=224, mean=0x4000, std=0x5000, image=0x10000,
             flow=0x20000, gt=0x30000, nhwc=None, absmax=None, raw=None, raw_fields=7, status=0x6000, seed=1, epoch=0,
             flip_thr=1 << 31, max_shift=16, contrast=0.2, brightness=0.1, params_in=None, params_out=None, stream=None)
    a.update(over)
    rc = _lib.LIB.egz_resident_gather_aug(*a.values())
    return rc, _lib.LIB.egz_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(pool=None), "pool"), (dict(table=None), "table"), (dict(idx=None), "idx"), (dict(B=0), "B"), (dict(H=0), "H"),
    (dict(H=6, W=10), "W = 10 must be a multiple of 4"), (dict(H=4, W=3), "multiple of 4"), (dict(H=2, W=2), "multiple of 4"),
    (dict(H=65536, W=32768), "2^31"),
    (dict(image=None, flow=None, gt=None), "no output"), (dict(nhwc=0x40000), "absmax"), (dict(status=None), "status"),
    (dict(raw=0x70000, raw_fields=8), "raw_fields"),
    (dict(flip_thr=(1 << 32) + 1), "flip_thr"), (dict(max_shift=-1), "max_shift"), (dict(max_shift=32768), "max_shift"),
    (dict(contrast=1.0), "contrast"), (dict(contrast=-0.5), "contrast"), (dict(contrast=float("nan")), "contrast"),
    (dict(brightness=1.5), "brightness"), (dict(brightness=float("nan")), "brightness"),
    (dict(params_in=0x7002), "params_in"), (dict(params_out=0x7001), "params_out"),
])
def test_cabi_refuses_bad_arguments_before_any_launch(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("egz_resident_gather_aug") and word in msg, (rc, msg)


def test_symbol_is_declared_bound_and_exported():
    import test_cabi_symbols as T
    from egaze_amd import _lib
    assert T._declared()["egz_resident_gather_aug"] == len(_lib.SIGNATURES["egz_resident_gather_aug"][1]) == 27
    assert T._declared()["egz_resident_gather"] == 19                 # the plain entry keeps its signature
    T.test_header_binding_and_library_agree()


def test_status_words_name_the_new_bit():
    from egaze_amd import hipops as Hp
    assert set(Hp.RESIDENT_STATUS) == set(range(1, 8))
    for st in (4, 5, 6, 7):
        assert "augmentation row" in Hp.RESIDENT_STATUS[st]
    assert "augmentation" not in Hp.RESIDENT_STATUS[3]
