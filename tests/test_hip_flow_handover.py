"""The in-memory flow hand-over on the GPU (data.extract_flow.flows_into, ResidentSTDataset.fill(flow_from=...), gaze_full
--flow_handover) against the existing path through files (extract_flow.main -> flow_x / flow_y JPEGs -> fill): pools and tables
byte for byte at three chunk sizes with both decoders, the image and ground-truth planes untouched, no file or folder written,
the counts; quality 0 against flow_to_u8; one gaze_full --train_sp epoch, checkpoint against checkpoint.

The tree is 2 videos x 30 frames of 44 x 60 (partial 8x8 blocks on both axes, above TV-L1's 16-pixel minimum); the samples are
frames 10 .. 15 and 22 .. 25, so flows 26 .. 29 are computed by no hand-over at chunk 1.  TV-L1 runs with 2 scales, 2 warps and
5 iterations: the comparison is between two routes for the same flow, not a test of the flow."""
import os

import pytest
import torch

from test_flow_handover_host import FLOWS, SAMPLES, TRAIN, VAL, flow_tree, st_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = {'tau': 0.25, 'lam': 0.15, 'theta': 0.3, 'zfactor': 0.5, 'nscales': 2, 'warps': 2, 'iterations': 5}
PARAM_ARGV = [v for k, x in PARAMS.items() for v in ("--" + k, str(x))]
N = len(SAMPLES)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("flow_handover")


@pytest.fixture(scope="module")
def tree(root):
    return flow_tree(root / "tree")


def _sets(tree, flow_path, decode="host", **fill):
    from egaze_amd.data.resident import ResidentSTDataset
    paths = dict(tree, flowPath=flow_path)
    return tuple(ResidentSTDataset(*st_args(paths, train), raw_u8=True, decode=decode).fill(DEV, **fill)
                 for train in (True, False))


@pytest.fixture(scope="module")
def without_flows(tree):
    """The image and ground-truth planes of both sets, from a fill that has no flow field."""
    from egaze_amd.data.resident import ResidentSTDataset
    out = []
    for train in (True, False):
        ds = ResidentSTDataset(*st_args(tree, train), raw_u8=True)
        ds.gpu_fields = ("image", "gt")
        ds.fill(DEV)
        assert ds.pool.shape == (4 * N, 44, 60)
        out.append(ds.pool)
    return out


@pytest.mark.parametrize("chunk", [1, 4, 32])
def test_pools_equal_the_file_paths(tree, root, without_flows, chunk):
    from egaze_amd.data import extract_flow as E
    from egaze_amd.data.resident import FlowFrom
    flow_path = str(root / f"flow_files_{chunk}")
    written = E.main(["--framePath", tree["framePath"], "--flowPath", flow_path, "--chunk", str(chunk)] + PARAM_ARGV)
    assert written == 2 * 2 * 29
    never = str(root / f"never_{chunk}")
    listing = sorted(os.listdir(str(root)))
    memory = _sets(tree, never, flow_from=FlowFrom(tree["framePath"], chunk=chunk, params=PARAMS))
    assert sorted(os.listdir(str(root))) == listing and not os.path.exists(never)         # no file, no folder
    frames = E.list_frames(os.path.join(tree["framePath"], TRAIN))
    pairs = sum(b - a for a, b in E.wanted_ranges(frames, FLOWS, chunk))
    assert pairs == {1: 25, 4: 28, 32: 29}[chunk]
    for decode in ("host", "gpu"):
        files = _sets(tree, flow_path, decode=decode)
        for f, m, plain in zip(files, memory, without_flows):
            assert m.pool.shape == f.pool.shape == (3 * N + 2 * len(FLOWS) + N, 44, 60) and m.pool.dtype == torch.uint8
            assert torch.equal(f.table, m.table) and m.table.device == m.pool.device
            assert [os.path.basename(p) for p, _, _ in f.files] == [os.path.basename(p) for p, _, _ in m.files]
            diff = int((f.pool != m.pool).sum())
            print(f"chunk {chunk}, decode {decode}: {diff} bytes differ")
            assert diff == 0 and torch.equal(f.pool, m.pool)
            assert torch.equal(m.pool[:3 * N], plain[:3 * N]) and torch.equal(m.pool[-N:], plain[-N:])
            flow = m.pool[3 * N:-N]
            print("flow planes: min", int(flow.min()), "max", int(flow.max()), "mean", float(flow.float().mean()))
            assert int(flow.max()) > int(flow.min())                                     # images, not one constant
            assert m.flow_counts == {"pairs": pairs, "planes": len(m.flow_keys), "files": 0} and len(m.flow_keys) == 50
            assert f.flow_counts is None and f.flow_keys == []
    # one pass over both sets, as fill_all runs it, gives the same pools and counts both videos
    from egaze_amd.data.resident import ResidentSTDataset, fill_all
    both = tuple(ResidentSTDataset(*st_args(dict(tree, flowPath=never), train), raw_u8=True) for train in (True, False))
    fill_all(both, DEV, flow_from=FlowFrom(tree["framePath"], chunk=chunk, params=PARAMS))
    assert all(torch.equal(a.pool, b.pool) for a, b in zip(both, memory))
    assert both[0].flow_counts == both[1].flow_counts == {"pairs": 2 * pairs, "planes": 100, "files": 0}
    assert not os.path.exists(never)


def test_quality_0_stores_flow_to_u8(tree, root):
    from egaze_amd.data import extract_flow as E
    from egaze_amd.data.resident import FlowFrom
    never = str(root / "never_q0")
    sets = _sets(tree, never, flow_from=FlowFrom(tree["framePath"], quality=0, params=PARAMS))
    lossy = _sets(tree, never, flow_from=FlowFrom(tree["framePath"], quality=95, params=PARAMS))
    for ds, jpeg, folder in zip(sets, lossy, (TRAIN, VAL)):
        src = os.path.join(tree["framePath"], folder)
        frames = E.list_frames(src)
        u8 = E.flow_images(E.decode_frames([os.path.join(src, name) for _, name in frames], None, DEV), 20.0, PARAMS)
        assert u8.shape == (2, 29, 44, 60) and len(ds.flow_keys) == 50
        for path, plane in ds.flow_keys:
            _, c, n = E.flow_key(path)
            assert torch.equal(ds.pool[plane], u8[c, n - 1]), (path, plane)
        assert not torch.equal(ds.pool, jpeg.pool) and torch.equal(ds.pool[:3 * N], jpeg.pool[:3 * N])
    assert not os.path.exists(never)


def test_refusals(tree, root):
    from egaze_amd.data import extract_flow as E
    from egaze_amd.data.resident import FlowFrom, ResidentSTDataset
    ds = ResidentSTDataset(*st_args(tree, True), raw_u8=True)
    ds.flow_from = FlowFrom(tree["framePath"])
    ds.plan()
    with pytest.raises(RuntimeError, match="has not run"):
        E.flows_into([ds], tree["framePath"], DEV)
    with pytest.raises(RuntimeError, match=rf"{ds.needed_bytes} bytes.* 1 bytes are allowed"):
        ds.fill(DEV, budget_bytes=1, flow_from=FlowFrom(tree["framePath"]))
    assert ds.pool is None


def test_gaze_full_writes_the_file_paths_checkpoint_and_no_flow_folder(root, monkeypatch):
    """--train_sp for one epoch on an 11 + 5-sample tree of 224 x 224 frames, TV-L1 at extract_flow's defaults."""
    from egaze_amd import gaze_full
    from egaze_amd.data import extract_flow as E
    monkeypatch.setattr(gaze_full, "_at_stage", lambda *a, **kw: None)        # the SP stage is what is compared
    monkeypatch.setattr(gaze_full, "_lf_stage", lambda *a, **kw: None)
    tree = flow_tree(root / "tree224", frames=21, hw=(224, 224),
                     samples={TRAIN: list(range(10, 21)), VAL: list(range(10, 15))})
    empty = str(root / "streams.pth.tar")
    torch.save({'state_dict': {}}, empty)
    flow_files = str(root / "flow224")
    assert E.main(["--framePath", tree["framePath"], "--flowPath", flow_files]) == 2 * 2 * 20
    out = {}
    for mode, flags in (("files", ["--flowPath", flow_files]),
                        ("memory", ["--flow_handover", "--framePath", tree["framePath"], "--flowPath", tree["flowPath"]])):
        d = root / f"main_{mode}"
        argv = ["--train_sp", "--gpu_resident", "--num_epoch", "1", "--batch_size_sp", "4", "--lr", "1e-4", "--sp_resume", "1",
                "--pretrained_spatial", empty, "--pretrained_temporal", empty, "--save_path", str(d), "--device", "0"]
        for k in ("imagePath", "gtPath", "fixsacPath"):
            argv += ["--" + k, tree[k]]
        torch.manual_seed(11)
        gaze_full.main(argv + flags)
        out[mode] = torch.load(str(d / "best_SP.pth.tar"), map_location='cpu', weights_only=False)
    assert not os.path.exists(tree["flowPath"])                                # --flowPath was a key, never a folder
    a, b = out["files"], out["memory"]
    assert repr((a['epoch'], a['auc'], a['aae'])) == repr((b['epoch'], b['auc'], b['aae']))
    assert list(a['state_dict']) == list(b['state_dict']) and len(a['state_dict']) > 20
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
