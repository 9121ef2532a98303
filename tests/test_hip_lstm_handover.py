"""The in-memory SP -> AT hand-over on the GPU: egz_lstm_store (hipops.lstm_store) against its numpy restatement
(lstm_store_ref) exactly -- every window at every border, the channel loop's tail, the planes on which another summation order
picks another gaze cell, the skips and refusals -- and extractLSTMw.extractw(into=...), ResidentLSTMDataset.from_st,
AT(lstm_handover=True) and gaze_full --lstm_handover against the existing hand-over through fix_*.pth.tar files: the pools and
plans byte for byte at chunk 1, the LSTM epochs and the whole run's checkpoints bit for bit, no file written."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import lstm_store_ref as R
from test_late_handover_host import st_args
from test_lstm_handover_host import lstm_tree, written_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def H():
    from egaze_amd import hipops
    return hipops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the kernel against the restatement
@pytest.fixture(scope="module")
def peaks():
    """196 planes, plane i with its peak in cell i over low noise; their gaze cells by the restatement, computed once."""
    rs = np.random.RandomState(0)
    planes = rs.randint(0, 60, (196, 224, 224)).astype(np.uint8)
    for i in range(196):
        y, x = 16 * (i // 14), 16 * (i % 14)
        planes[i, y:y + 16, x:x + 16] = rs.randint(150, 256, (16, 16))
    cells = np.array([R.gaze_cell(p) for p in planes])
    assert cells.tolist() == list(range(196))
    feat = rs.standard_normal((196, 14, 14, 8)).astype(np.float32)
    return planes, torch.from_numpy(planes).to(DEV), feat, torch.from_numpy(feat).to(DEV)


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5])
def test_every_window_at_every_border(peaks, size):
    planes, planes_d, feat, feat_d = peaks
    rs = np.random.RandomState(size)
    gt_src = rs.permutation(196)                          # sample b takes plane gt_src[b] ...
    dst = rs.permutation(230)[:196]                       # ... and writes row dst[b] of a pool with 34 rows nobody names
    pool = torch.full((230, 8), float("nan"), device=DEV)
    before = _bits(pool).clone()
    out, cells = H().lstm_store(feat_d, planes_d, torch.from_numpy(gt_src).to(DEV), pool, torch.from_numpy(dst), size,
                                want_cells=True)
    assert out is pool
    assert cells.cpu().tolist() == gt_src.tolist()        # plane i peaks in cell i
    want, want_cells = R.store_rows(feat, planes, gt_src, dst, size)
    assert want_cells.tolist() == gt_src.tolist() and sorted(want) == sorted(dst.tolist())
    got = _bits(pool)
    for row, v in want.items():
        assert np.array_equal(got[row].numpy(), v.view(np.int32)), (size, row)
    free = sorted(set(range(230)) - set(dst.tolist()))
    assert torch.equal(got[free], before[free])           # rows not named: the same NaN, bit for bit
    # ... and egz_window_mean on the same features and windows
    wins = [R.window(int(c), size, 14) for c in gt_src]
    assert len({(w[1] - w[0], w[3] - w[2]) for w in wins}) >= 1 + size % 2      # an odd size: the low border's window is a cell smaller
    ref = H().window_mean(feat_d, wins)
    assert torch.equal(_bits(ref), got[torch.from_numpy(dst)])


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("C", [1, 5, 256, 257, 512])
def test_channel_tail_and_batch(peaks, B, C):
    planes, planes_d, _, _ = peaks
    rs = np.random.RandomState(C + B)
    feat = rs.standard_normal((B, 14, 14, C)).astype(np.float32)
    gt_src = rs.permutation(196)[:B]
    dst = np.arange(B)[::-1].copy()
    pool = torch.full((B + 1, C), float("nan"), device=DEV)
    H().lstm_store(torch.from_numpy(feat).to(DEV), planes_d, torch.from_numpy(gt_src).to(DEV), pool,
                   torch.from_numpy(dst).to(DEV), 3)      # (a device dst: read back for the duplicate check)
    want, _ = R.store_rows(feat, planes, gt_src, dst, 3)
    got = _bits(pool)
    for row, v in want.items():
        assert np.array_equal(got[row].numpy(), v.view(np.int32)), (B, C, row)
    assert bool(torch.isnan(pool[B]).all())
    ref = H().window_mean(torch.from_numpy(feat).to(DEV), [R.window(int(c), 3, 14) for c in gt_src])
    assert torch.equal(_bits(ref), got[torch.from_numpy(dst)])


def test_tie_planes_follow_torchs_summation_order():
    """test_lstm_handover_host's blob set: cells that tie in their exact sums.  The restatement equals torch's CPU avg_pool2d
    there (checked on the host); the kernel must equal the restatement on every plane."""
    blobs = R.corner_blobs(120, seed=1)
    want = np.array([R.gaze_cell(p) for p in blobs])
    assert sum(R.integer_sum_cell(p) != c for p, c in zip(blobs, want)) * 3 >= len(blobs)
    pool = torch.zeros((120, 1), device=DEV)
    _, cells = H().lstm_store(torch.ones((120, 14, 14, 1), device=DEV), torch.from_numpy(blobs).to(DEV),
                              torch.arange(120, device=DEV), pool, torch.arange(120), 3, want_cells=True)
    wrong = np.nonzero(cells.cpu().numpy() != want)[0]
    print(f"\ntie planes: {len(wrong)} of 120 cells differ from the restatement")
    assert len(wrong) == 0, wrong[:10]
    assert bool((pool == 1).all())                        # the mean of ones
    zero = torch.zeros((1, 224, 224), dtype=torch.uint8, device=DEV)          # an all-zero plane: cell 0
    _, cells = H().lstm_store(torch.ones((1, 14, 14, 1), device=DEV), zero, torch.zeros(1, dtype=torch.int64, device=DEV),
                              pool, torch.zeros(1, dtype=torch.int64), 3, want_cells=True)
    assert cells.tolist() == [0]


# ----------------------------------------------------------------------------- skips and refusals
def test_skips_and_out_of_range_numbers(peaks):
    _, planes_d, _, feat_d = peaks
    h = H()
    pool = torch.full((4, 8), float("nan"), device=DEV)
    before = _bits(pool).clone()
    far = 1 << 40
    # a skipped sample reads nothing: its gt_src would be out of range and raises no bit
    out, cells = h.lstm_store(feat_d[:2], planes_d, torch.tensor([far, -far], device=DEV), pool, torch.tensor([-1, -1]), 3,
                              want_cells=True)
    assert cells.tolist() == [-1, -1] and torch.equal(_bits(pool), before)
    for gt_src, dst in (([196, 0], [0, -1]), ([-1, 0], [1, -1]), ([far, 0], [2, -1]), ([0, 0], [4, -1]), ([0, 0], [-2, -1]),
                        ([0, 0], [far, -1]), ([196, -1], [0, 1])):
        with pytest.raises(RuntimeError, match="outside its pool"):
            h.lstm_store(feat_d[:2], planes_d, torch.tensor(gt_src, device=DEV), pool, torch.tensor(dst), 3)
        assert torch.equal(_bits(pool), before), (gt_src, dst)          # the whole pool is unchanged
    status = {}
    h.lstm_store(feat_d[:2], planes_d, torch.tensor([196, 5], device=DEV), pool, torch.tensor([0, 1]), 3, status_to=status)
    word = h.lstm_store_status(status['_lstm_store_status'])
    assert word == 1                                      # left for the caller: nothing raised in the call
    with pytest.raises(RuntimeError, match="chunk 7.*outside its pool"):
        h.check_lstm_store_status(word, who="chunk 7")
    h.check_lstm_store_status(0)
    got = _bits(pool)
    assert torch.equal(got[[0, 2, 3]], before[[0, 2, 3]]) and not bool(torch.isnan(pool[1]).any())      # the good sample was stored


def test_wrapper_refusals(peaks):
    _, planes_d, _, feat_d = peaks
    h = H()
    f, src, pool, dst = feat_d[:2], torch.tensor([0, 1], device=DEV), torch.zeros((4, 8), device=DEV), torch.tensor([0, 1])
    bad = [
        (dict(dst=torch.tensor([2, 2])), "names row 2 twice"),
        (dict(dst=torch.tensor([2, 2], device=DEV)), "names row 2 twice"),
        (dict(feat_nhwc=torch.zeros((2, 14, 13, 8), device=DEV)), "H == W"),
        (dict(gt_pool=planes_d[:, :208]), r"planes of \(208, 224\)"),
        (dict(gt_pool=planes_d[:, :, :208].contiguous()), r"planes of \(224, 208\)"),
        (dict(cell=8), r"needs \(112, 112\)"),
        (dict(pool=torch.zeros((4, 9), device=DEV)), "C = 8"),
        (dict(feat_nhwc=f.double()), "float32"),
        (dict(gt_pool=planes_d.float()), "uint8"),
        (dict(gt_src=src.int()), "int64"),
        (dict(pool=pool.double()), "float32"),
        (dict(dst=dst.int()), "int64"),
        (dict(dst=torch.tensor([0])), r"\(2,\)"),
        (dict(feat_nhwc=f.cpu()), "no CPU path"),
        (dict(gt_src=src.cpu()), "device"),
        (dict(pool=pool.cpu()), "device"),
        (dict(gt_pool=planes_d.cpu()), "device"),
        (dict(feat_nhwc=feat_d[:4:2]), "contiguous"),
        (dict(pool=torch.zeros((4, 16), device=DEV)[:, :8]), "contiguous"),
        (dict(size=0), "size"), (dict(size=15), "size"), (dict(size=3.0), "size"), (dict(cell=0), "cell"),
        (dict(gt_src=None), "must be a tensor"),
    ]
    for change, message in bad:
        args = dict(feat_nhwc=f, gt_pool=planes_d, gt_src=src, pool=pool, dst=dst, size=3)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            h.lstm_store(**args)
    assert bool((pool == 0).all())                        # refused before any launch


def test_raw_entry_messages_come_back_through_check(peaks):
    from egaze_amd._lib import EgazeHipError
    _, planes_d, _, feat_d = peaks
    h = H()
    src, dst = torch.tensor([0], device=DEV), torch.tensor([0], device=DEV)
    pool, status = torch.zeros((1, 8), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(**change):
        a = dict(feat=feat_d.data_ptr(), B=1, H=14, W=14, C=8, gt_pool=planes_d.data_ptr(), Q=196, gt_src=src.data_ptr(), cell=16,
                 size=3, pool=pool.data_ptr(), rows=1, dst=dst.data_ptr(), cells=None, status=status.data_ptr())
        a.update(change)
        h.check(h.LIB.egz_lstm_store(*a.values(), h._stream()), "egz_lstm_store")

    for change, message in ((dict(feat=None), "feat is null"), (dict(gt_src=None), "gt_pool / gt_src is null"),
                            (dict(pool=None), "pool / dst is null"), (dict(status=None), "status is null"),
                            (dict(B=0), r"B = 0 outside 1 \.\. 65535"), (dict(W=13), "14 x 13 map"),
                            (dict(size=0), r"size = 0 outside 1 \.\. H = 14"), (dict(size=15), r"size = 15 outside 1 \.\. H = 14"),
                            (dict(cell=0), "cell = 0"), (dict(C=0), "C = 0"), (dict(rows=0), "rows = 0"), (dict(Q=0), "Q = 0")):
        with pytest.raises(EgazeHipError, match=message):
            call(**change)
    call()                                                # ... and the same arguments untouched launch
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and bool((pool != 0).any())


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("lstm_handover")


@pytest.fixture(scope="module")
def tree(root):
    return lstm_tree(root / "tree")


@pytest.fixture(scope="module")
def sp_checkpoint(root):
    from oracle import synth
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    path = str(root / "best_SP.pth.tar")
    torch.save({'state_dict': synth.synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1,
                                                     head_gain=0.25)}, path)
    return path


@pytest.fixture(scope="module")
def encoder(sp_checkpoint):
    """features_s alone, as extract_LSTM_training_data builds it."""
    from egaze_amd.utils import cfg, make_layers
    model = make_layers(cfg['D'], 3)
    sd = torch.load(sp_checkpoint, map_location='cpu', weights_only=False)['state_dict']
    own = model.state_dict()
    own.update({k[len('features_s.'):]: v for k, v in sd.items() if k.startswith('features_s.')})
    model.load_state_dict(own)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def st_sets(tree):
    """(training, validation) ResidentSTDatasets, filled once; no test may change their pools."""
    from egaze_amd.data.resident import ResidentSTDataset
    return tuple(ResidentSTDataset(*st_args(tree, train), raw_u8=True).fill(DEV) for train in (True, False))


def _loader(ds):
    return DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=getattr(ds, 'collate_fn', None))


@pytest.fixture(scope="module")
def file_sets(st_sets, encoder, root):
    """The existing hand-over: extractw through files, then ResidentLSTMDataset(folder).fill()."""
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.extractLSTMw import extractw
    sets = []
    for st, sub, train in zip(st_sets, ("train", "test"), (True, False)):
        folder = str(root / "512w" / sub)
        extractw(_loader(st), encoder, folder, 3, DEV)
        assert sorted(os.listdir(folder)) == sorted(written_names(train))
        sets.append(ResidentLSTMDataset(folder).fill(DEV))
    return tuple(sets)


def _memory_set(st, encoder, chunk):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.extractLSTMw import extractw
    into = ResidentLSTMDataset.from_st(st).allocate(DEV)
    assert not into.filled and bool((into.pool == 0).all())
    with pytest.raises(RuntimeError, match="not been completed"):
        into[0]
    extractw(_loader(st), encoder, None, 3, DEV, into=into, chunk=chunk)
    assert into.filled
    return into


def test_chunk_1_equals_the_files_byte_for_byte(st_sets, encoder, file_sets, root, monkeypatch):
    import egaze_amd.extractLSTMw as ex
    st_before = [s.pool.clone() for s in st_sets]
    listing = sorted(os.listdir(str(root)))
    saves, reads, waits, syncs = [], [], [], []
    inner_status, inner_wait, inner_sync = H().lstm_store_status, torch.cuda.Event.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch, "save", lambda *a, **kw: saves.append(a))
    monkeypatch.setattr(H(), "lstm_store_status", lambda p: reads.append(1) or inner_status(p))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: waits.append(1) or inner_wait(self))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: syncs.append(1) or inner_sync(*a))
    for st, files, F in zip(st_sets, file_sets, (6, 4)):
        del reads[:], waits[:], syncs[:]
        into = _memory_set(st, encoder, 1)
        print(f"\n{F} vectors at chunk 1: {len(reads)} status read-back(s), {len(waits)} event wait(s), "
              f"{len(syncs)} device synchronisation(s), {len(saves)} torch.save call(s)")
        assert len(reads) == 1 and len(waits) == 1 and syncs == [] and saves == []
        assert into.pool.shape == files.pool.shape == (F, 512) and into.pool.dtype == torch.float32
        assert torch.equal(_bits(into.pool), _bits(files.pool))
        assert bool(into.pool.abs().sum() > 0) and len({tuple(r) for r in _bits(into.pool).tolist()}) == F     # F different vectors
        assert into.listFiles == files.listFiles and into.n_steps == files.n_steps == F - 2
        assert into.needed_bytes == files.needed_bytes
        for a, b in zip(into.plan, files.plan):
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
        sample, want = into[1], files[1]                  # lstmDataset's dict from pool rows
        assert torch.equal(sample['input'], want['input']) and torch.equal(sample['gt'], want['gt']) and sample['same'] == want['same']
    assert file_sets[0].plan[2].tolist() == [1, 0, 1, 0]  # a state reset inside the training plan
    assert sorted(os.listdir(str(root))) == listing       # no file, no folder
    for s, before in zip(st_sets, st_before):
        assert torch.equal(s.pool, before)                # the ST pool is unchanged
    assert ex.extractw.__defaults__[-1] == 1              # chunk 1 is the default


@pytest.mark.parametrize("chunk", [4, 64])
def test_larger_chunks_equal_the_batched_composition(st_sets, encoder, chunk):
    """chunk 4: two chunks of the training set, the last partial; 64: one chunk holding every vector.  The reference is the
    same batches through existing ops: model(batch) -> to_nhwc -> hipops.window_mean with host windows from gt.cpu()."""
    from egaze_amd.extractLSTMw import var_window
    from egaze_amd.functions import to_nhwc
    for st in st_sets:
        into = _memory_set(st, encoder, chunk)
        frames = sorted(into.st_index.tolist())
        row_of = {i: r for r, i in enumerate(into.st_index.tolist())}
        for k0 in range(0, len(frames), chunk):
            idx = torch.tensor(frames[k0:k0 + chunk], device=DEV)
            image, _, gt = H().resident_gather(st.pool, st.table, idx, fields=('image', 'gt'))
            with torch.no_grad():
                feat = encoder(image)
            pooled = torch.nn.functional.avg_pool2d(gt.cpu().float(), 16)
            cells = torch.max(pooled.view(pooled.size(0), -1), 1)[1].tolist()
            want = H().window_mean(to_nhwc(feat), [var_window(c, 3, 14, 14) for c in cells])
            rows = torch.tensor([row_of[i] for i in frames[k0:k0 + chunk]], device=DEV)
            assert torch.equal(_bits(into.pool[rows]), _bits(want)), (chunk, k0)


def _bare_at(seed=5):
    from egaze_amd.AT import AT
    from egaze_amd.functions import MSELoss
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.optim import FusedAdam
    torch.manual_seed(seed)
    at = AT.__new__(AT)
    at.lstm, at.criterion_lstm, at.device = lstmnet().to(DEV), MSELoss.apply, torch.device(DEV)
    at.optimizer_lstm = FusedAdam(at.lstm.parameters(), lr=1e-4)
    return at


def test_lstm_epochs_are_bit_identical(st_sets, encoder, file_sets):
    memory = tuple(_memory_set(st, encoder, 1) for st in st_sets)
    res = {}
    for name, sets in (("files", file_sets), ("memory", memory)):
        at = _bare_at()
        at.lstmTrainLoader, at.lstmValLoader = DataLoader(sets[0], batch_size=1), DataLoader(sets[1], batch_size=1)
        losses = [at.trainLSTM(), at.trainLSTM(), at.testLSTM()]
        torch.cuda.synchronize()
        res[name] = (losses, [p.detach().clone() for p in at.lstm.parameters()], at.optimizer_lstm.flat_m.clone(),
                     at.optimizer_lstm.flat_v.clone(), at.optimizer_lstm.step_count)
    a, b = res["files"], res["memory"]
    print("\nlosses, files:", a[0], "memory:", b[0])
    assert a[0] == b[0] and all(np.isfinite(a[0])) and a[0][0] != a[0][1] and a[4] == b[4] == 8
    assert all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and bool(a[2].abs().sum() > 0)


def test_gaze_full_writes_the_file_paths_checkpoint_and_no_folder(tree, sp_checkpoint, root, monkeypatch):
    from egaze_amd import gaze_full
    monkeypatch.setattr(gaze_full, "_lf_stage", lambda *a, **kw: None)        # the AT stage is what is compared
    out = {}
    for mode, flags in (("files", []), ("memory", ["--lstm_handover"])):
        d = root / f"main_{mode}"
        d.mkdir()
        argv = ["--gpu_resident", "--extract_lstm", "--train_lstm", "--num_epoch_lstm", "2", "--pretrained_model", sp_checkpoint,
                "--extract_lstm_path", str(d / "512w"), "--save_path", str(d), "--device", "0"]
        for k, v in tree.items():
            argv += ["--" + k, v]
        torch.manual_seed(11)
        gaze_full.main(argv + flags)
        out[mode] = {n: torch.load(str(d / n), map_location='cpu', weights_only=False)
                     for n in ("best_lstm.pth.tar", "valbest_lstm.pth.tar")}
        assert os.path.isdir(str(d / "512w")) == (mode == "files")
    for name, a in out["files"].items():
        b = out["memory"][name]
        assert list(a) == list(b) and len(a) == 10
        assert all(torch.equal(a[k], b[k]) for k in a), name


def test_refusals(st_sets, encoder, tree):
    from egaze_amd.data.STdatas import STDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.extractLSTMw import extractw
    st = st_sets[1]
    into = ResidentLSTMDataset.from_st(st).allocate(DEV)
    with pytest.raises(ValueError, match="shard"):
        extractw(_loader(st), encoder, None, 3, DEV, into=into, shard=(0, 1))
    with pytest.raises(ValueError, match="align"):
        extractw(_loader(st), encoder, None, 3, DEV, align=True, into=into)
    with pytest.raises(ValueError, match="ResidentSTDataset"):              # a file-backed dataset
        extractw(_loader(STDataset(*st_args(tree, False), raw_u8=True)), encoder, None, 3, DEV, into=into)
    with pytest.raises(ValueError, match="not been filled"):
        extractw(_loader(ResidentSTDataset(*st_args(tree, False), raw_u8=True)), encoder, None, 3, DEV, into=into)
    with pytest.raises(ValueError, match="allocate"):
        extractw(_loader(st), encoder, None, 3, DEV, into=ResidentLSTMDataset.from_st(st))
    with pytest.raises(ValueError, match="not planned from this"):
        extractw(_loader(st_sets[0]), encoder, None, 3, DEV, into=into)
    with pytest.raises(ValueError, match="from_st"):
        extractw(_loader(st), encoder, None, 3, DEV, into=object())
    with pytest.raises(ValueError, match="chunk"):
        extractw(_loader(st), encoder, None, 3, DEV, into=into, chunk=0)
    with pytest.raises(ValueError, match="savepath"):
        extractw(_loader(st), encoder, None, 3, DEV)
    assert not into.filled and bool((into.pool == 0).all())                 # refused before any launch
    from egaze_amd.AT import AT
    for kwargs, message in ((dict(extract_lstm=False), "extract_lstm"), (dict(shard=(0, 1)), "one process"),
                            (dict(align=True), "align"), (dict(traindata=object()), "ResidentSTDataset")):
        args = dict(pretrained_model="unused", extract_lstm=True, traindata=st_sets[0], valdata=st_sets[1], lstm_handover=True)
        args.update(kwargs)
        with pytest.raises(ValueError, match=message):
            AT(**args)
    done = _memory_set(st, encoder, 64)
    assert done[0]['input'].shape == (512,)
    done.release()
    assert not done.filled and done.pool is None
    with pytest.raises(RuntimeError, match="hand-over"):
        done[0]
    with pytest.raises(RuntimeError, match="from_st"):
        done.fill(DEV)
