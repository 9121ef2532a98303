"""The in-memory AT -> LF hand-over on the GPU (AT.extract_late(into=...), LF(datasets=...), gaze_full --late_handover) against
the existing hand-over through files: the pools and tables byte for byte, no file written, the ST pool untouched, one LF epoch
and the whole gaze_full run bit for bit; the refusals.

The file path's feat plane is resized on the host by data._io.resize: cv2.resize where cv2 is installed (the reference's
arithmetic, which linear_u8.h restates and egz_late_store uses), PIL's BILINEAR where it is not.  PIL rounds differently (1 LSB
on about a fifth of the pixels of a 14 x 14 -> 224 x 224 map), so where cv2 is missing the file path of these tests runs with
test_vis_host.resize_linear in resize's place -- the integer restatement of cv2's INTER_LINEAR that test_vis_host checks
against cv2 itself where it can.  The comparison is torch.equal either way."""
import os

import numpy as np
import pytest
import torch

from test_late_handover_host import TRAIN, handover_tree, st_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TRAIN, N_VAL = 11, 5


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("late_handover")


@pytest.fixture(scope="module")
def tree(root):
    return handover_tree(root / "tree", N_TRAIN, N_VAL)


@pytest.fixture(scope="module")
def weights(root):
    """Seeded random SP and LSTM checkpoints, and the folders AT lists for its LSTM loaders."""
    from oracle import synth
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import cfg, make_layers
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    save = root / "save"
    save.mkdir()
    sp, lstm = str(save / "best_SP.pth.tar"), str(save / "best_lstm.pth.tar")
    torch.save({'state_dict': synth.synth_state_dict(shapes(model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))),
                                                     seed=1, head_gain=0.25)}, sp)
    torch.save(synth.synth_state_dict(shapes(lstmnet()), seed=2), lstm)
    for sub in ("train", "test"):
        d = root / "512w" / sub
        d.mkdir(parents=True)
        ins, _ = synth.synth_at_batch(4, 1, seed=1)
        for i in range(4):
            torch.save(ins[i, 0].clone(), str(d / f"fix_{TRAIN}_{i:010d}.pth.tar"))
    return sp, lstm, str(root / "512w"), str(save)


@pytest.fixture(scope="module")
def st_sets(tree):
    """(training, validation) ResidentSTDatasets, filled once; no test may change their pools."""
    from egaze_amd.data.resident import ResidentSTDataset
    sets = tuple(ResidentSTDataset(*st_args(tree, train), raw_u8=True).fill(DEV) for train in (True, False))
    assert [len(s) for s in sets] == [N_TRAIN, N_VAL]
    assert [int(f) for f in sets[0].fixsac] == [1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0]      # runs of both kinds
    return sets


@pytest.fixture(scope="module")
def at(weights):
    from egaze_amd.AT import AT
    sp, lstm, vectors, save = weights
    return AT(pretrained_model=sp, pretrained_lstm=lstm, save_path=save, device='0', lstm_data_path=vectors)


@pytest.fixture(scope="module")
def reference_resize():
    """The file path's host resize in cv2's arithmetic where cv2 itself is missing (see the module docstring)."""
    patch = pytest.MonkeyPatch()
    try:
        import cv2  # noqa: F401
    except ImportError:
        import egaze_amd.AT as at_module
        from test_vis_host import resize_linear
        patch.setattr(at_module, "resize", lambda arr, size: resize_linear(arr, (size[1], size[0])))
    yield
    patch.undo()


def _loader(ds):
    from torch.utils.data import DataLoader
    return DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=ds.collate_fn)


def _file_sets(at, st_sets, tree, out, chunk):
    """The existing hand-over: both passes into folders, then LF's listing of them decoded into resident sets."""
    from egaze_amd.LF import _split
    from egaze_amd.data.late_resident import ResidentLateDataset
    pred, feat = str(out / "pred"), str(out / "feat")
    for st in (st_sets[1], st_sets[0]):
        at.extract_late(_loader(st), pred + "/", feat + "/", chunk=chunk)
    assert len(os.listdir(pred)) == len(os.listdir(feat)) == N_TRAIN + N_VAL
    sets = []
    for k in (0, 1):
        args = (pred, tree["gtPath"], feat, _split(pred, "Alireza", None)[k], _split(tree["gtPath"], "Alireza", None)[k],
                _split(feat, "Alireza", None)[k])
        sets.append(ResidentLateDataset(*args).fill(DEV))
    return tuple(sets)


def _memory_sets(at, st_sets, chunk):
    from egaze_amd.data.late_resident import ResidentLateDataset
    sets = tuple(ResidentLateDataset.from_st(st).allocate(DEV) for st in st_sets)
    for st, into in ((st_sets[1], sets[1]), (st_sets[0], sets[0])):
        assert not into.filled
        with pytest.raises(RuntimeError, match="has not completed"):
            into.gather(into.collate_fn([into[0]]), DEV)
        at.extract_late(_loader(st), "/nonexistent/pred/", "/nonexistent/feat/", chunk=chunk, into=into)
        assert into.filled
    return sets


@pytest.fixture(scope="module")
def handovers(at, st_sets, tree, root, reference_resize):
    """``get(chunk)`` -> (file sets, memory sets) of one chunk size, each (training, validation), computed once; the memory
    pass must leave the test's folder as it found it."""
    done = {}

    def get(chunk):
        if chunk not in done:
            files = _file_sets(at, st_sets, tree, root / f"files{chunk}", chunk)
            listing = sorted(os.listdir(str(root)))
            memory = _memory_sets(at, st_sets, chunk)
            assert sorted(os.listdir(str(root))) == listing and not os.path.exists("/nonexistent")      # no file, no folder
            done[chunk] = (files, memory)
        return done[chunk]
    return get


@pytest.mark.parametrize("chunk", [1, 4, 32])
def test_pools_equal_the_file_hand_overs(handovers, st_sets, chunk):
    """chunk 1: the reference's schedule; 4: three chunks, the last partial, LSTM calls in each with the state carried across;
    32: one chunk per pass."""
    st_before = [s.pool.clone() for s in st_sets]
    files, memory = handovers(chunk)
    for f, m, n in zip(files, memory, (N_TRAIN, N_VAL)):
        assert f.pool.shape == m.pool.shape == (3 * n, 224, 224) and m.pool.dtype == torch.uint8
        assert torch.equal(f.table, m.table) and m.table.device == m.pool.device
        for c, name in enumerate(("pred", "feat", "gt")):
            diff = int((f.pool[c * n:(c + 1) * n] != m.pool[c * n:(c + 1) * n]).sum())
            print(f"chunk {chunk}, {n} frames, {name}: {diff} bytes differ")
            assert diff == 0, (chunk, n, name)
        assert torch.equal(f.pool, m.pool)
        assert int(m.pool[:n].max()) > int(m.pool[:n].min()) and int(m.pool[n:2 * n].max()) > 0     # real maps, not zeros
    for s, before in zip(st_sets, st_before):
        assert torch.equal(s.pool, before)                                                       # the ST pool is unchanged


def test_one_lf_epoch_is_bit_identical(handovers, tree, weights):
    from egaze_amd.LF import LF
    kept = dict(zip(("files", "memory"), handovers(4)))
    res = {}
    for name in ("files", "memory"):
        torch.manual_seed(7)
        lf = LF(save_path=weights[3], device='0', batch_size=4, lr=1e-4, datasets=kept[name], gt_path=tree["gtPath"],
                late_pred_path="/nonexistent/pred", late_feat_path="/nonexistent/feat")
        assert lf.train_loader.dataset is kept[name][0] and lf.val_loader.dataset is kept[name][1]
        out = lf.trainLate()
        val = lf.testLate()
        torch.cuda.synchronize()
        res[name] = (out, val, [p.detach().clone() for p in lf.model.parameters()],
                     [b.detach().clone() for b in lf.model.buffers()], lf.optimizer.flat_m.clone(), lf.optimizer.flat_v.clone())
    a, b = res["files"], res["memory"]
    assert all(np.isfinite(v) for v in a[0]) and a[0] == b[0] and a[1] == b[1]                  # loss, AUC, AAE: equal floats
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and bool(a[4].abs().sum() > 0)
    with pytest.raises(ValueError, match="not complete"):
        LF(save_path=weights[3], device='0', datasets=(_incomplete(kept), kept["memory"][1]))
    with pytest.raises(ValueError, match="ResidentLateDataset"):
        LF(save_path=weights[3], device='0', datasets=(kept["memory"][0], object()))


def _incomplete(kept):
    """A from_st set that has its pool but has not been written."""
    import copy
    ds = copy.copy(kept["memory"][0])
    ds._complete = False
    return ds


def test_gaze_full_writes_the_file_paths_checkpoint_and_no_folder(tree, weights, root, reference_resize):
    from egaze_amd import gaze_full
    sp, lstm, vectors, save = weights
    out = {}
    for mode, flags in (("files", ["--late_resident"]), ("memory", ["--late_handover"])):
        d = root / f"main_{mode}"
        d.mkdir()
        torch.save(torch.load(lstm, weights_only=False), str(d / "best_lstm.pth.tar"))
        argv = ["--gpu_resident", "--extract_late", "--train_late", "--num_epoch", "1", "--batch_size", "4",
                "--lr_late", "1e-4", "--pretrained_model", sp, "--extract_lstm_path", vectors, "--save_path", str(d), "--device", "0",
                "--extract_late_pred_folder", str(d / "pred") + "/", "--extract_late_feat_folder", str(d / "feat") + "/"]
        for k, v in tree.items():
            argv += ["--" + k, v]
        torch.manual_seed(11)
        gaze_full.main(argv + flags)
        out[mode] = {n: torch.load(str(d / n), weights_only=False) for n in ("best_late.pth.tar", "valbest_late.pth.tar")}
        assert os.path.isdir(str(d / "pred")) == os.path.isdir(str(d / "feat")) == (mode == "files")
    for name, a in out["files"].items():
        b = out["memory"][name]
        assert (a['loss'], a['auc'], a['aae']) == (b['loss'], b['auc'], b['aae']) and np.isfinite(a['loss'])
        assert list(a['state_dict']) == list(b['state_dict'])
        assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])


def test_refusals(at, st_sets, tree):
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    st = st_sets[1]
    into = ResidentLateDataset.from_st(st).allocate(DEV)
    before = into.pool.clone()
    host = STDataset(*st_args(tree, False), raw_u8=True)
    with pytest.raises(ValueError, match="ResidentSTDataset"):              # a file-backed dataset
        at.extract_late(_loader(host), into=into)
    with pytest.raises(ValueError, match="shard"):
        at.extract_late(_loader(st), into=into, shard=(0, 1))
    no_gt = ResidentSTDataset(*st_args(tree, False), raw_u8=True)
    no_gt.gpu_fields = ("image", "flow")
    no_gt.fill(DEV)
    with pytest.raises(ValueError, match=r"\['gt'\]"):                       # a resident set without the ground truth
        at.extract_late(_loader(no_gt), into=into)
    with pytest.raises(ValueError, match="not been filled"):
        at.extract_late(_loader(ResidentSTDataset(*st_args(tree, False), raw_u8=True)), into=into)
    with pytest.raises(ValueError, match="allocate"):
        at.extract_late(_loader(st), into=ResidentLateDataset.from_st(st))
    with pytest.raises(ValueError, match="not planned from this"):
        at.extract_late(_loader(st_sets[0]), into=into)
    with pytest.raises(ValueError, match="from_st"):
        at.extract_late(_loader(st), into=object())
    assert not into.filled and torch.equal(into.pool, before)               # refused before any launch
