"""The resident late-fusion dataset on the GPU: the fill against imread, its reports of bad files, the staging pipeline against
the file loader (the same tensors in the same batches), LF training on the resident set against LF on the files (identical
parameters, metrics and checkpoints), and gaze_full's LF stage with --late_resident."""
import os
import types

import numpy as np
import pytest
import torch

from test_late_resident_host import late_args, late_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TRAIN, N_VAL = 14, 5


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """The same 14 + 5 frames at 224 x 224 written once as PNGs and once as grey baseline JPEGs."""
    return {ext: late_tree(tmp_path_factory.mktemp("late_" + ext), ext, N_TRAIN, N_VAL) for ext in ("png", "jpg")}


# ----------------------------------------------------------------------------- fill
@pytest.mark.parametrize("ext", ["png", "jpg"])
@pytest.mark.parametrize("decode", ["host", "gpu"])
def test_fill_every_plane_equals_imread(trees, ext, decode, capsys):
    from egaze_amd.data._io import imread
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.STdatas import sniff
    ds = ResidentLateDataset(*late_args(trees[ext]), decode=decode)
    ds.fill(DEV, chunk=17)                                # several chunks, the staging buffer reused
    out = capsys.readouterr().out
    assert f"{3 * N_TRAIN} files decoded ({decode})" in out and str(ds.needed_bytes) in out
    pool = ds.pool.cpu().numpy()
    assert pool.shape == (3 * N_TRAIN, 224, 224) and torch.equal(ds.table.cpu(), ds.plane_table)
    for path, plane, channels in ds.files:
        assert np.array_equal(pool[plane], imread(path, gray=True)), path
    # what the GPU decoder is asked to take: the grey JPEGs, none of the PNGs
    takes = [sniff(open(path, "rb").read()) is not None for path, _, _ in ds.files]
    assert all(takes) if ext == "jpg" else not any(takes)


def test_fill_reports_bad_files(tmp_path):
    from PIL import Image
    from egaze_amd.data.late_resident import ResidentLateDataset
    folders = late_tree(tmp_path, "jpg", 4, 1)
    args = late_args(folders)
    feat = os.path.join(args[2], args[5][1])
    data = open(feat, "rb").read()
    with open(feat, "wb") as f:                           # corrupt data: a warning that names the file
        f.write(data[: len(data) // 2])
    with pytest.warns(RuntimeWarning, match=os.path.basename(feat)):
        ResidentLateDataset(*args, decode="gpu").fill(DEV)
    with open(feat, "wb") as f:
        f.write(data)
    gt = os.path.join(args[1], args[4][2])
    keep = open(gt, "rb").read()
    Image.fromarray(np.zeros((223, 225), dtype=np.uint8)).save(gt)      # wrongly sized
    for decode in ("host", "gpu"):
        with pytest.raises(RuntimeError, match=os.path.basename(gt)):
            ResidentLateDataset(*args, decode=decode).fill(DEV)
    with open(gt, "wb") as f:                             # not an image at all
        f.write(b"no image")
    for decode in ("host", "gpu"):
        with pytest.raises(RuntimeError, match=os.path.basename(gt)):
            ResidentLateDataset(*args, decode=decode).fill(DEV)
    with open(gt, "wb") as f:
        f.write(keep)
    pred = os.path.join(args[0], args[3][3])
    os.remove(pred)                                       # unreadable
    for decode in ("host", "gpu"):
        with pytest.raises(RuntimeError, match=os.path.basename(pred)):
            ResidentLateDataset(*args, decode=decode).fill(DEV)


def test_gather_needs_the_pool_on_the_batchs_device(trees):
    from egaze_amd.data.late_resident import ResidentLateDataset
    ds = ResidentLateDataset(*late_args(trees["png"], train=False)).fill(DEV)
    sample = ds.collate_fn([ds[0], ds[4]])
    with pytest.raises(RuntimeError, match="the pool is on"):
        ds.gather(sample, "cpu")
    raw = ds.gather(sample, DEV, raw=True)
    assert torch.equal(raw, ds.pool[ds.table[sample["index"].to(DEV)]])


# ----------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("ext,decode", [("png", "host"), ("jpg", "gpu")])
def test_staged_batches_identical_to_the_file_loader(trees, ext, decode):
    from torch.utils.data import DataLoader
    from egaze_amd.LF import _stage_late, _stage_late_resident
    from egaze_amd.data.lateDataset import lateDataset
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.STdatas import staged_batches
    args = late_args(trees[ext])
    host, res = lateDataset(*args), ResidentLateDataset(*args, decode=decode).fill(DEV)
    dev = torch.device(DEV)
    for seed in (4, 9):
        got = {}
        for name, ds, stage in (("host", host, _stage_late), ("resident", res, _stage_late_resident)):
            torch.manual_seed(seed)
            loader = DataLoader(ds, batch_size=4, shuffle=True, num_workers=0, pin_memory=True,
                                collate_fn=getattr(ds, "collate_fn", None))
            got[name] = [[t.clone() for t in staged] for _ in range(2) for _, staged in staged_batches(loader, dev, stage)]
            torch.cuda.synchronize()
        assert len(got["host"]) == len(got["resident"]) == 8
        assert [b[0].shape[0] for b in got["resident"]] == [4, 4, 4, 2] * 2             # a trailing partial batch
        for (im, gt, feat), (fused, gt_r) in zip(got["host"], got["resident"]):
            assert fused.dtype == gt_r.dtype == torch.float32
            assert torch.equal(feat, fused[:, 0:1]) and torch.equal(im, fused[:, 1:2]) and torch.equal(gt, gt_r)
        assert not torch.equal(got["host"][0][0], got["host"][4][0])                    # the epochs are shuffled apart


def _train(folders, save, resident, decode="host"):
    """LF(...).train() for 2 epochs from seed 0 -> (parameters, buffers, per-epoch (loss, auc, aae), the two checkpoints)."""
    from egaze_amd.LF import LF
    os.makedirs(save, exist_ok=True)
    torch.manual_seed(0)
    lf = LF(save_path=save, device='0', late_pred_path=folders[0], late_feat_path=folders[1], gt_path=folders[2],
            num_epoch=2, val_name='Alireza', batch_size=4, lr=1e-4, resident=resident, decode=decode)
    epochs = []
    for name in ("trainLate", "testLate"):
        inner = getattr(lf, name)
        setattr(lf, name, lambda inner=inner, name=name: epochs.append((name,) + tuple(inner())) or epochs[-1][1:])
    lf.train()
    torch.cuda.synchronize()
    cks = [torch.load(os.path.join(save, n), map_location='cpu', weights_only=False)
           for n in ("best_late.pth.tar", "valbest_late.pth.tar")]
    return lf, ([p.detach().cpu() for p in lf.model.parameters()], [b.detach().cpu() for b in lf.model.buffers()], epochs, cks)


@pytest.mark.parametrize("graphed", [True, False])
def test_training_identical_on_files_and_resident(trees, tmp_path, graphed, monkeypatch):
    from egaze_amd import LF as lf_mod
    from egaze_amd import hipops as Hp
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.lateDataset import lateDataset
    monkeypatch.setattr(lf_mod, "LF_GRAPH", graphed)
    cat2 = []
    inner = Hp.cat2_planes
    monkeypatch.setattr(Hp, "cat2_planes", lambda *a, **kw: cat2.append(1) or inner(*a, **kw))
    lf_h, host = _train(trees["jpg"], str(tmp_path / "host"), False)
    assert isinstance(lf_h.train_loader.dataset, lateDataset) and not isinstance(lf_h.train_loader.dataset, ResidentLateDataset)
    n_host = len(cat2)
    assert n_host > 0
    lf_r, res = _train(trees["jpg"], str(tmp_path / "resident"), True, decode="gpu")
    assert len(cat2) == n_host                            # no cat2_planes launch is left in the resident iteration
    for loader, n in ((lf_r.train_loader, N_TRAIN), (lf_r.val_loader, N_VAL)):
        ds = loader.dataset
        assert isinstance(ds, ResidentLateDataset) and ds.decode == "gpu" and ds.pool.shape == (3 * n, 224, 224)
        assert loader.num_workers == 0 and loader.collate_fn == ds.collate_fn
    assert len(host[0]) == len(res[0]) == 14 and all(torch.equal(p, q) for p, q in zip(host[0], res[0]))
    assert len(host[1]) == len(res[1]) > 0 and all(torch.equal(p, q) for p, q in zip(host[1], res[1]))
    assert len(host[2]) == 4 and [e[0] for e in host[2]] == ["trainLate", "testLate"] * 2
    assert host[2] == res[2]                              # every epoch's loss, AUC and AAE, training and validation
    assert all(np.isfinite(v) for e in host[2] for v in e[1:])
    for ck_h, ck_r in zip(host[3], res[3]):
        assert (ck_h['loss'], ck_h['auc'], ck_h['aae']) == (ck_r['loss'], ck_r['auc'], ck_r['aae'])
        assert list(ck_h['state_dict']) == list(ck_r['state_dict'])
        assert all(torch.equal(ck_h['state_dict'][k], ck_r['state_dict'][k]) for k in ck_h['state_dict'])
    w0 = lf_mod.late_fusion().fusion[0].weight
    assert not torch.equal(host[0][0], w0.detach())


# ----------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("gpu_decode", [False, True])
def test_gaze_full_lf_stage_with_late_resident(trees, tmp_path, gpu_decode, capsys):
    from egaze_amd import gaze_full
    folders = trees["jpg"]
    argv = ["--late_resident", "--train_late", "--num_epoch", "1", "--batch_size", "4", "--save_path", str(tmp_path),
            "--extract_late_pred_folder", folders[0], "--extract_late_feat_folder", folders[1], "--gtPath", folders[2],
            "--gpu_resident_gb", "0.5"] + (["--gpu_decode"] if gpu_decode else [])
    args = gaze_full.build_parser().parse_args(argv)
    # pools of --gpu_resident still held by the ST datasets: released before the LF pools are filled
    st = types.SimpleNamespace(pool=torch.zeros(8, dtype=torch.uint8, device=DEV), table=torch.zeros(1, device=DEV))
    gaze_full._lf_stage(args, (st,))
    assert st.pool is None and st.table is None
    out = capsys.readouterr().out
    mode = "gpu" if gpu_decode else "host"
    assert f"{3 * N_TRAIN} files decoded ({mode})" in out and f"{3 * N_VAL} files decoded ({mode})" in out
    assert "LF module training finished!" in out
    assert os.path.exists(str(tmp_path / "best_late.pth.tar")) and os.path.exists(str(tmp_path / "valbest_late.pth.tar"))
    # the budget is --gpu_resident_gb's, over both sets, refused from the plan alone
    args.gpu_resident_gb = 1e-3
    need = 3 * (N_TRAIN + N_VAL) * 50176 + (N_TRAIN + N_VAL) * 24
    with pytest.raises(RuntimeError, match=rf"--late_resident: .*{need} bytes, 1000000 bytes are allowed"):
        gaze_full._lf_stage(args)
