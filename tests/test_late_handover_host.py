"""Host side of the in-memory AT -> LF hand-over (``gaze_full --late_handover``): ResidentLateDataset.from_st plans the set LF
would list from the hand-over folders, row for row, or refuses; the parser's refusals.  No GPU: nothing touches a device."""
import os
import types

import numpy as np
import pytest
import torch

TRAIN, VAL = "Ahmad_Pizza1", "Alireza_Pizza1"
# STDataset dilates the labels by one frame each side: the training flags become 1 1 0 0 0 0 1 1 1 0 0
RAW_FLAGS = {TRAIN: [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], VAL: [0, 0, 0, 1, 0]}


def handover_tree(root, n_train=11, n_val=5, seed=0):
    """A dataset tree with one training video and one validation video (Alireza's): lossless PNG frames named ``*.png`` (the
    hand-over files take the frames' names, so the existing path writes PNGs), grey JPEG flow with the ten-frame window behind
    every sample, PNG ground-truth blobs, one fixation file per video.  -> the paths as gaze_full's flags name them."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    root = str(root)
    paths = {k: os.path.join(root, d) for k, d in (("flowPath", "flow"), ("imagePath", "img"), ("gtPath", "gt"),
                                                   ("fixsacPath", "fs"))}
    for d in paths.values():
        os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:224, 0:224]

    def smooth(shape):                                    # low-frequency content: 28 x 28 noise, enlarged
        a = rs.randint(0, 256, (28, 28) + shape).astype(np.uint8)
        return np.asarray(Image.fromarray(a.squeeze()).resize((224, 224), Image.BICUBIC))

    for folder, n in ((TRAIN, n_train), (VAL, n_val)):
        os.makedirs(os.path.join(paths["flowPath"], folder), exist_ok=True)
        for num in range(1, 10 + n):
            for ax in "xy":
                name = os.path.join(paths["flowPath"], folder, f"flow_{ax}_{num:05d}.jpg")
                Image.fromarray(smooth(())).save(name, quality=90)
        for num in range(10, 10 + n):
            Image.fromarray(smooth((3,))).save(os.path.join(paths["imagePath"], f"{folder}_img_{num:05d}.png"))
            cy, cx = rs.uniform(40, 180, 2)
            blob = 255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * 18.0 ** 2))
            Image.fromarray(blob.astype(np.uint8)).save(os.path.join(paths["gtPath"], f"{folder}_000000_{num:05d}.png"))
        flags = (RAW_FLAGS[folder] * (n // len(RAW_FLAGS[folder]) + 1))[:n]
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), np.array(flags, dtype=float))
    return paths


def st_args(paths, train=True, val_name="Alireza"):
    """STDataset's positional arguments for one split of the tree, listed as gaze_full.main lists it."""
    from egaze_amd.gaze_full import _split
    k = 0 if train else 1
    return (paths["flowPath"], paths["imagePath"], paths["gtPath"], sorted(os.listdir(paths["flowPath"])),
            _split(paths["imagePath"], val_name)[k], _split(paths["gtPath"], val_name)[k],
            _split(paths["fixsacPath"], val_name)[k], paths["fixsacPath"])


def _fake_st(names, gts, hw=(6, 10)):
    """What from_st reads of a planned ResidentSTDataset."""
    return types.SimpleNamespace(listTrainFiles=list(names), listGtFiles=list(gts), gtPath="gt", hw=hw)


def _names(n, folder=TRAIN):
    return [f"{folder}_img_{k:05d}.png" for k in range(10, 10 + n)], [f"{folder}_000000_{k:05d}.png" for k in range(10, 10 + n)]


@pytest.mark.parametrize("train", [True, False])
def test_from_st_plans_what_plan_builds_from_the_files(tmp_path, train):
    """The hand-over folders hold one file per frame under the frame's name (what extract_late writes); LF's listing of them,
    planned by plan(), gives the table, the names and the bytes from_st gives without looking at them."""
    from PIL import Image
    from egaze_amd.LF import _split
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.resident import ResidentSTDataset
    paths = handover_tree(tmp_path / "tree", n_train=5, n_val=3)
    st = ResidentSTDataset(*st_args(paths, train), raw_u8=True)
    assert list(st.fixsac) == ([1, 1, 0, 0, 0] if train else [0, 0, 0])
    pred, feat = str(tmp_path / "pred"), str(tmp_path / "feat")
    for folder in (pred, feat):
        os.makedirs(folder)
        for name in os.listdir(paths["imagePath"]):       # both videos, as both extraction passes write into one folder
            Image.fromarray(np.zeros((224, 224), np.uint8)).save(os.path.join(folder, name))
    k = 0 if train else 1
    listed = ResidentLateDataset(pred, paths["gtPath"], feat, _split(pred, "Alireza", None)[k],
                                 _split(paths["gtPath"], "Alireza", None)[k], _split(feat, "Alireza", None)[k]).plan()
    ds = ResidentLateDataset.from_st(st)
    N = 5 if train else 3
    assert len(ds) == len(listed) == N and ds.hw == listed.hw == (224, 224) and ds.planes == listed.planes == 3 * N
    assert ds.plane_table.dtype == torch.int64 and torch.equal(ds.plane_table, listed.plane_table)
    assert ds.plane_table.tolist() == [[i, N + i, 2 * N + i] for i in range(N)]
    assert (ds.listFiles, ds.listFeat, ds.listGtFiles) == (listed.listFiles, listed.listFeat, listed.listGtFiles)
    assert ds.gtPath == listed.gtPath and ds.st_index.tolist() == list(range(N))
    assert ds.needed_bytes == listed.needed_bytes == 3 * N * 224 * 224 + N * 3 * 8
    assert ds.pool is None and ds.table is None and not ds.filled and ds.loader_workers == 0
    with pytest.raises(RuntimeError, match="fill"):       # no pool yet: nothing to gather from, nothing to decode
        ds.gather(ds.collate_fn([ds[0]]), "cuda:0")
    with pytest.raises(RuntimeError, match="from_st"):
        ds.fill("cuda:0")
    with pytest.raises(RuntimeError, match=rf"{ds.needed_bytes} bytes.* 1 bytes are allowed"):
        ds.allocate("cuda:0", budget_bytes=1)             # refused before anything is allocated
    assert ds.pool is None and ds.table is None


def test_from_st_with_a_task_keeps_lfs_rows():
    """LF filters the listed names by ``task``; the rows that stay keep their ST sample numbers."""
    from egaze_amd.data.late_resident import ResidentLateDataset
    names = [f"Ahmad_{t}_img_{k:05d}.png" for t, k in (("American1", 10), ("American1", 11), ("Pizza1", 10), ("Pizza1", 12))]
    gts = [f"Ahmad_{t}_000000_{k:05d}.png" for t, k in (("American1", 10), ("American1", 11), ("Pizza1", 10), ("Pizza1", 12))]
    ds = ResidentLateDataset.from_st(_fake_st(names, gts), task="Pizza")
    assert ds.listFiles == names[2:] and ds.listGtFiles == gts[2:] and ds.st_index.tolist() == [2, 3]
    assert ds.plane_table.tolist() == [[0, 2, 4], [1, 3, 5]] and ds.needed_bytes == 6 * 60 + 2 * 3 * 8
    with pytest.raises(RuntimeError, match="no samples"):
        ResidentLateDataset.from_st(_fake_st(names, gts), task="Burger")


def test_from_st_refuses_what_lf_would_list_differently():
    from egaze_amd.data.late_resident import ResidentLateDataset
    names, gts = _names(5)
    assert len(ResidentLateDataset.from_st(_fake_st(names, gts))) == 5
    dup = list(names)
    dup[3] = dup[1]                                       # two frames, one hand-over file
    with pytest.raises(ValueError, match=rf"sample 3 \({dup[3]}\) has the name of sample 1"):
        ResidentLateDataset.from_st(_fake_st(dup, gts))
    swapped = [names[0], names[2], names[1], names[3], names[4]]
    with pytest.raises(ValueError, match=rf"sample 2 \({names[1]}\) sorts before sample 1 \({names[2]}\)"):
        ResidentLateDataset.from_st(_fake_st(swapped, gts))
    paired = [gts[0], gts[1], gts[3], gts[2], gts[4]]     # sorted() would hand sample 2 the map of sample 3
    with pytest.raises(ValueError, match=rf"sample 2 \({names[2]}\) has ground truth {gts[3]}.*{gts[2]}"):
        ResidentLateDataset.from_st(_fake_st(names, paired))
    with pytest.raises(ValueError, match="5 images but 4 ground-truth maps"):
        ResidentLateDataset.from_st(_fake_st(names, gts[:4]))


def test_parser_refusals(monkeypatch, capsys):
    from egaze_amd.gaze_full import build_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    full = ["--gpu_resident", "--extract_late", "--train_late", "--late_handover"]
    ns = build_parser().parse_args(full)
    assert ns.late_handover is True and ns.late_resident is True            # implies --late_resident
    assert not hasattr(build_parser().parse_args([]), "late_handover")      # the reference's namespace without the flag
    assert not hasattr(build_parser().parse_args(full[:3]), "late_resident")
    for drop in ("--gpu_resident", "--extract_late", "--train_late"):
        with pytest.raises(SystemExit) as e:
            build_parser().parse_args([a for a in full if a != drop])
        assert e.value.code == 2 and f"--late_handover needs {drop}" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        build_parser().parse_args(full)
    assert e.value.code == 2 and "one process" in capsys.readouterr().err
    build_parser().parse_args(full[:3])                                     # without the flag WORLD_SIZE is not looked at
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert build_parser().parse_args(full).late_handover
