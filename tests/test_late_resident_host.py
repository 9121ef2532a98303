"""Host side of the resident late-fusion dataset (data/late_resident.py, egz_late_gather's argument checks).  No GPU: plan()
and the refusals touch no device and launch nothing."""
import os

import numpy as np
import pytest
import torch

SUBJECTS = ("Ahmad", "Carlos", "Alireza")
TASKS = ("American", "Pizza")


def late_tree(root, ext="png", n_train=14, n_val=5, hw=(224, 224), seed=0):
    """pred / feat / gt folders of seeded grey maps, written by Pillow (``ext`` 'jpg': baseline grey JPEGs, as the hand-over
    has them with the real dataset's names).  Training frames alternate between two subjects and two tasks, the validation
    frames are Alireza's.  -> (pred, feat, gt) folder paths."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    names = [f"{SUBJECTS[i % 2]}_{TASKS[(i // 2) % 2]}_frame_{i:05d}.{ext}" for i in range(n_train)]
    names += [f"Alireza_{TASKS[i % 2]}_frame_{i:05d}.{ext}" for i in range(n_val)]
    folders = tuple(os.path.join(str(root), d) for d in ("pred", "feat", "gt"))
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    for k, folder in enumerate(folders):
        os.makedirs(folder, exist_ok=True)
        for name in names:
            if k == 2:                                    # a blob, as a gaze map is
                cy, cx = rs.uniform(0.2, 0.8) * hw[0], rs.uniform(0.2, 0.8) * hw[1]
                arr = 255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.08 * max(hw)) ** 2))
            else:
                arr = rs.randint(0, 256, hw)
            Image.fromarray(arr.astype(np.uint8)).save(os.path.join(folder, name))
    return folders


def late_args(folders, val_name="Alireza", task=None, train=True):
    """lateDataset's positional arguments for one split of the tree, listed as LF lists it."""
    from egaze_amd.LF import _split
    pred, feat, gt = folders
    k = 0 if train else 1
    return (pred, gt, feat, _split(pred, val_name, task)[k], _split(gt, val_name, task)[k], _split(feat, val_name, task)[k])


def test_plan_table_files_and_bytes(tmp_path):
    from egaze_amd.data.late_resident import ResidentLateDataset
    folders = late_tree(tmp_path, hw=(6, 10), n_train=6, n_val=3)
    args = late_args(folders)
    ds = ResidentLateDataset(*args)
    assert len(ds) == 6 and ds.loader_workers == 0 and ds.pool is None
    ds.plan()
    assert ds.hw == (6, 10) and ds.planes == 18 and len(ds.files) == 18
    t = ds.plane_table
    assert t.shape == (6, 3) and t.dtype == torch.int64
    assert ds.needed_bytes == 18 * 60 + 6 * 3 * 8
    start = {path: plane for path, plane, channels in ds.files}
    assert sorted(start.values()) == list(range(18)) and all(c == 1 for _, _, c in ds.files)
    for i in range(6):                                    # column order: pred, feat, gt
        want = [os.path.join(args[0], args[3][i]), os.path.join(args[2], args[5][i]), os.path.join(args[1], args[4][i])]
        assert [start[p] for p in want] == t[i].tolist()


def test_plan_gives_a_file_listed_twice_one_plane(tmp_path):
    from egaze_amd.data.late_resident import ResidentLateDataset
    folders = late_tree(tmp_path, hw=(4, 4), n_train=4, n_val=1)
    pred, gt, feat, lp, lg, lf = late_args(folders)
    lp = [lp[0], lp[1], lp[0], lp[3]]                     # sample 2 reads sample 0's prediction
    ds = ResidentLateDataset(pred, gt, feat, lp, lg, lf).plan()
    assert ds.planes == 11 and len(ds.files) == 11
    assert ds.plane_table[2, 0] == ds.plane_table[0, 0]
    assert ds.needed_bytes == 11 * 16 + 4 * 3 * 8
    assert len(set(ds.plane_table.flatten().tolist())) == 11


@pytest.mark.parametrize("val_name,task", [("Alireza", None), ("Carlos", None), ("Alireza", "Pizza"), ("Ahmad", "American")])
def test_splits_are_lfs(tmp_path, val_name, task):
    """The resident set lists what LF._split lists: the same names in the same order, per column."""
    from egaze_amd.LF import _split
    from egaze_amd.data.late_resident import ResidentLateDataset
    folders = late_tree(tmp_path, hw=(4, 4), n_train=8, n_val=4)
    for k, train in ((0, True), (1, False)):
        ds = ResidentLateDataset(*late_args(folders, val_name, task, train)).plan()
        names = _split(folders[0], val_name, task)[k]
        assert len(ds) == len(names) > 0
        by_plane = {plane: path for path, plane, _ in ds.files}
        for c, folder in enumerate(folders):
            assert [by_plane[int(p)] for p in ds.plane_table[:, c]] == [os.path.join(folder, n) for n in names]
        assert all((val_name in n) == (not train) and (task is None or task in n) for n in names)


def test_samples_read_no_file_and_collate_carries_indices(tmp_path):
    from egaze_amd.data.late_resident import ResidentLateDataset
    folders = late_tree(tmp_path, hw=(4, 4), n_train=4, n_val=1)
    ds = ResidentLateDataset(*late_args(folders))
    for folder in folders:
        for f in os.listdir(folder):
            os.remove(os.path.join(folder, f))
    b = ds.collate_fn([ds[3], ds[0], ds[3]])
    assert set(b) == {"resident", "index"} and b["resident"] is ds
    assert b["index"].dtype == torch.int64 and b["index"].tolist() == [3, 0, 3]
    with pytest.raises(RuntimeError, match="fill"):
        ds.gather(b, "cuda:0")


def test_over_budget_is_refused_before_any_allocation(tmp_path):
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.resident import fill_all
    folders = late_tree(tmp_path, hw=(6, 10), n_train=6, n_val=3)
    train = ResidentLateDataset(*late_args(folders)).plan()
    val = ResidentLateDataset(*late_args(folders, train=False)).plan()
    need = (18 * 60 + 6 * 24, 9 * 60 + 3 * 24)
    assert (train.needed_bytes, val.needed_bytes) == need
    with pytest.raises(RuntimeError, match=rf"{sum(need)} bytes, 1 bytes are allowed"):
        fill_all((train, val), "cuda:0", budget_gb=1e-9)
    with pytest.raises(RuntimeError, match=rf"ResidentLateDataset.fill.*{need[0]} bytes.* 1 bytes are allowed"):
        train.fill("cuda:0", budget_bytes=1)
    assert train.pool is None and train.table is None and val.pool is None


def test_fill_all_budgets_a_mix_of_both_kinds(tmp_path):
    from test_resident_host import resident_tree
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.resident import ResidentSTDataset, fill_all
    st = ResidentSTDataset(*resident_tree(tmp_path / "st"), raw_u8=True)
    late = ResidentLateDataset(*late_args(late_tree(tmp_path / "late", hw=(6, 10), n_train=6, n_val=3)))
    need = 60 * 50176 + 7 * 22 * 8 + 18 * 60 + 6 * 24
    with pytest.raises(RuntimeError, match=rf"{need} bytes, 1000 bytes are allowed"):
        fill_all((st, late), "cuda:0", budget_gb=1e-6)
    assert st.pool is None and late.pool is None


def test_parser_keeps_the_37_defaults_and_the_flag_is_absent_unless_given():
    from egaze_amd.gaze_full import build_parser
    ns = build_parser().parse_args([])
    assert len(vars(ns)) == 37 and not hasattr(ns, "late_resident")
    ns = build_parser().parse_args(["--late_resident"])
    assert ns.late_resident is True and len(vars(ns)) == 38
    ns = build_parser().parse_args(["--late_resident", "--gpu_decode", "--gpu_resident_gb", "60"])
    assert ns.late_resident is True and ns.gpu_decode is True and ns.gpu_resident_gb == 60.0


@pytest.mark.parametrize("shuffle", [True, False])
def test_rank_shard_sampler_yields_the_host_sets_indices(tmp_path, shuffle):
    from egaze_amd import dp
    from egaze_amd.data.lateDataset import lateDataset
    from egaze_amd.data.late_resident import ResidentLateDataset
    args = late_args(late_tree(tmp_path, hw=(4, 4), n_train=11, n_val=1))
    host, res = lateDataset(*args), ResidentLateDataset(*args)
    for rank in range(3):
        a = dp.RankShardSampler(host, shuffle, 2, world=3, rank_=rank, pad=shuffle)
        b = dp.RankShardSampler(res, shuffle, 2, world=3, rank_=rank, pad=shuffle)
        for epoch in range(2):
            a.set_epoch(epoch)
            b.set_epoch(epoch)
            assert list(a) == list(b) and len(a) == len(b) > 0


@pytest.mark.parametrize("seed", [0, 7])
def test_batch_order_is_the_host_datasets(tmp_path, seed):
    """A seeded shuffling loader draws the same indices in the same batches over both datasets, epoch after epoch."""
    from torch.utils.data import DataLoader, Dataset
    from egaze_amd.data.late_resident import ResidentLateDataset
    args = late_args(late_tree(tmp_path, hw=(4, 4), n_train=7, n_val=1))

    class Numbers(Dataset):                               # the host dataset's length, its samples replaced by their numbers
        def __len__(self):
            return len(args[4])

        def __getitem__(self, i):
            return i
    res = ResidentLateDataset(*args)
    order = {}
    for name, ds, collate in (("host", Numbers(), None), ("resident", res, res.collate_fn)):
        torch.manual_seed(seed)
        loader = DataLoader(ds, batch_size=3, shuffle=True, num_workers=0, collate_fn=collate)
        order[name] = [[(b if name == "host" else b["index"]).tolist() for b in loader] for _ in range(2)]
    assert order["host"] == order["resident"] and order["host"][0] != order["host"][1]
    assert [len(b) for b in order["resident"][0]] == [3, 3, 1]


# ----------------------------------------------------------------------------- C-ABI refusals (nothing is launched)
def _call(**over):
    from egaze_amd import _lib
    a = dict(pool=0x1000, P=57, table=0x2000, N=14, idx=0x3000, B=4, H=224, W=224, fused=0x10000, gt=0x20000, raw=None,
             status=0x6000, stream=None)
    a.update(over)
    rc = _lib.LIB.egz_late_gather(*a.values())
    return rc, _lib.LIB.egz_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(pool=None), "pool"), (dict(table=None), "table"), (dict(idx=None), "idx"), (dict(status=None), "status"),
    (dict(B=0), "B"), (dict(B=-1), "B"), (dict(B=65536), "B"), (dict(H=0), "H"), (dict(W=-3), "W"),
    (dict(H=3, W=3), "multiple of 4"), (dict(H=1, W=2), "multiple of 4"),
    (dict(fused=None, gt=None), "no output"),
    (dict(fused=0x10004), "16-byte"), (dict(gt=0x20008), "16-byte"), (dict(raw=0x30002), "4-byte"), (dict(pool=0x1001), "4-byte"),
    (dict(P=0), "P"), (dict(N=0), "N"),
])
def test_cabi_refuses_bad_arguments_before_any_launch(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("egz_late_gather") and word in msg, (rc, msg)


def test_symbol_is_declared_bound_exported_and_wrapped():
    import test_cabi_symbols as T
    from egaze_amd import _lib, hipops
    assert T._declared()["egz_late_gather"] == len(_lib.SIGNATURES["egz_late_gather"][1]) == 13
    T.test_header_binding_and_library_agree()
    assert hipops.late_gather is hipops.dataprep.late_gather
