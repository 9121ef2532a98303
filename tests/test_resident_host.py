"""Host side of the resident dataset (data/resident.py, egz_resident_gather's argument checks).  No GPU: plan() and the
refusals touch no device and launch nothing."""
import os

import numpy as np
import pytest
import torch

from test_jpeg_host import make_tree

FRAMES = tuple(range(11, 18))


def resident_tree(root):
    """7 samples with overlapping flow windows, progressive frames and PNG ground truths (the host route)."""
    args = make_tree(str(root), frames=FRAMES)
    np.savetxt(os.path.join(args[7], "a.txt"), np.array([0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0]))
    return args


def test_plan_counts_shares_and_assigns_each_plane_once(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True)
    assert len(ds) == 7 and ds.loader_workers == 0
    ds.plan()
    assert ds.planes == 21 + 7 + 32 == 60 and ds.hw == (224, 224)
    t = ds.plane_table
    assert t.shape == (7, 22) and t.dtype == torch.int64
    assert ds.needed_bytes == 60 * 50176 + t.numel() * 8
    for i in range(6):                                    # consecutive samples share 18 of their 20 flow planes
        for j in range(1, 19):
            assert t[i + 1, j + 2] == t[i, j], (i, j)
    # every plane belongs to exactly one file, files do not overlap, and the table points at file starts
    taken = np.zeros(ds.planes, dtype=int)
    start = {}
    for path, plane, channels in ds.files:
        taken[plane:plane + channels] += 1
        start[path] = plane
    assert (taken == 1).all() and len(start) == len(ds.files) == 7 + 7 + 32
    for i in range(7):
        assert [start[p] for p in ds._files(i)] == t[i].tolist()
    assert len(set(t[:, 0].tolist())) == 7 and len(set(t[:, 21].tolist())) == 7
    assert len(set(t[:, 1:21].flatten().tolist())) == 32


def test_plan_honours_gpu_fields(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True)
    ds.gpu_fields = ("flow", "gt")
    ds.plan()
    assert ds.planes == 32 + 7 and (ds.plane_table[:, 0] == -1).all() and (ds.plane_table[:, 1:] >= 0).all()
    assert all("img" not in os.path.basename(f[0]) for f in ds.files)
    ds.gpu_fields = ("image", "gt")
    ds.plan()
    assert ds.planes == 21 + 7 and (ds.plane_table[:, 1:21] == -1).all()


def test_fill_over_budget_raises_before_touching_a_device(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    ds = ResidentSTDataset(*resident_tree(tmp_path), raw_u8=True)
    needed = 60 * 50176 + 7 * 22 * 8
    with pytest.raises(RuntimeError, match=rf"{needed} bytes.* 1 bytes are allowed"):
        ds.fill("cuda:0", budget_bytes=1)
    assert ds.pool is None and ds.table is None


def test_samples_read_no_file_and_collate_carries_indices(tmp_path):
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    args = resident_tree(tmp_path / "t")
    ds, host = ResidentSTDataset(*args, raw_u8=True), STDataset(*args, raw_u8=True)
    for f in os.listdir(args[1]):                         # no image file left: a resident sample opens none
        os.remove(os.path.join(args[1], f))
    s = ds[4]
    assert set(s) == {"index", "fixsac", "imname"} and s["index"] == 4 and s["imname"] == args[4][4]
    assert torch.equal(s["fixsac"], torch.FloatTensor([host.fixsac[4]]))
    b = ds.collate_fn([ds[5], ds[0], ds[5]])
    assert b["resident"] is ds and b["index"].dtype == torch.int64 and b["index"].tolist() == [5, 0, 5]
    assert b["fixsac"].shape == (3, 1) and b["imname"] == [args[4][5], args[4][0], args[4][5]]


@pytest.mark.parametrize("seed", [0, 7])
def test_batch_order_is_the_host_datasets(tmp_path, seed):
    """A seeded shuffling loader visits the same samples in the same batches over both datasets, epoch after epoch."""
    from torch.utils.data import DataLoader
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    args = resident_tree(tmp_path)
    order = {}
    for name, ds in (("host", STDataset(*args, raw_u8=True)), ("resident", ResidentSTDataset(*args, raw_u8=True))):
        torch.manual_seed(seed)
        loader = DataLoader(ds, batch_size=3, shuffle=True, num_workers=0, collate_fn=ds.collate_fn)
        order[name] = [[list(b["imname"]) for b in loader] for _ in range(2)]
    assert order["host"] == order["resident"]
    assert len(order["host"][0]) == 3 and order["host"][0] != order["host"][1]
    assert sorted(n for b in order["resident"][0] for n in b) == sorted(args[4])


# ----------------------------------------------------------------------------- C-ABI refusals (nothing is launched)
def _call(**over):
    from egaze_amd import _lib
    a = dict(pool=0x1000, P=60, table=0x2000, N=7, idx=0x3000, B=3, H=224, W=224, mean=0x4000, std=0x5000, image=0x10000,
             flow=0x20000, gt=0x30000, nhwc=None, absmax=None, raw=None, raw_fields=7, status=0x6000, stream=None)
    a.update(over)
    rc = _lib.LIB.egz_resident_gather(*a.values())
    return rc, _lib.LIB.egz_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(pool=None), "pool"), (dict(table=None), "table"), (dict(idx=None), "idx"),
    (dict(B=0), "B"), (dict(B=-1), "B"), (dict(H=0), "H"), (dict(W=-3), "W"),
    (dict(H=3, W=3), "multiple of 4"), (dict(H=1, W=2), "multiple of 4"),
    (dict(image=None, flow=None, gt=None), "no output"),
    (dict(nhwc=0x40000), "absmax"), (dict(absmax=0x50000), "flow_nhwc32"),
    (dict(status=None), "status"), (dict(mean=None), "mean"),
    (dict(raw=0x70000, raw_fields=0), "raw_fields"),
])
def test_cabi_refuses_bad_arguments_before_any_launch(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("egz_resident_gather") and word in msg, (rc, msg)


def test_symbol_is_declared_bound_and_exported():
    """The entry is in all three places the existing symbol test compares (which passes with it)."""
    import test_cabi_symbols as T
    from egaze_amd import _lib
    assert T._declared()["egz_resident_gather"] == len(_lib.SIGNATURES["egz_resident_gather"][1]) == 19
    T.test_header_binding_and_library_agree()


def test_cli_flags_are_absent_unless_given():
    from egaze_amd import gaze_full, streamtrain
    for parser in (gaze_full.build_parser(), streamtrain.build_parser("spatial"), streamtrain.build_parser("temporal")):
        ns = parser.parse_args([])
        assert not hasattr(ns, "gpu_resident") and not hasattr(ns, "gpu_resident_gb")
        ns = parser.parse_args(["--gpu_resident", "--gpu_resident_gb", "100", "--gpu_decode"])
        assert ns.gpu_resident is True and ns.gpu_resident_gb == 100.0 and ns.gpu_decode is True


def test_cli_budget_refusal_covers_both_sets_and_touches_no_device(tmp_path):
    """streamtrain.make_loaders with --gpu_resident and a budget the planes do not fit: refused from the plan alone."""
    import argparse
    from egaze_amd import streamtrain
    a = resident_tree(tmp_path)
    args = argparse.Namespace(flowPath=a[0], imagePath=a[1], gtPath=a[2], fixsacPath=a[7], val_name="Alireza", batch_size=3,
                              device="0", gpu_resident=True, gpu_resident_gb=1e-3)
    with pytest.raises(RuntimeError, match=rf"{(32 + 7) * 50176 + 7 * 22 * 8} bytes, 1000000 bytes are allowed"):
        streamtrain.make_loaders(args, key="flow")
