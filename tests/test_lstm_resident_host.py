"""Host side of the resident LSTM dataset (data/lstm_resident.py, hipops.lstm_pool_fetch's status words, --lstm_resident).  No
GPU: the plan is built from file names, and every refusal here happens before a device is touched."""
import os

import numpy as np
import pytest
import torch


def vector_tree(folder, videos, width=8, seed=0):
    """``videos``: [(name, frames)] -> fix_<name>_<10 digits>.pth.tar files of seeded float32 vectors, as extractLSTMw names
    them (the last 14 characters are the frame number's last six digits and the extension).  -> the sorted file names."""
    os.makedirs(str(folder), exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    names = []
    for name, frames in videos:
        for i in range(frames):
            names.append(f"fix_{name}_{i + 1:010d}.pth.tar")
            torch.save(torch.randn(width, generator=g), os.path.join(str(folder), names[-1]))
    return sorted(names)


def walked_plan(ds):
    """The plan derived again from the samples of lstmDataset: the reference's loop scores the prediction made from sample
    i - 1 against the target of sample i, so the step of iteration i runs the forward pass of sample i - 1 (reset first where
    THAT sample was flagged same == 0, or nothing ran before) against sample i's target.  Only names are compared: a
    sample's 'input' is file i, its 'gt' file i + 1."""
    from egaze_amd.data.LSTMdatas import lstmDataset
    row = {name: r for r, name in enumerate(ds.listFiles)}
    in_row, tgt_row, reset = [], [], []
    prev, pending_reset = None, True
    for i in range(lstmDataset.__len__(ds)):
        a, b = ds.listFiles[i], ds.listFiles[i + 1]
        same = b[:-14] == a[:-14]                     # lstmDataset.__getitem__'s flag
        if prev is not None:
            in_row.append(row[prev])
            tgt_row.append(row[b])
            reset.append(1 if pending_reset else 0)
            pending_reset = False
        if not same:
            pending_reset = True
        prev = a
    return np.array(in_row, dtype=np.int32), np.array(tgt_row, dtype=np.int32), np.array(reset, dtype=np.uint8)


def test_schedule_of_the_golden_replay_flags():
    """same = [1, 1, 1, 0, 1] (test_hip_at's replay fixture): four steps, the state reset on the first and on the one whose
    deferred sample (3) carries the 0."""
    from egaze_amd.data.LSTMdatas import deferred_steps
    same = [1, 1, 1, 0, 1]
    steps = list(deferred_steps((f"in{i}", f"gt{i}", same[i]) for i in range(5)))
    assert steps == [("in0", "gt1", True), ("in1", "gt2", False), ("in2", "gt3", False), ("in3", "gt4", True)]
    assert all(type(s[2]) is bool for s in steps)


@pytest.mark.parametrize("n", [0, 1])
def test_schedule_of_fewer_than_two_samples_is_empty(n):
    from egaze_amd.data.LSTMdatas import deferred_steps
    assert list(deferred_steps([("in", "gt", 0)] * n)) == []


def test_schedule_reads_nothing_ahead():
    """After yielding k steps the generator has pulled exactly k + 1 samples: the file loop reads no file early."""
    from egaze_amd.data.LSTMdatas import deferred_steps
    pulled = []

    def samples():
        for i in range(6):
            pulled.append(i)
            yield i, 10 + i, i != 2
    steps = deferred_steps(samples())
    assert pulled == []                                 # nothing before the first step is asked for
    for k, got in enumerate(steps, start=1):
        assert len(pulled) == k + 1
        assert got == (k - 1, 10 + k, k == 1 or k == 3)
    assert k == 5 and len(pulled) == 6


def test_plan_of_the_five_file_example(tmp_path):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset, lstm_plan
    vector_tree(tmp_path, [("A_x", 3), ("B_x", 2)])
    ds = ResidentLSTMDataset(str(tmp_path))
    assert len(ds.listFiles) == 5 and len(ds) == 4 and ds.pool is None and ds.plan is None and not ds.filled
    got = ds.plan_host
    assert [a.dtype for a in got] == [np.int32, np.int32, np.uint8]
    triples = list(zip(*(a.tolist() for a in got)))
    assert triples == [(0, 2, 1), (1, 3, 0), (2, 4, 1)]       # the reset falls on the LAST frame of video A (file 2)
    assert ds.n_steps == len(ds) - 1 == 3
    for a, b in zip(got, walked_plan(ds)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for a, b in zip(lstm_plan(ds.listFiles), got):
        assert np.array_equal(a, b)
    # before fill() the dataset is the file set
    s = ds[2]
    assert torch.equal(s['input'], torch.load(os.path.join(str(tmp_path), ds.listFiles[2]))) and s['same'] is False


def test_plan_of_three_videos_under_a_name_filter(tmp_path):
    from egaze_amd.data.LSTMdatas import lstmDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    vector_tree(tmp_path, [("Ahmad_Pizza1", 4), ("Carlos_Tea2", 5), ("Ahmad_Pizza3", 1), ("Ahmad_Tea1", 3)])
    ds = ResidentLSTMDataset(str(tmp_path), name="Ahmad")
    assert ds.listFiles == lstmDataset(str(tmp_path), "Ahmad").listFiles and len(ds.listFiles) == 8
    triples = list(zip(*(a.tolist() for a in ds.plan_host)))
    # files: Pizza1 x 4 (rows 0-3), Pizza3 x 1 (row 4), Tea1 x 3 (rows 5-7); a one-frame video resets twice in a row
    assert triples == [(0, 2, 1), (1, 3, 0), (2, 4, 0), (3, 5, 1), (4, 6, 1), (5, 7, 0)]
    assert ds.n_steps == len(ds) - 1
    for a, b in zip(ds.plan_host, walked_plan(ds)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("F", [2, 1])
def test_short_sets_have_no_step(tmp_path, F):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    vector_tree(tmp_path, [("A_x", F)])
    ds = ResidentLSTMDataset(str(tmp_path))
    assert ds.n_steps == 0 and all(len(a) == 0 for a in ds.plan_host)
    assert all(len(a) == 0 for a in walked_plan(ds))


def test_budget_refusal_names_the_bytes_and_leaves_no_pool(tmp_path):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    vector_tree(tmp_path, [("A_x", 6), ("B_x", 5)], width=24)
    ds = ResidentLSTMDataset(str(tmp_path))
    need = 11 * 24 * 4 + 9 * 9
    allowed = int((need - 1) / 1e9 * 1e9)
    with pytest.raises(RuntimeError) as e:
        ds.fill("cuda:0", budget_gb=(need - 1) / 1e9)
    assert allowed < need and f"needs {need} bytes, {allowed} bytes are allowed" in str(e.value)
    assert ds.pool is None and ds.plan is None and ds.needed_bytes == need


@pytest.mark.parametrize("bad", ["float64", "length"])
def test_a_bad_file_is_named(tmp_path, bad):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    names = vector_tree(tmp_path, [("A_x", 4)])
    v = torch.zeros(8, dtype=torch.float64) if bad == "float64" else torch.zeros(9)
    torch.save(v, os.path.join(str(tmp_path), names[2]))
    ds = ResidentLSTMDataset(str(tmp_path))
    with pytest.raises(ValueError, match=names[2].replace(".", r"\.")):
        ds.fill("cuda:0", budget_gb=1.0)
    assert ds.pool is None


def test_parser_keeps_the_37_defaults():
    from egaze_amd.gaze_full import build_parser
    ns = build_parser().parse_args([])
    assert len(vars(ns)) == 37 and not hasattr(ns, "lstm_resident")
    ns = build_parser().parse_args(["--lstm_resident", "--gpu_resident_gb", "2.5"])
    assert ns.lstm_resident is True and ns.gpu_resident_gb == 2.5 and not hasattr(ns, "late_resident")


def test_status_checker_raises_on_every_nonzero_word():
    from egaze_amd import hipops as Hp
    assert sorted(Hp.LSTM_POOL_STATUS) == [1, 2, 3]
    Hp.check_lstm_pool_status(0)
    for word, text in ((1, "cursor outside the plan"), (2, "plan row outside the pool")):
        with pytest.raises(RuntimeError, match=text):
            Hp.check_lstm_pool_status(word)
    with pytest.raises(RuntimeError, match="cursor outside the plan and a plan row outside the pool"):
        Hp.check_lstm_pool_status(3)


def test_wrapper_refuses_host_tensors_and_wrong_shapes():
    from egaze_amd import hipops as Hp
    z = torch.zeros
    plan = (z(3, dtype=torch.int32), z(3, dtype=torch.int32), z(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pool must be"):
        Hp.lstm_pool_fetch(z(4, 8), plan, z(2, dtype=torch.int32), z(8), z(8), None, z(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="pool must be"):
        Hp.lstm_pool_fetch(None, plan, z(2, dtype=torch.int32), z(8), z(8), None, z(1, dtype=torch.int32))
