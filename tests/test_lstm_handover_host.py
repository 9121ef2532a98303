"""Host side of the in-memory SP -> AT hand-over (``gaze_full --lstm_handover``): the numpy restatement of egz_lstm_store
(lstm_store_ref) against torch on the CPU -- the cell scores and the gaze cell bit for bit, on planes where another summation
order picks another cell; ResidentLSTMDataset.from_st against the listing of a folder of vector files; the parser's refusals.
No GPU: nothing touches a device."""
import os
import types

import numpy as np
import pytest
import torch

import lstm_store_ref as R
from test_late_handover_host import st_args

TRAIN_VIDEOS, VAL_VIDEO = ("Ahmad_American1", "Ahmad_Pizza1"), "Alireza_Pizza1"
# STDataset dilates the labels by one frame each side: every five frames become 1 1 1 0 0, one fixation of three frames
RAW_FLAGS = [0, 1, 0, 0, 0]
N_TRAIN, N_VAL = 15, 20                                   # frames per training video / of the validation video


def lstm_tree(root, n_train=N_TRAIN, n_val=N_VAL, seed=0):
    """A dataset tree with two training videos and one validation video (Alireza's), test_late_handover_host.handover_tree's
    recipe: 224 x 224 PNG frames, grey JPEG flow with the ten-frame window behind every sample, PNG ground-truth blobs, one
    fixation file per video.  Every fifth frame from the second on is the second frame of a fixation: three vectors per training
    video (a state reset lies between the videos), four in the validation video.  -> the paths as gaze_full's flags name them."""
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

    for folder, n in [(v, n_train) for v in TRAIN_VIDEOS] + [(VAL_VIDEO, n_val)]:
        os.makedirs(os.path.join(paths["flowPath"], folder), exist_ok=True)
        for num in range(1, 10 + n):
            for ax in "xy":
                Image.fromarray(smooth(())).save(os.path.join(paths["flowPath"], folder, f"flow_{ax}_{num:05d}.jpg"), quality=90)
        for num in range(10, 10 + n):
            Image.fromarray(smooth((3,))).save(os.path.join(paths["imagePath"], f"{folder}_img_{num:05d}.png"))
            cy, cx = rs.uniform(20, 200, 2)
            blob = 255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * 18.0 ** 2))
            Image.fromarray(blob.astype(np.uint8)).save(os.path.join(paths["gtPath"], f"{folder}_000000_{num:05d}.png"))
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), np.array((RAW_FLAGS * n)[:n], dtype=float))
    return paths


def written_names(train):
    """The files extractw writes for one split of lstm_tree, from the flag pattern alone: frames 1, 6, 11, ... of a video."""
    videos = [(v, N_TRAIN) for v in TRAIN_VIDEOS] if train else [(VAL_VIDEO, N_VAL)]
    return [f"fix_{v}_img_{10 + i:05d}.pth.tar" for v, n in videos for i in range(1, n, 5)]


def vector_folder(path, names):
    os.makedirs(path)
    for name in names:
        torch.save(torch.zeros(512), os.path.join(path, name))
    return path


# ----------------------------------------------------------------------------- the restatement against torch on the CPU
def _torch_cell(u8):
    pooled = torch.nn.functional.avg_pool2d(torch.from_numpy(u8).float()[None, None] / 255, 16)
    return pooled[0, 0].numpy(), int(torch.max(pooled.view(1, 1, -1), 2)[1])


def _planes():
    rs = np.random.RandomState(3)
    planes = [rs.randint(0, 256, (224, 224)).astype(np.uint8) for _ in range(6)]
    planes.append(np.zeros((224, 224), np.uint8))
    for y, x, v in ((0, 0, 1), (223, 223, 255), (100, 37, 7)):
        p = np.zeros((224, 224), np.uint8)
        p[y, x] = v
        planes.append(p)
    planes.append(np.full((224, 224), 255, np.uint8))
    return planes


def test_cell_scores_and_gaze_cell_equal_torch_bit_for_bit():
    for p in _planes():
        want, cell = _torch_cell(p)
        got = R.cell_scores(p)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert R.gaze_cell(p) == cell
    assert R.gaze_cell(np.zeros((224, 224), np.uint8)) == 0                  # an all-zero plane: the first cell


def test_tie_planes_separate_the_summation_orders():
    """Blobs centred on a cell corner or edge: the restatement follows torch on every one, the exact integer sums pick another
    cell on at least a third of them (a condition on this test's own inputs: an integer-sum kernel cannot pass here)."""
    blobs = R.corner_blobs(120, seed=1)
    differ = 0
    for p in blobs:
        want, cell = _torch_cell(p)
        assert np.array_equal(R.cell_scores(p).view(np.uint32), want.view(np.uint32))
        assert R.gaze_cell(p) == cell
        differ += R.integer_sum_cell(p) != cell
    print(f"\n{differ} of {len(blobs)} tie planes: the exact integer sums pick another cell than torch")
    assert differ * 3 >= len(blobs)


def test_window_equals_var_window():
    from egaze_amd.extractLSTMw import var_window
    for size in range(1, 6):
        for ind in range(196):
            assert R.window(ind, size, 14) == var_window(ind, size, 14, 14), (size, ind)
    for H in (6, 7):                                                          # up to the whole map, odd and even sides
        for size in (1, H - 1, H):
            for ind in range(H * H):
                win = R.window(ind, size, H)
                assert win == var_window(ind, size, H, H) and 0 <= win[0] < win[1] <= H and 0 <= win[2] < win[3] <= H


def _rows_and_channel_weight(size):
    """store_rows and the host's channel_weight on the same eight samples -> (rows (8, C), want (8, C), window counts (8,),
    feat)."""
    from egaze_amd.extractLSTMw import channel_weight
    rs = np.random.RandomState(size)
    planes = np.stack(_planes()[:4] + list(R.corner_blobs(4, seed=size)))
    feat = rs.standard_normal((len(planes), 14, 14, 24)).astype(np.float32)
    rows, cells = R.store_rows(feat, planes, np.arange(len(planes)), np.arange(len(planes)), size)
    want, counts = [], []
    for b, p in enumerate(planes):
        nchw = torch.from_numpy(feat[b:b + 1]).permute(0, 3, 1, 2).contiguous()
        want.append(channel_weight(nchw, torch.from_numpy(p).float()[None, None] / 255, size, False).numpy())
        assert cells[b] == _torch_cell(p)[1]
        y0, y1, x0, x1 = R.window(int(cells[b]), size, 14)
        counts.append((y1 - y0) * (x1 - x0))
    skipped, cells = R.store_rows(feat, planes, np.arange(len(planes)), np.full(len(planes), -1), size)
    assert skipped == {} and (cells == -1).all()
    return np.stack([rows[b] for b in range(len(planes))]), np.stack(want), np.array(counts), feat


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5])
def test_store_rows_equal_channel_weight_on_the_cpu(size):
    """Bit for bit: the host branch of channel_weight adds the window's cells one after the other (extractLSTMw.sequential_mean),
    as egz_window_mean and egz_lstm_store do.  (torch's own ``mean`` adds in several partial sums from 16 elements on: with it
    sizes 3, 4 and 5 -- windows of 12 to 36 cells -- differed in the last bits on 123, 133 and 150 of these 192 values.)"""
    rows, want, counts, _ = _rows_and_channel_weight(size)
    a, b = rows.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    ulp = np.abs(np.where(a < 0, -(a & 0x7fffffff), a) - np.where(b < 0, -(b & 0x7fffffff), b))
    print(f"\nsize {size}: windows of {sorted(set(counts.tolist()))} cells, {int((ulp > 0).sum())} of {ulp.size} values differ, "
          f"at most {int(ulp.max())} ulp")
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return lstm_tree(tmp_path_factory.mktemp("lstm_handover_host") / "tree")


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("task", [None, "Pizza"])
def test_from_st_plans_what_the_folder_lists(tree, tmp_path, train, task):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.data.resident import ResidentSTDataset
    st = ResidentSTDataset(*st_args(tree, train), raw_u8=True)
    assert [int(f) for f in st.fixsac[:5]] == [1, 1, 1, 0, 0]
    listed = ResidentLSTMDataset(vector_folder(str(tmp_path / "vec"), written_names(train)), task)
    ds = ResidentLSTMDataset.from_st(st, task=task)
    F = (3 if task else 6) if train else 4
    assert ds.listFiles == listed.listFiles and len(ds.listFiles) == F and len(ds) == len(listed) == F - 1
    for a, b in zip(ds.plan_host, listed.plan_host):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert ds.n_steps == listed.n_steps == F - 2
    assert ds.needed_bytes == F * 512 * 4 + 9 * (F - 2)
    if train and task is None:
        assert ds.plan_host[2].tolist() == [1, 0, 1, 0]   # the third step's input is the last vector of the first video
    names = [n for n in written_names(train) if task is None or task in n]
    assert [st.listTrainFiles[i] for i in ds.st_index.tolist()] == [n[4:-8] + ".png" for n in names]
    assert ds.st_index.dtype == torch.int64 and ds.pool is None and ds.plan is None and not ds.filled
    with pytest.raises(RuntimeError, match="from_st"):    # no files to read
        ds.fill("cuda:0")
    with pytest.raises(RuntimeError, match=rf"{ds.needed_bytes} bytes, 1 bytes are allowed"):
        ds.allocate("cuda:0", budget_bytes=1)             # refused before anything is allocated
    assert ds.pool is None and ds.plan is None
    with pytest.raises(RuntimeError, match="device memory only"):
        ds[0]
    with pytest.raises(RuntimeError, match="from_st"):    # ... and a listed folder is never allocated empty
        listed.allocate("cuda:0")


def _fake_st(names, flags):
    return types.SimpleNamespace(listTrainFiles=list(names), fixsac=np.array(flags, dtype=float))


def test_rows_follow_the_sorted_names_not_the_dataset_order(tmp_path):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset, lstm_plan
    names = [f"{v}_img_{k:05d}.png" for v in ("Zed_Tea1", "Ahmad_Pizza1", "Mo_Tea2") for k in (10, 11, 12, 13)]
    flags = [1, 1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 0]          # second frames: 1, 6, 9
    ds = ResidentLSTMDataset.from_st(_fake_st(names, flags))
    assert ds.st_index.tolist() == [6, 9, 1]              # Ahmad, Mo, Zed: the rows are the sorted names' positions
    assert ds.listFiles == ["fix_Ahmad_Pizza1_img_00012.pth.tar", "fix_Mo_Tea2_img_00011.pth.tar", "fix_Zed_Tea1_img_00011.pth.tar"]
    listed = ResidentLSTMDataset(vector_folder(str(tmp_path / "vec"), ds.listFiles))
    assert listed.listFiles == ds.listFiles and all(np.array_equal(a, b) for a, b in zip(ds.plan_host, lstm_plan(listed.listFiles)))
    assert ResidentLSTMDataset.from_st(_fake_st(names, flags), task="Tea").st_index.tolist() == [9, 1]


def test_from_st_refusals():
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    names = [f"Ahmad_Pizza1_img_{k:05d}.png" for k in range(10, 18)]
    flags = [1, 1, 0, 0, 1, 1, 1, 0]
    assert ResidentLSTMDataset.from_st(_fake_st(names, flags)).st_index.tolist() == [1, 5]
    dup = list(names)
    dup[5] = dup[1]                                       # two extracted frames, one vector file
    with pytest.raises(ValueError, match=rf"sample 5 \({dup[5]}\) has the name of sample 1"):
        ResidentLSTMDataset.from_st(_fake_st(dup, flags))
    with pytest.raises(RuntimeError, match="fixation is not processed"):      # a one-frame fixation: the file path's error
        ResidentLSTMDataset.from_st(_fake_st(names, [0, 1, 0, 0, 1, 1, 0, 0]))
    with pytest.raises(ValueError, match="8 frames but 7 fixation flags"):
        ResidentLSTMDataset.from_st(_fake_st(names, flags[:7]))
    empty = ResidentLSTMDataset.from_st(_fake_st(names, flags), task="Burger")      # a task that matches nothing: an empty
    assert empty.listFiles == [] and empty.n_steps == 0 and empty.needed_bytes == 0  # listing, as of an empty folder ...
    with pytest.raises(RuntimeError, match="no vectors"):                             # ... and nothing to allocate
        empty.allocate("cuda:0")


# ----------------------------------------------------------------------------- the parser
def test_parser_refusals(monkeypatch, capsys):
    from egaze_amd.gaze_full import build_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    full = ["--gpu_resident", "--extract_lstm", "--train_lstm", "--lstm_handover"]
    ns = build_parser().parse_args(full)
    assert ns.lstm_handover is True and ns.lstm_resident is True            # implies --lstm_resident
    assert not hasattr(ns, "lstm_handover_chunk")
    assert build_parser().parse_args(full + ["--lstm_handover_chunk", "32"]).lstm_handover_chunk == 32
    assert not hasattr(build_parser().parse_args([]), "lstm_handover")      # the reference's namespace without the flag
    assert not hasattr(build_parser().parse_args(full[:3]), "lstm_resident")
    for drop in ("--gpu_resident", "--extract_lstm", "--train_lstm"):
        with pytest.raises(SystemExit) as e:
            build_parser().parse_args([a for a in full if a != drop])
        assert e.value.code == 2 and f"--lstm_handover needs {drop}" in capsys.readouterr().err
    for extra, message in ((["--align"], "does not take --align"), (["--lstm_handover_chunk", "0"], "at least 1")):
        with pytest.raises(SystemExit) as e:
            build_parser().parse_args(full + extra)
        assert e.value.code == 2 and message in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        build_parser().parse_args(full[:3] + ["--lstm_handover_chunk", "4"])
    assert e.value.code == 2 and "--lstm_handover_chunk needs --lstm_handover" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        build_parser().parse_args(full)
    assert e.value.code == 2 and "one process" in capsys.readouterr().err
    build_parser().parse_args(full[:3])                                     # without the flag WORLD_SIZE is not looked at
    monkeypatch.setenv("WORLD_SIZE", "1")
    both = build_parser().parse_args(full + ["--extract_late", "--train_late", "--late_handover"])
    assert both.lstm_handover and both.late_handover and both.lstm_resident and both.late_resident
