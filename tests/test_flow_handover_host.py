"""Host side of the in-memory flow hand-over (``gaze_full --gpu_resident --flow_handover``): the parser's refusals, the plan
with ``flow_from`` against the plan over files, the refusal of a sample whose flow the frames cannot give, and which chunk
ranges flows_into decodes and computes.  No GPU: nothing touches a device (flows_into runs on CPU tensors with the decode and
the flow computation replaced by recorders, at quality 0)."""
import os

import numpy as np
import pytest
import torch

TRAIN, VAL = "Ahmad_Pizza1", "Alireza_Pizza1"
SAMPLES = list(range(10, 16)) + list(range(22, 26))          # a gap: flows 26 .. 29 of the 30 frames are never referred to
FLOWS = set(range(1, 26))                                    # the ten flows ending at each sample's number


def flow_tree(root, frames=30, hw=(44, 60), samples=SAMPLES, seed=0, frame_quality=92):
    """Two videos (training / validation) of ``frames`` colour JPEG frames img_00001 .. under framePath, and for the frame
    numbers in ``samples`` (a list, or one list per video) an image (PNG), a ground-truth blob (PNG) and a fixation flag.  A textured pattern drifts across
    the frames so that TV-L1 has a flow to find.  No flow folder is made.  -> the paths as gaze_full's flags name them."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    root = str(root)
    paths = {k: os.path.join(root, d) for k, d in (("framePath", "frames"), ("flowPath", "flow"), ("imagePath", "img"),
                                                   ("gtPath", "gt"), ("fixsacPath", "fs"))}
    for k, d in paths.items():
        if k != "flowPath":
            os.makedirs(d, exist_ok=True)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    per_video = samples if isinstance(samples, dict) else {TRAIN: samples, VAL: samples}
    for folder in (TRAIN, VAL):
        samples = per_video[folder]
        os.makedirs(os.path.join(paths["framePath"], folder))
        low = rs.randint(0, 256, (h // 4 + 8, w // 4 + 20, 3)).astype(np.uint8)
        big = np.asarray(Image.fromarray(low).resize((4 * low.shape[1], 4 * low.shape[0]), Image.BICUBIC))
        for num in range(1, frames + 1):
            dy, dx = int(round(6 + 5 * np.sin(num / 4.0))), 2 * num
            frame = big[dy:dy + h, dx:dx + w]
            Image.fromarray(frame).save(os.path.join(paths["framePath"], folder, f"img_{num:05d}.jpg"), quality=frame_quality)
            if num in samples:
                Image.fromarray(frame).save(os.path.join(paths["imagePath"], f"{folder}_img_{num:05d}.png"))
                cy, cx = rs.uniform(0.2 * h, 0.8 * h), rs.uniform(0.2 * w, 0.8 * w)
                blob = 255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (h / 12.0) ** 2))
                Image.fromarray(blob.astype(np.uint8)).save(os.path.join(paths["gtPath"], f"{folder}_000000_{num:05d}.png"))
        np.savetxt(os.path.join(paths["fixsacPath"], folder + ".txt"), (rs.rand(len(samples)) < 0.5).astype(float))
    return paths


def st_args(paths, train=True, listed="framePath", val_name="Alireza"):
    """STDataset's positional arguments for one split, listed as gaze_full.main lists it (``listed``: the folder whose
    sub-folders are the videos -- framePath under --flow_handover, flowPath otherwise)."""
    from egaze_amd.gaze_full import _split
    k = 0 if train else 1
    return (paths["flowPath"], paths["imagePath"], paths["gtPath"], sorted(os.listdir(paths[listed])),
            _split(paths["imagePath"], val_name)[k], _split(paths["gtPath"], val_name)[k],
            _split(paths["fixsacPath"], val_name)[k], paths["fixsacPath"])


def test_parser_refusals(monkeypatch, capsys):
    from egaze_amd.gaze_full import build_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    full = ["--gpu_resident", "--flow_handover", "--framePath", "frames"]
    ns = build_parser().parse_args(full)
    assert ns.flow_handover is True and ns.framePath == "frames"
    assert not hasattr(ns, "flow_quality") and not hasattr(ns, "flow_bound")              # main() takes extract_flow's defaults
    ns = build_parser().parse_args(full + ["--flow_quality", "0", "--flow_bound", "15"])
    assert ns.flow_quality == 0 and ns.flow_bound == 15.0
    bare = build_parser().parse_args([])
    assert not any(hasattr(bare, k) for k in ("flow_handover", "framePath", "flow_quality", "flow_bound"))

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            build_parser().parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    refused(full[1:], "--flow_handover needs --gpu_resident")
    refused(full[:2], "--flow_handover needs --framePath")
    refused(["--gpu_resident", "--framePath", "frames"], "--framePath needs --flow_handover")
    refused(["--gpu_resident", "--flow_quality", "95"], "--flow_quality needs --flow_handover")
    refused(["--gpu_resident", "--flow_bound", "20"], "--flow_bound needs --flow_handover")
    refused(full + ["--flow_quality", "101"], "--flow_quality must be 0 .. 100")
    refused(full + ["--flow_quality", "-1"], "--flow_quality must be 0 .. 100")
    refused(full + ["--flow_bound", "0"], "--flow_bound must be positive")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(full, "one process")
    build_parser().parse_args(["--gpu_resident"])                                         # without the flag WORLD_SIZE is not looked at
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert build_parser().parse_args(full).flow_handover


@pytest.mark.parametrize("train", [True, False])
def test_plan_with_flow_from_is_the_plan_over_files(tmp_path, train):
    """Same files list, planes, table and bytes; the flow paths are keys with the planes the file plan gives them, and no flow
    file or folder has to exist for either plan."""
    from egaze_amd.data.resident import FlowFrom, ResidentSTDataset
    paths = flow_tree(tmp_path / "tree")
    assert not os.path.exists(paths["flowPath"])
    over_files = ResidentSTDataset(*st_args(paths, train), raw_u8=True).plan()
    ds = ResidentSTDataset(*st_args(paths, train), raw_u8=True)
    ds.flow_from = FlowFrom(paths["framePath"])
    ds.plan()
    N = len(SAMPLES)
    assert len(ds) == N and ds.hw == over_files.hw == (44, 60)
    assert ds.files == over_files.files and ds.planes == over_files.planes == 3 * N + 2 * len(FLOWS) + N
    assert torch.equal(ds.plane_table, over_files.plane_table) and int(ds.plane_table.min()) >= 0
    assert ds.needed_bytes == over_files.needed_bytes == ds.planes * 44 * 60 + N * 22 * 8
    assert over_files.flow_keys == [] and over_files.flow_from is None
    folder = TRAIN if train else VAL
    assert sorted(os.path.basename(p) for p, _ in ds.flow_keys) == sorted(
        f"flow_{ax}_{n:05d}.jpg" for n in FLOWS for ax in "xy")
    assert all(os.path.basename(os.path.dirname(p)) == folder for p, _ in ds.flow_keys)
    where = {path: plane for path, plane, _ in ds.files}
    assert all(where[p] == plane for p, plane in ds.flow_keys)
    assert sorted(plane for _, plane in ds.flow_keys) == list(range(3 * N, 3 * N + 2 * len(FLOWS)))
    assert ds.pool is None and not os.path.exists(paths["flowPath"])
    # flow planes only: the plane size is the frames'
    only = ResidentSTDataset(*st_args(paths, train), raw_u8=True)
    only.gpu_fields = ("flow",)
    only.flow_from = FlowFrom(paths["framePath"])
    assert only.plan().hw == (44, 60) and only.planes == 2 * len(FLOWS) == len(only.flow_keys)


def test_a_sample_whose_flow_the_frames_cannot_give_is_refused(tmp_path):
    from egaze_amd.data.resident import FlowFrom, ResidentSTDataset

    def planned(paths):
        ds = ResidentSTDataset(*st_args(paths, True), raw_u8=True)
        ds.flow_from = FlowFrom(paths["framePath"])
        return ds.plan()
    # below the first frame: sample 9 needs flow 0
    paths = flow_tree(tmp_path / "low", samples=[9, 10, 11, 12])
    with pytest.raises(RuntimeError, match=rf"sample 0 \({TRAIN}_000000_00009.png\) needs flow_x_00000.jpg of {TRAIN}.*"
                                           r"img_00000.jpg is missing"):
        planned(paths)
    # past the last pair: flow 30 runs from frame 30 to frame 31
    paths = flow_tree(tmp_path / "high", samples=[28, 29, 30])
    with pytest.raises(RuntimeError, match=rf"sample 2 \({TRAIN}_000000_00030.png\) needs flow_x_00030.jpg.*img_00031.jpg is missing"):
        planned(paths)
    # a frame missing in the middle: flows 11 and 12 are gone, sample 11 is the first to need one
    paths = flow_tree(tmp_path / "hole")
    os.remove(os.path.join(paths["framePath"], TRAIN, "img_00012.jpg"))
    with pytest.raises(RuntimeError, match=r"sample 1 \(.*_00011.png\) needs flow_x_00011.jpg.*img_00012.jpg is missing"):
        planned(paths)
    ok = ResidentSTDataset(*st_args(paths, False), raw_u8=True)                          # the other video is whole
    ok.flow_from = FlowFrom(paths["framePath"])
    assert ok.plan().pool is None


def test_wanted_ranges_are_process_folders_ranges_that_hold_a_wanted_flow():
    from egaze_amd.data.extract_flow import chunk_ranges, missing_frame, wanted_ranges
    frames = [(n, f"img_{n:05d}.jpg") for n in range(1, 31)]
    assert wanted_ranges(frames, FLOWS, 1) == [(i, i + 1) for i in range(25)]
    assert wanted_ranges(frames, FLOWS, 4) == chunk_ranges(30, 4)[:7] and chunk_ranges(30, 4)[7:] == [(28, 29)]
    assert wanted_ranges(frames, FLOWS, 32) == [(0, 29)]
    assert wanted_ranges(frames, {29}, 4) == [(28, 29)] and wanted_ranges(frames, {30}, 4) == []     # frame 30 starts no pair
    assert wanted_ranges(frames, {4, 5}, 4) == [(0, 4), (4, 8)] and wanted_ranges(frames, set(), 4) == []
    assert wanted_ranges(frames[:1], {1}, 4) == []
    assert missing_frame({1, 2, 3}, 2) is None and missing_frame({1, 2, 3}, 3) == 4 and missing_frame({1, 2, 3}, 0) == 0


class _FakeSet:
    """What flows_into reads of a filled ResidentSTDataset, with a pool on the host."""

    def __init__(self, folder, numbers, planes, hw=(4, 6)):
        self.hw = hw
        self.pool = torch.full((planes,) + hw, 0xA5, dtype=torch.uint8)
        self.flow_keys, p = [], 1                                                         # plane 0 is somebody else's
        for n in numbers:
            for ax in "xy":
                self.flow_keys.append((os.path.join("nowhere", folder, f"flow_{ax}_{n:05d}.jpg"), p))
                p += 2                                                                    # every other plane
        self.n = len(numbers)

    def __len__(self):
        return self.n


@pytest.mark.parametrize("chunk", [1, 4, 32])
def test_flows_into_skips_the_ranges_nobody_refers_to(tmp_path, monkeypatch, chunk):
    """Frames are 'decoded' to planes holding their number and 'flow' x / y of pair n is a plane of n / n + 100: the planes land
    where the keys say, only wanted ranges are decoded, every other plane keeps its bytes, the counts add up."""
    from egaze_amd.data import extract_flow as E
    frame_dir = tmp_path / "frames"
    for folder in (TRAIN, VAL):
        (frame_dir / folder).mkdir(parents=True)
        for n in range(1, 31):
            (frame_dir / folder / f"img_{n:05d}.jpg").write_bytes(b"")
    decoded = []

    def fake_decode(paths, size, device):
        assert size == (4, 6)
        decoded.append([os.path.join(os.path.basename(os.path.dirname(p)), os.path.basename(p)) for p in paths])
        nums = torch.tensor([int(os.path.basename(p)[4:9]) for p in paths], dtype=torch.uint8)
        return nums.view(-1, 1, 1, 1).expand(-1, 3, 4, 6).contiguous()

    def fake_flow(bgr, bound, params):
        assert bound == 20.0 and params == E.TVL1_DEFAULTS
        first = bgr[:-1, 0]
        return torch.stack((first, first + 100))
    monkeypatch.setattr(E, "decode_frames", fake_decode)
    monkeypatch.setattr(E, "flow_images", fake_flow)
    numbers = sorted(FLOWS)
    sets = [_FakeSet(TRAIN, numbers, 2 + 4 * len(numbers)), _FakeSet(VAL, [3, 4, 29], 14), _FakeSet(VAL, [], 3)]
    counts = E.flows_into(sets, str(frame_dir), "cpu", quality=0, chunk=chunk)
    frames = E.list_frames(str(frame_dir / TRAIN))
    want = [[os.path.join(TRAIN, frames[i][1]) for i in range(a, b + 1)] for a, b in E.wanted_ranges(frames, FLOWS, chunk)] + \
           [[os.path.join(VAL, frames[i][1]) for i in range(a, b + 1)] for a, b in E.wanted_ranges(frames, {3, 4, 29}, chunk)]
    assert decoded == want
    assert counts == {"pairs": sum(len(r) - 1 for r in want), "planes": 2 * len(numbers) + 6, "files": 0}
    if chunk == 1:
        assert counts["pairs"] == 25 + 3 and not any("img_00028" in p for r in decoded for p in r if p.startswith(TRAIN))
    for ds, nums in ((sets[0], numbers), (sets[1], [3, 4, 29])):
        written = {}
        for (path, plane) in ds.flow_keys:
            _, c, n = E.flow_key(path)
            written[plane] = n + 100 * c
        for p in range(ds.pool.shape[0]):
            assert bool((ds.pool[p] == written.get(p, 0xA5)).all()), (p, written.get(p))
    assert bool((sets[2].pool == 0xA5).all())
    with pytest.raises(ValueError, match="chunk"):
        E.flows_into(sets, str(frame_dir), "cpu", quality=0, chunk=0)
    for q in (-1, 101, True, 95.0):
        with pytest.raises(ValueError, match="quality"):
            E.flows_into(sets, str(frame_dir), "cpu", quality=q)
