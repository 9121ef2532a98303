"""Host build of the JPEG decode core (csrc/jpeg_core.h) under AddressSanitizer + UBSan: bit-identical with the fixture's
libjpeg-turbo decodes, and memory-safe on truncated and byte-flipped streams.  Also the host side of STDataset(decode='gpu'):
the worker's header sniff and the batch collate.  No GPU needed."""
import os
import platform
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
CSRC = os.path.join(ROOT, "egocentric-gaze-prediction_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "jpeg_host_driver.cpp")

_BIN = {}


def fixture():
    z = np.load(FIXTURE)
    off, data, eoff = z["offsets"], z["data"], z["expect_offsets"]
    cases = []
    for i, name in enumerate(z["names"]):
        h, w, c = int(z["h"][i]), int(z["w"][i]), int(z["channels"][i])
        cases.append(dict(name=str(name), data=data[off[i]:off[i + 1]].tobytes(), h=h, w=w, c=c,
                          expect=z["expect"][eoff[i]:eoff[i + 1]].reshape(c, h, w)))
    extra = dict(progressive=z["progressive"].tobytes(), progressive_bgr=z["progressive_bgr"], png=z["png"].tobytes(),
                 png_gray=z["png_gray"])
    return cases, extra


def host_decoder():
    """g++ -fsanitize=address,undefined build of tests/jpeg_host_driver.cpp (once per session, in a temp directory)."""
    if "bin" not in _BIN:
        d = tempfile.mkdtemp(prefix="jpeg_host_")
        exe = os.path.join(d, "jpeg_host")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", CSRC, DRIVER, "-o", exe], check=True)
        _BIN["bin"] = exe
    return _BIN["bin"]


def host_decode(streams):
    """streams: list of (bytes, h, w, channels) -> list of (status, uint8 (c, h, w)).  Raises if the sanitizers report."""
    exe = host_decoder()
    d = tempfile.mkdtemp(prefix="jpeg_run_")
    try:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(streams)))
            for data, h, w, c in streams:
                f.write(struct.pack("<iiiq", h, w, c, len(data)))
                f.write(data)
        # without address-space randomisation: the AddressSanitizer runtime of older compilers cannot always place its
        # shadow memory when the kernel randomises mmap with more bits than it expects (a crash before main, no report)
        pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
        r = subprocess.run(pre + [exe, fin, fout], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
        buf = open(fout, "rb").read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res, p = [], 0
    for data, h, w, c in streams:
        st = struct.unpack_from("<i", buf, p)[0]
        p += 4
        res.append((st, np.frombuffer(buf, np.uint8, c * h * w, p).reshape(c, h, w)))
        p += c * h * w
    assert p == len(buf)
    return res


def broken_streams(cases, seed=0, flips=300):
    """Truncations at many cut points and a fixed-seed set of single-byte flips of a few fixture streams.
    -> list of (bytes, h, w, c, broken) with broken = True where the stream certainly cannot decode cleanly."""
    out = []
    pick = [c for c in cases if c["name"] in ("c420_225x223_q100", "gray_224_opt", "c422_61x45_opt_rst_blocks",
                                              "c420_96x72_rst_rows", "gray_17x31_rst_blocks", "c444_17x31_q75")]
    assert len(pick) == 6
    for c in pick:
        n = len(c["data"])
        for cut in sorted(set(np.linspace(0, n - 16, 24).astype(int).tolist())):
            out.append((c["data"][:cut], c["h"], c["w"], c["c"], True))
    rng = np.random.default_rng(seed)
    for _ in range(flips):
        c = pick[int(rng.integers(len(pick)))]
        b = bytearray(c["data"])
        pos = int(rng.integers(len(b)))
        b[pos] ^= int(rng.integers(1, 256))
        out.append((bytes(b), c["h"], c["w"], c["c"], False))
    return out


needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")


@needs_gxx
def test_host_core_matches_fixture_bit_exact():
    cases, _ = fixture()
    res = host_decode([(c["data"], c["h"], c["w"], c["c"]) for c in cases])
    for c, (st, got) in zip(cases, res):
        assert st == 0, (c["name"], st)
        assert np.array_equal(got, c["expect"]), (c["name"], int((got != c["expect"]).sum()))


@needs_gxx
def test_host_core_is_memory_safe_on_broken_streams():
    cases, _ = fixture()
    br = broken_streams(cases)
    res = host_decode([s[:4] for s in br])
    n_flip_bad = 0
    for (data, h, w, c, broken), (st, _) in zip(br, res):
        assert st in (0, 1, 2, 3, 4)
        if broken:
            assert st != 0, (len(data), h, w, c)
        else:
            n_flip_bad += st != 0
    assert n_flip_bad > 0                     # the flips do reach the error paths


@needs_gxx
def test_host_core_statuses_for_unsupported_and_wrong_size():
    cases, extra = fixture()
    c = cases[0]
    res = host_decode([(extra["progressive"], 224, 224, 3), (extra["png"], 224, 224, 1),
                       (c["data"], c["h"] + 1, c["w"], c["c"]), (b"", 8, 8, 1)])
    assert [r[0] for r in res] == [2, 4, 3, 4]            # PNG and empty stream: fatal in libjpeg (cv2 returns None)


FOLDER = "Ahmad_American"


def make_tree(root, frames=(11, 12, 13)):
    """An on-disk dataset tree of fixture bytes (no encoder needed): 224 x 224 colour frames (4:2:0, 4:4:4 and one
    progressive, which the GPU path leaves to the host), grayscale JPEG flow, JPEG ground truth and one PNG ground truth.
    -> STDataset positional arguments."""
    cases, extra = fixture()
    by = {c["name"]: c["data"] for c in cases}
    grays = [by["gray_224x224_q95"], by["gray_224x224_q50"], by["gray_224_opt"]]
    images = [by["c420_224x224_q95"], extra["progressive"], by["c444_224x224_q50"]]
    gts = [(by["gray_224x224_q50"], "jpg"), (extra["png"], "png"), (by["gray_224_opt"], "jpg")]
    for d in ("flow/" + FOLDER, "img", "gt", "fs"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    k = 0
    for n in range(min(frames) - 9, max(frames) + 1):
        for ax in "xy":
            with open(os.path.join(root, "flow", FOLDER, f"flow_{ax}_{n:05d}.jpg"), "wb") as f:
                f.write(grays[k % 3])
            k += 1
    names, gtn = [], []
    for i, n in enumerate(frames):
        names.append(f"{FOLDER}_img_{n:05d}.jpg")
        gtn.append(f"{FOLDER}_000000_{n:05d}.{gts[i % 3][1]}")
        with open(os.path.join(root, "img", names[-1]), "wb") as f:
            f.write(images[i % 3])
        with open(os.path.join(root, "gt", gtn[-1]), "wb") as f:
            f.write(gts[i % 3][0])
    np.savetxt(os.path.join(root, "fs", "a.txt"), np.array([0.0, 1.0, 0.0]))
    return (os.path.join(root, "flow"), os.path.join(root, "img"), os.path.join(root, "gt"), [FOLDER], names, gtn,
            ["a.txt"], os.path.join(root, "fs"))


def test_sniff_classifies_fixtures():
    from egaze_amd.data.STdatas import sniff
    cases, extra = fixture()
    for c in cases:
        assert sniff(c["data"]) == (c["h"], c["w"]), c["name"]
    assert sniff(extra["progressive"]) is None and sniff(extra["png"]) is None
    d = cases[0]["data"]
    assert sniff(d[:20]) is None and sniff(b"") is None
    # Adobe APP14 with transform 0 (RGB) after SOI: host decode
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    c3 = next(c for c in cases if c["c"] == 3)["data"]
    assert sniff(c3[:2] + adobe + c3[2:]) == sniff(c3)             # JFIF present: YCbCr regardless
    nojfif = c3[:2] + c3[2 + 2 + int.from_bytes(c3[4:6], "big"):]  # drop the APP0 segment
    assert c3[2:4] == b"\xff\xe0" and sniff(nojfif) is not None
    assert sniff(nojfif[:2] + adobe + nojfif[2:]) is None


def test_gpu_mode_sample_and_collate(tmp_path):
    """decode='gpu' samples carry bytes; the worker's collate builds one buffer + table, host-decodes what the kernel does
    not take (the progressive frame, the PNG ground truth) into the right planes."""
    import torch
    from egaze_amd.data.STdatas import STDataset, collate_gpu
    _, extra = fixture()
    args = make_tree(str(tmp_path))
    ds = STDataset(*args, raw_u8=True, decode="gpu")
    assert ds.collate_fn is collate_gpu and STDataset(*args).collate_fn is None
    batch = [ds[i] for i in range(3)]
    b = collate_gpu(batch)
    B, n = 3, b["jpeg_n"]
    assert b["jpeg_hw"] == (224, 224) and b["batch"] == B
    assert n == B * 22 - 2 and b["jpeg_n3"] == 2           # 22 files per sample; 2 colour JPEGs, 2 files host-decoded
    blob = b["jpeg_blob"]
    off = blob[:8 * (n + 1)].view(torch.int64).tolist()
    planes = blob[8 * (n + 1):8 * (2 * n + 1)].view(torch.int64).tolist()
    chans = blob[8 * (2 * n + 1):8 * (2 * n + 1) + 4 * n].view(torch.int32).tolist()
    head = 8 * (2 * n + 1) + 4 * n
    head += -head % 8
    data = blob[head:].numpy().tobytes()
    assert off[0] == 0 and off[-1] == len(data)
    expect = []
    for s_i, s in enumerate(batch):
        for k, path in enumerate(s["files"]):
            plane = 3 * s_i if k == 0 else (3 * B + 20 * s_i + k - 1 if k <= 20 else 23 * B + s_i)
            expect.append((path, plane, 3 if k == 0 else 1))
    got = list(zip(b["jpeg_files"], planes, chans))
    for i, (path, plane, ch) in enumerate(got):
        assert data[off[i]:off[i + 1]] == open(path, "rb").read()
        assert (path, plane, ch) in expect
    host_paths = sorted(set(e[0] for e in expect) - set(b["jpeg_files"]))
    assert [os.path.basename(p) for p in host_paths] == [f"{FOLDER}_000000_00012.png", f"{FOLDER}_img_00012.jpg"]
    assert b["host_index"].tolist() == [3, 4, 5, 23 * B + 1]
    assert np.array_equal(b["host_planes"][:3].numpy(), extra["progressive_bgr"])
    assert np.array_equal(b["host_planes"][3:].numpy(), extra["png_gray"])
    assert b["imname"] == [s["imname"] for s in batch] and b["fixsac"].shape == (B, 1)


def test_gpu_mode_reads_only_the_fields_in_use(tmp_path):
    """The single-stream scripts set gpu_fields: the other fields' files are neither read nor shipped."""
    from egaze_amd.data.STdatas import STDataset, collate_gpu
    ds = STDataset(*make_tree(str(tmp_path)), raw_u8=True, decode="gpu")
    ds.gpu_fields = ("image", "gt")
    b = collate_gpu([ds[i] for i in range(3)])
    assert b["jpeg_n"] == 3 * 2 - 2 and all("flow" not in os.path.basename(f) for f in b["jpeg_files"])
    ds.gpu_fields = ("flow", "gt")
    b = collate_gpu([ds[i] for i in range(3)])
    assert b["jpeg_n"] == 3 * 21 - 1 and b["jpeg_n3"] == 0
