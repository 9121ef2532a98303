"""Host build of the JPEG round-trip core (csrc/jpeg_roundtrip_core.h) under AddressSanitizer + UBSan: the per-block chain
FDCT -> quantise -> dequantise -> IDCT, run over whole images, gives the pixels Pillow's save(JPEG, quality) -> open gives,
exactly -- on the grey images of test_jpeg_enc_host.random_cases and on 224 x 224 at qualities 1, 50, 75, 95 and 100.  Pillow
runs live.  No GPU needed."""
import io
import os
import platform
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from test_jpeg_enc_host import random_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egocentric-gaze-prediction_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "jpeg_roundtrip_host_driver.cpp")

_BIN = {}

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")


def pil_roundtrip(a, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a)).save(b, format="JPEG", quality=quality)
    b.seek(0)
    im = Image.open(b)
    assert im.mode == "L"
    return np.asarray(im)


def host_binary():
    if "bin" not in _BIN:
        d = tempfile.mkdtemp(prefix="jpeg_roundtrip_host_")
        exe = os.path.join(d, "jpeg_roundtrip_host")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", CSRC, DRIVER, "-o", exe], check=True)
        _BIN["bin"] = exe
    return _BIN["bin"]


def host_roundtrip(images):
    """images: list of ((H, W) uint8 array, quality) -> list of (return code, (H, W) array or None)."""
    exe = host_binary()
    d = tempfile.mkdtemp(prefix="jpeg_roundtrip_run_")
    try:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(images)))
            for a, q in images:
                f.write(struct.pack("<iii", a.shape[0], a.shape[1], q))
                f.write(np.ascontiguousarray(a).tobytes())
        # without address-space randomisation: see tests/test_jpeg_host.py
        pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
        r = subprocess.run(pre + [exe, fin, fout], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
        buf = open(fout, "rb").read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res, p = [], 0
    for a, _ in images:
        rc = struct.unpack_from("<i", buf, p)[0]
        p += 4
        if rc == 0:
            res.append((rc, np.frombuffer(buf, np.uint8, a.size, p).reshape(a.shape)))
            p += a.size
        else:
            res.append((rc, None))
    assert p == len(buf)
    return res


def contents_224(rng):
    y, x = np.mgrid[0:224, 0:224]
    return {
        "noise": rng.integers(0, 256, (224, 224)),
        "smooth": x * 0.7 + y * 0.4 + rng.normal(0, 2, (224, 224)),
        "two-level": rng.integers(0, 2, (224, 224)) * 255,
        "near-saturated": np.where(rng.random((224, 224)) < 0.5, rng.integers(0, 4, (224, 224)),
                                   rng.integers(252, 256, (224, 224))),
    }


def cases():
    grey = [(a, q) for a, q in random_cases() if a.ndim == 2]
    rng = np.random.default_rng(77)
    big = [(np.clip(a, 0, 255).astype(np.uint8), q) for q in (1, 50, 75, 95, 100) for a in contents_224(rng).values()]
    return grey, big


@needs_gxx
def test_host_core_equals_pillow_encode_then_decode():
    grey, big = cases()
    assert len(grey) == 120 and len(big) == 20
    assert {q for _, q in grey} >= {1, 50, 100}
    assert any(a.shape[0] % 8 and a.shape[1] % 8 for a, _ in grey) and any(min(a.shape) < 8 for a, _ in grey)
    imgs = grey + big
    bad = []
    for (a, q), (rc, got) in zip(imgs, host_roundtrip(imgs)):
        assert rc == 0
        want = pil_roundtrip(a, q)
        if not np.array_equal(got, want):
            bad.append((a.shape, q, int((got != want).sum())))
    assert not bad, (len(bad), bad[:10])


@needs_gxx
def test_host_core_refuses_bad_arguments():
    a = np.zeros((8, 8), np.uint8)
    res = host_roundtrip([(a, 0), (a, 101), (np.zeros((1, 4097), np.uint8), 95)])
    assert [r[0] for r in res] == [-1, -1, -1]
