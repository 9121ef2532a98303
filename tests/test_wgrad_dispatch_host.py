"""Host side of the 3x3 weight gradient (csrc/conv3x3_wgrad.hip) under AddressSanitizer + UBSan: every guard of
egz_conv3x3_wgrad rejects its arguments before any launch with the message the callers match, egz_conv3x3_wgrad_ws_bytes
returns the recorded size at every point of a sweep over geometries and flags, and at every one of those points the launch
rejects a workspace four bytes short of it -- the launch never needs less than the size query reports.  The host half of the
source is compiled alone (no device code) and run on the CPU.  No GPU needed.

tests/golden/wgrad_ws_bytes.npz holds the sweep as the same driver recorded it when built against the source before the size
query and the launch shared one plan (`python tests/test_wgrad_dispatch_host.py <csrc of that checkout> <out.npz>`)."""
import os
import platform
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egocentric-gaze-prediction_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "wgrad_guard_driver.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_ws_bytes.npz")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
RECORD = np.dtype([("args", "<i4", (6,)), ("ws_bytes", "<u8")])      # B, H, W, C, K, flags

NULL = "egz_conv3x3_wgrad: null pointer"
XBN = ("egz_conv3x3_wgrad: a deferred-BatchNorm operand (x_bn) exists on the narrow split-half kernel only "
       "(C, K <= 32, W % 16 == 0, plain conv)")
EVEN = "egz_conv3x3_wgrad: upsampled output must be even"
PRE = ("egz_conv3x3_wgrad: a pre-split x / dy operand (flags 0x8000 / 0x10000) needs the split-half 9-tap kernel's geometry "
       "(egz_conv3x3_wgrad_presplit_ok), f16 x3 (dy_absmax, x_absmax) and a plain conv")
SMALL = "egz_conv3x3_wgrad: workspace too small"
EXPECT = {
    "null": NULL, "null_ws": NULL,
    "xbn_wide": XBN, "xbn_width12": XBN, "xbn_ups": XBN, "xbn_pertap": XBN, "xbn_c6": XBN, "xbn_f32": XBN,
    "c6": "egz_conv3x3_wgrad: C=6 K=8 must be multiples of 4", "k0": "egz_conv3x3_wgrad: C=8 K=0 must be multiples of 4",
    "ups_odd_h": EVEN, "ups_odd_w": EVEN,
    "xpre_ups": PRE, "dpre_ups": PRE, "xpre_no_dy_absmax": PRE, "dpre_no_dy_absmax": PRE, "xpre_no_x_absmax": PRE,
    "xpre_f32": PRE, "xpre_xbn": PRE, "dpre_xbn": PRE, "xpre_k32": PRE, "dpre_c32": PRE, "xpre_width36": PRE, "xpre_4gib": PRE,
    "ws_small": SMALL, "ws_small_ups_f32": SMALL,
}


def _hipcc():
    exe = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(exe):
        pytest.fail("hipcc not found: the host build of the dispatch needs the compiler the library is built with")
    return exe


def _run_driver(csrc):
    """Builds the driver against the sources in ``csrc`` and runs it -> (guards: name -> (rc, message), sweep records,
    (calls, not rejected) of the short-workspace pass)."""
    d = tempfile.mkdtemp(prefix="wgrad_guard_")
    try:
        obj, exe, sweep = os.path.join(d, "guard.o"), os.path.join(d, "guard"), os.path.join(d, "sweep.bin")
        host_san = [f for s in SAN for f in ("-Xarch_host", s)]
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g",
                        "-fno-omit-frame-pointer", *host_san, "-I", csrc, "-c", DRIVER, "-o", obj], check=True)
        # the device binary of the translation unit is defined as absent: see tests/test_x3s_dispatch_host.py
        syms = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout.split()
        fatbin = [s for s in syms if s.startswith("__hip_fatbin_") and not s.startswith("__hip_fatbin_wrapper")]
        assert len(fatbin) == 1, fatbin
        subprocess.run([_hipcc(), "--offload-arch=gfx950", *SAN, obj, f"-Wl,--defsym={fatbin[0]}=0", "-o", exe], check=True)
        # (without address-space randomisation: see tests/test_jpeg_host.py)
        pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
        r = subprocess.run(pre + [exe, sweep], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
        records = np.fromfile(sweep, dtype=RECORD) if os.path.exists(sweep) else None
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    guards, short4 = {}, None
    for line in r.stdout.splitlines():
        kind, *rest = line.split("\t")
        if kind == "guard":
            guards[rest[0]] = (int(rest[1]), rest[2])
        elif kind == "short4":
            short4 = (int(rest[0]), int(rest[1]))
    return guards, records, short4


@pytest.fixture(scope="module")
def report():
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer build of host code: runs where there is no GPU")
    return _run_driver(CSRC)


def test_driver_covers_every_expected_guard(report):
    assert sorted(report[0]) == sorted(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_guard_rejects_before_launch(report, name):
    rc, msg = report[0][name]
    assert rc == 1, (name, rc, msg)             # hipErrorInvalidValue: an argument check, not a launch failure
    assert msg == EXPECT[name]


def test_ws_bytes_sweep_matches_recorded(report):
    """3 batch sizes x 16 images x 8 C x 7 K x {f32, split} x {plain, upsampled (even images)} x 5 A/B variants, and four
    points past the 4 GiB rule: the same points, in the same order, with the same sizes."""
    records = report[1]
    want = np.load(GOLDEN)
    assert len(records) == 3 * (16 + 12) * 8 * 7 * 2 * 5 + 4
    assert np.array_equal(records["args"], want["args"])
    diff = np.flatnonzero(records["ws_bytes"] != want["ws_bytes"])
    assert diff.size == 0, (diff.size, [(records["args"][i].tolist(), int(records["ws_bytes"][i]), int(want["ws_bytes"][i]))
                                        for i in diff[:5]])


def test_workspace_short_by_four_rejected(report):
    """Two calls (bf16 x3 / f32, and f16 x3 with both abs-max operands) per sweep point, each "workspace too small"."""
    records, (calls, wrong) = report[1], report[2]
    assert calls == 2 * len(records)
    assert wrong == 0


if __name__ == "__main__":                      # records the sweep of the sources in argv[1] as argv[2]
    _, rec, _ = _run_driver(sys.argv[1])
    np.savez_compressed(sys.argv[2], args=rec["args"], ws_bytes=rec["ws_bytes"])
