"""Host side of the BatchNorm / ReLU / pool passes (csrc/bn_pool.hip) and of the first-layer convolution (csrc/conv_first.hip)
under AddressSanitizer + UBSan: every guard of the entry points listed in ENTRY_POINTS rejects its arguments before any launch
with the message the callers match, the size queries return the recorded values at every point of their grids, and at every
one of those points each entry point that takes a workspace rejects one that is 8 bytes short of what it needs.  The host half
of the two sources is compiled alone (no device code) and run on the CPU.  No GPU needed.

tests/golden/bn_host_sizes.npz holds the sweep as the same driver recorded it when built against the sources before the
workspace layout, the fold and the reduction grid had one definition each
(`python tests/test_bn_dispatch_host.py <csrc of that checkout> <out.npz>`)."""
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
DRIVER = os.path.join(ROOT, "tests", "bn_guard_driver.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bn_host_sizes.npz")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
RECORD = np.dtype([("args", "<i4", (6,)), ("value", "<u8")])      # query (enum Query of the driver), its arguments, 0-padded
BN_WS, BN_BWD_WS, RELU_BIAS_WS, FIRST_BWD_WS, FIRST_WGRAD_WS, FIRST_STAT_ROWS = range(6)

ENTRY_POINTS = ["egz_bn_finalize", "egz_bn_finalize_bound", "egz_bn_finalize_deferred", "egz_bn_eval_coeffs",
                "egz_bn_relu_pool_fwd", "egz_bn_relu_pool_fwd_presplit", "egz_bn_relu_pool_bwd", "egz_bn_relu_pool_bwd_presplit",
                "egz_bn_bwd_first_wgrad", "egz_relu_bwd_bias", "egz_colsum", "egz_colsum_f64", "egz_conv_first_fwd",
                "egz_conv_first_wgrad"]

# the messages, as the sources had them before the entry points shared their implementations
BWD = "egz_bn_relu_pool_bwd: "
BWD_NULL, BWD_EVEN = BWD + "null pointer", BWD + "pooled map must be even"
BWD_SUMS = BWD + "precomputed sums need sums_rows > 0 and no pooling"
BWDP = "egz_bn_relu_pool_bwd_presplit: needs absmax, y_minmax, dout_absmax and K % 64 == 0, K <= 512"
DEF_K = "egz_bn_finalize_deferred: K=%d must be 16, 32 or 64"
FWG = "egz_bn_bwd_first_wgrad: "
FWG_COVERS = FWG + "covers C <= 3 input channels and 32 / 64 filters (got %d -> %d)"
C64 = "egz_colsum_f64: bad arguments"
CFF_MM = ("egz_conv_first_fwd: minmax_out / minmax_ordered exist on the direct kernel only (C <= 3 -> 32 / 64 filters, "
          "with stat_partial)")
CFW_CIN = "egz_conv_first_wgrad: Cin=%d unsupported (1..3 or 18..21)"
BWD_WS_64 = (1024 + 64) * 2 * 64 * 8 + 2 * 64 * 4           # [BWD_BLOCKS + RED_ROWS][2][K] fp64 + 2 [K] fp32 at K = 64
FWG_WS_2_32 = (1024 + 64) * 2 * 32 * 8 + 2 * 32 * 4 + 1024 * 32 * 2 * 9 * 4     # the same at K = 32 + [FWG_BLOCKS][K][C][9] fp32
EXPECT = {
    "fin_null_stat": "egz_bn_finalize: null pointer", "fin_null_shift": "egz_bn_finalize: null pointer",
    "fin_null_ws": "egz_bn_finalize: null pointer", "fin_ws_small": "egz_bn_finalize: workspace too small",
    "fin_unpaired": "egz_bn_finalize: running stats must come in pairs",
    "finb_null_stat": "egz_bn_finalize_bound: null pointer", "finb_null_minmax": "egz_bn_finalize_bound: null pointer",
    "finb_null_absmax": "egz_bn_finalize_bound: null pointer",
    "finb_k32": "egz_bn_finalize_bound: K=32 must be a multiple of 64",
    "finb_ws_small": "egz_bn_finalize_bound: workspace too small",
    "finb_unpaired": "egz_bn_finalize_bound: running stats must come in pairs",
    "find_null_stat": "egz_bn_finalize_deferred: null pointer", "find_null_minmax": "egz_bn_finalize_deferred: null pointer",
    "find_null_absmax": "egz_bn_finalize_deferred: null pointer",
    "find_k128": DEF_K % 128, "find_rows0": DEF_K % 32, "find_mm_rows0": DEF_K % 32,
    "find_unpaired": "egz_bn_finalize_deferred: running stats must come in pairs",
    "eval_null_mean": "egz_bn_eval_coeffs: null pointer", "eval_null_shift": "egz_bn_eval_coeffs: null pointer",
    "fwd_null_y": "egz_bn_relu_pool_fwd: null pointer", "fwd_null_out": "egz_bn_relu_pool_fwd: null pointer",
    "fwd_k6": "egz_bn_relu_pool_fwd: K=6 must be a multiple of 4",
    "fwd_pool_odd_h": "egz_bn_relu_pool_fwd: pooled map must be even",
    "fwd_pool_odd_w": "egz_bn_relu_pool_fwd: pooled map must be even",
    "fwdp_null_y": "egz_bn_relu_pool_fwd_presplit: null pointer",
    "fwdp_null_absmax": "egz_bn_relu_pool_fwd_presplit: null pointer",
    "fwdp_k6": "egz_bn_relu_pool_fwd_presplit: K=6 must be a multiple of 4",
    "fwdp_pool_odd_h": "egz_bn_relu_pool_fwd_presplit: pooled map must be even",
    "fwdp_pool_odd_w": "egz_bn_relu_pool_fwd_presplit: pooled map must be even",
    "bwd_null_y": BWD_NULL, "bwd_null_dy": BWD_NULL, "bwd_null_ws": BWD_NULL,
    "bwd_sums_rows0": BWD_SUMS, "bwd_sums_pool": BWD_SUMS,
    "bwd_k6": BWD + "K=6 must be a multiple of 4, <= 1024", "bwd_k1028": BWD + "K=1028 must be a multiple of 4, <= 1024",
    "bwd_pool_odd_h": BWD_EVEN, "bwd_pool_odd_w": BWD_EVEN,
    "bwd_ws_small": BWD + "workspace too small (%d < %d)" % (BWD_WS_64 - 8, BWD_WS_64),
    "bwdp_null_absmax": BWDP, "bwdp_null_minmax": BWDP, "bwdp_null_dout_absmax": BWDP, "bwdp_k32": BWDP, "bwdp_k576": BWDP,
    # past its own guard the pre-split form shares the implementation, which reports under the plain entry point's name
    "bwdp_null_y": BWD_NULL, "bwdp_sums_pool": BWD_SUMS, "bwdp_pool_odd": BWD_EVEN,
    "bwdp_ws_small": BWD + "workspace too small (%d < %d)" % (BWD_WS_64 - 8, BWD_WS_64),
    "fwg_null_x": FWG + "null pointer", "fwg_null_dw": FWG + "null pointer", "fwg_null_ws": FWG + "null pointer",
    "fwg_k16": FWG_COVERS % (2, 16), "fwg_c4": FWG_COVERS % (4, 64), "fwg_c0": FWG_COVERS % (0, 32),
    "fwg_b0": FWG + "bad shape", "fwg_w0": FWG + "bad shape", "fwg_2gi": FWG + "bad shape",
    "fwg_sums_rows0": FWG + "sums need sums_rows > 0",
    "fwg_ws_small": FWG + "workspace too small (%d < %d)" % (FWG_WS_2_32 - 8, FWG_WS_2_32),
    "rbb_null_db": "egz_relu_bwd_bias: null pointer", "rbb_null_ws": "egz_relu_bwd_bias: null pointer",
    "rbb_k6": "egz_relu_bwd_bias: K=6 must be a multiple of 4, <= 1024",
    "rbb_k1028": "egz_relu_bwd_bias: K=1028 must be a multiple of 4, <= 1024",
    "rbb_ws_small": "egz_relu_bwd_bias: workspace too small",
    "colsum_null_x": "egz_colsum: null pointer", "colsum_null_ws": "egz_colsum: null pointer",
    "colsum_ws_small": "egz_colsum: workspace too small",
    "colsum64_null_part": C64, "colsum64_null_ws": C64, "colsum64_rows0": C64, "colsum64_cols0": C64, "colsum64_nout0": C64,
    "colsum64_nout_wide": C64, "colsum64_ws_small": "egz_colsum_f64: workspace too small",
    "cff_null_x": "egz_conv_first_fwd: null pointer", "cff_null_y": "egz_conv_first_fwd: null pointer",
    "cff_mm_no_stat": CFF_MM, "cff_mmo_no_stat": CFF_MM, "cff_mm_c20": CFF_MM, "cff_mm_2gi": CFF_MM,
    "cff_k16": "egz_conv_first_fwd: Cout must be 64 or 32 (got 16)",
    "cff_c0": "egz_conv_first_fwd: bad shape", "cff_c65": "egz_conv_first_fwd: bad shape",
    "cff_h0": "egz_conv_first_fwd: bad shape",
    "cfw_null_dy": "egz_conv_first_wgrad: null pointer", "cfw_null_ws": "egz_conv_first_wgrad: null pointer",
    "cfw_k16": "egz_conv_first_wgrad: Cout must be 64 or 32 (got 16)",
    "cfw_c4": CFW_CIN % 4, "cfw_c22": CFW_CIN % 22, "cfw_ws_small": "egz_conv_first_wgrad: workspace too small",
}


def _hipcc():
    exe = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(exe):
        pytest.fail("hipcc not found: the host build of the dispatch needs the compiler the library is built with")
    return exe


def _run_driver(csrc):
    """Builds the driver against the sources in ``csrc`` and runs it -> (guards: name -> (rc, message), sweep records,
    (calls, not rejected) of the short-workspace pass)."""
    d = tempfile.mkdtemp(prefix="bn_guard_")
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
    guards, short8 = {}, None
    for line in r.stdout.splitlines():
        kind, *rest = line.split("\t")
        if kind == "guard":
            guards[rest[0]] = (int(rest[1]), rest[2])
        elif kind == "short8":
            short8 = (int(rest[0]), int(rest[1]))
    return guards, records, short8


@pytest.fixture(scope="module")
def report():
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer build of host code: runs where there is no GPU")
    return _run_driver(CSRC)


def test_driver_covers_every_expected_guard(report):
    assert sorted(report[0]) == sorted(EXPECT)


def test_every_guard_of_every_entry_point_is_expected():
    """Each EGZ_CHECK_ARG between the opening line of a listed entry point (or of the implementation it forwards to) and its
    closing brace has a message that some case of EXPECT produces: a guard added later needs a case here."""
    import re
    impls = {"egz_bn_finalize": "bn_finalize_impl", "egz_bn_finalize_bound": "bn_finalize_impl",
             "egz_bn_relu_pool_fwd": "bn_relu_pool_fwd_impl", "egz_bn_relu_pool_fwd_presplit": "bn_relu_pool_fwd_impl",
             "egz_bn_relu_pool_bwd": "bn_relu_pool_bwd_impl", "egz_bn_relu_pool_bwd_presplit": "bn_relu_pool_bwd_impl"}
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("bn_pool.hip", "conv_first.hip"))
    seen = 0
    for name in ENTRY_POINTS:
        for fn in {name, impls.get(name, name)}:
            m = re.search(r"^(?:EGZ_API |static )?int %s\(.*?^}" % fn, src, re.S | re.M)
            assert m, fn
            for fmt in re.findall(r'EGZ_CHECK_ARG\(.*?,\s*"((?:[^"\\]|\\.)*)"', m.group(0), re.S):
                # printf conversions become wildcards, "%%" a literal per cent sign
                parts = re.split(r"%(?:zu|d|s)", fmt.replace("%%", "\0"))
                pat = ".*".join(re.escape(p.replace("\0", "%")) for p in parts)
                assert any(re.fullmatch(pat, msg) for msg in EXPECT.values()), (fn, fmt)
                seen += 1
    assert seen >= 40


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_guard_rejects_before_launch(report, name):
    rc, msg = report[0][name]
    assert rc == 1, (name, rc, msg)             # hipErrorInvalidValue: an argument check, not a launch failure
    assert msg == EXPECT[name]


def test_size_queries_match_recorded(report):
    """egz_bn_ws_bytes, egz_bn_relu_pool_bwd_ws_bytes and egz_relu_bwd_bias_ws_bytes at K = 4 ... 1024 step 4,
    egz_bn_bwd_first_wgrad_ws_bytes at C 1..3 x K {32, 64}, egz_conv_first_wgrad_ws_bytes at 3 batch sizes x 12 images x 8 Cin
    and egz_conv_first_stat_rows_for at those x K {32, 64}: the same points, in the same order, with the same values."""
    records = report[1]
    want = np.load(GOLDEN)
    assert len(records) == 3 * 256 + 6 + 3 * 12 * 8 * (1 + 2)
    assert [int((records["args"][:, 0] == q).sum()) for q in range(6)] == [256, 256, 256, 6, 288, 576]
    assert np.array_equal(records["args"], want["args"])
    diff = np.flatnonzero(records["value"] != want["value"])
    assert diff.size == 0, (diff.size, [(records["args"][i].tolist(), int(records["value"][i]), int(want["value"][i]))
                                        for i in diff[:5]])


def test_workspace_short_by_eight_rejected(report):
    """Per K of the grid: egz_bn_finalize, egz_colsum, egz_colsum_f64, egz_relu_bwd_bias and egz_bn_relu_pool_bwd (with and
    without sums), and where K % 64 == 0 egz_bn_finalize_bound and (K <= 512) egz_bn_relu_pool_bwd_presplit (with and without
    sums); egz_bn_bwd_first_wgrad with and without sums per (C, K); egz_conv_first_wgrad with 32 and 64 filters per geometry
    whose Cin it covers (6 of the 8).  Each "workspace too small"."""
    (calls, wrong) = report[2]
    assert calls == 256 * 6 + 16 + 2 * 8 + 6 * 2 + 3 * 12 * 6 * 2
    assert wrong == 0


if __name__ == "__main__":                      # records the sweep of the sources in argv[1] as argv[2]
    _, rec, _ = _run_driver(sys.argv[1])
    np.savez_compressed(sys.argv[2], args=rec["args"], value=rec["value"])
