"""Host side of the streamed 3x3 convolution's launch dispatch (csrc/conv3x3_igemm_x3s.hip) under AddressSanitizer + UBSan:
every guard of egz_conv3x3_fwd_streamed rejects its arguments before any launch, with the message the callers and the GPU tests
match.  The host half of the source is compiled alone (no device code) and run on the CPU.  No GPU needed."""
import os
import platform
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egocentric-gaze-prediction_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "x3s_guard_driver.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PRE = ("egz_conv3x3_fwd_streamed: a pre-split operand needs mode 0, dtype 1, epi 0 / 2 / 5, K % 64 == 0, C % 32 == 0 and "
       "x_absmax")
MASK32 = "egz_conv3x3_fwd_streamed: the mask epilogue is not built for 32-column tiles"
BNSUMS = ("egz_conv3x3_fwd_streamed: epi 5 (BatchNorm sums) needs mode 0, the narrow geometry (C, K <= 32, H and W multiples "
          "of 16) or K % 64 == 0, mask_src = the pre-BN conv output of the layer below, bn_coef, stat_partial and no bias")
UPSF = "egz_conv3x3_fwd_streamed: the upsample forward has the bias and bias + ReLU epilogues only"
BN_IN = ("egz_conv3x3_fwd_streamed: a deferred-BatchNorm input (bn_coef) exists on the narrow persistent kernel only (C, K <= "
         "32, H and W multiples of 16); minmax_out needs epi 2 and that geometry or K % 64 == 0")
EXPECT = {
    "null": "egz_conv3x3_fwd_streamed: null pointer",
    "bf16_p2": "egz_conv3x3_fwd_streamed: dtype 0x10 (two products) goes with f16 (dtype 0x11)",
    "pre_epi1": PRE, "pre_bf16": PRE, "pre_k32": PRE,
    "mask_32col": MASK32, "mask_narrow_geometry": MASK32,
    "mask_no_src": "egz_conv3x3_fwd_streamed: mask epilogue needs mask_src and absmax_out and takes no bias",
    "bnsums_mode1": BNSUMS, "bnsums_32col": BNSUMS,
    "upsf_stats": UPSF, "upsf_stats_k128": UPSF,
    "upsf_bf16": "egz_conv3x3_fwd_streamed: the upsample forward runs in f16 x3 (dtype 1)",
    "stats_no_rows": "egz_conv3x3_fwd_streamed: stats / mask epilogue needs stat_partial",
    "geometry": "egz_conv3x3_fwd_streamed: geometry B=2 H=16 W=16 C=30 K=128 mode=0 is not covered (see egz_conv3x3_streamed_ok)",
    "bad_epi": "egz_conv3x3_fwd_streamed: bad dtype / epilogue",
    "absmax_32col": "egz_conv3x3_fwd_streamed: the abs-max epilogue exists for 64- and 128-column tiles only (K % 64 == 0)",
    "bn_in_wide": BN_IN, "minmax_epi0": BN_IN,
    "splitk_epi3": "egz_conv3x3_fwd_streamed_splitk: bad dtype / epilogue",
    "splitk_nsplit": "egz_conv3x3_fwd_streamed_splitk: nsplit=5 outside [2, C/32]",
}


def _hipcc():
    exe = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(exe):
        pytest.fail("hipcc not found: the host build of the dispatch needs the compiler the library is built with")
    return exe


@pytest.fixture(scope="module")
def guard_report():
    """name -> (return code, error message) of every call the driver makes."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer build of host code: runs where there is no GPU")
    d = tempfile.mkdtemp(prefix="x3s_guard_")
    try:
        obj, exe = os.path.join(d, "guard.o"), os.path.join(d, "guard")
        host_san = [f for s in SAN for f in ("-Xarch_host", s)]
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g",
                        "-fno-omit-frame-pointer", *host_san, "-I", CSRC, "-c", DRIVER, "-o", obj], check=True)
        # Relies on two behaviours of hipcc / the HIP runtime: (1) an --offload-host-only object refers to the device binary
        # of its translation unit through ONE undefined symbol __hip_fatbin_<hash> (besides its own __hip_fatbin_wrapper*),
        # and (2) registering a null device binary at start-up is harmless as long as nothing is launched.  No call of the
        # driver reaches a launch, so the symbol is defined as absent.  If a ROCm upgrade changes either, this fixture fails
        # in its build or at the driver's start-up -- that is the fixture, not the dispatch.
        syms = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout.split()
        fatbin = [s for s in syms if s.startswith("__hip_fatbin_") and not s.startswith("__hip_fatbin_wrapper")]
        assert len(fatbin) == 1, fatbin
        subprocess.run([_hipcc(), "--offload-arch=gfx950", *SAN, obj, f"-Wl,--defsym={fatbin[0]}=0", "-o", exe], check=True)
        # (without address-space randomisation: see tests/test_jpeg_host.py)
        pre = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
        r = subprocess.run(pre + [exe], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = {}
    for line in r.stdout.splitlines():
        name, rc, msg = line.split("\t")
        rep[name] = (int(rc), msg)
    return rep


def test_driver_covers_every_expected_guard(guard_report):
    assert sorted(guard_report) == sorted(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_guard_rejects_before_launch(guard_report, name):
    rc, msg = guard_report[name]
    assert rc == 1, (name, rc, msg)             # hipErrorInvalidValue: an argument check, not a launch failure
    assert msg == EXPECT[name]
