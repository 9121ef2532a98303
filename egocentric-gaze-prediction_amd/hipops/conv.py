"""3x3 convolutions: arithmetic policy, forward / data-gradient / weight-gradient launches, the first layer."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_STATS, LIB, PROF, _out, _p, _req, _stream
from .absmax import _new_absmax, _want_absmax, _want_fwd_absmax

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# hipops.PRECISION: arithmetic of the wide convolutions (GEMM output channels % 128 == 0):
#   "split" (default) error-compensated split-half operands on the 16-bit MFMA path: f16 x3 (22 significant bits;
#           measured err 5e-7 of max|ref| per layer vs 8.6e-7 for the exact-f32 MFMA kernel) in the forward pass, the
#           data gradient and the weight gradient (GRAD_SPLIT below) -- conv3x3_igemm_x3.hip, conv3x3_wgrad.hip.
#   "f32"   exact-f32 MFMA everywhere (v_mfma_f32_32x32x2_f32); EGAZE_PRECISION=f32 selects it.
# hipops.GRAD_SPLIT: operand type of the split-half GRADIENT kernels (data and weight gradients):
#   "f16" (default) f16 x3, 22 significant bits (3e-7 per layer, the exact-f32 kernels' own level -- the reference's
#          arithmetic class): the gradient producers (BN / ReLU / fusion backward) also emit max |dy| and the conv backward
#          scales dy by the matching power of two so that gradients of 1e-3 ... 1e-13 stay representable;
#   "bf16" bf16 x3, 16 significant bits (5e-6 per layer), fp32 exponent range, no scaling: ~3 % faster per step, opt-in.
F32, F16X3, BF16X3 = 0, 1, 2


def precision_banner() -> str:
    """One line for the drivers' logs: which arithmetic the convolutions run in (an environment default, so say it)."""
    if _H.PRECISION != "split":
        return "egaze-hip arithmetic: exact-f32 MFMA (EGAZE_PRECISION=f32)"
    g = "f16x3, 22 bits, abs-max scaled" if _H.GRAD_SPLIT == "f16" else "bf16x3, 16 bits"
    return (f"egaze-hip arithmetic: split-half MFMA -- forward f16x3 (22 significant bits per operand), gradients {g}; fp32 "
            f"accumulate; EGAZE_PRECISION=f32 selects exact-f32 MFMA")


def conv_dtype(role: str, gemm_out: int, gemm_in: int, operand: Optional[torch.Tensor] = None) -> int:
    """dtype code for a conv launch under the current PRECISION policy (role: 'fwd' | 'dgrad').  ``operand`` = the gathered
    activation / gradient tensor: one of 4 GiB or more (B >= 320 at 224 x 224 x 64) stays on the 64-bit-addressed f32 kernels."""
    if _H.PRECISION != "split":
        return F32
    if operand is not None and operand.numel() * 4 >= _H._SPLIT_MAX_BYTES:
        return F32
    if gemm_out % 64 != 0 or gemm_in % 32 != 0:
        # narrow layers (the late-fusion stack: 32 -> 32 -> 8 channels): only the streamed-weight kernel's 32-column tile
        # takes them, and only for plain convs over an operand whose geometry it covers
        if not (operand is not None and operand.dim() == 4
                and LIB.egz_conv3x3_streamed_ok(operand.shape[0], operand.shape[1], operand.shape[2], gemm_in, gemm_out, 0)):
            return F32
    return F16X3 if (role == "fwd" or _H.GRAD_SPLIT == "f16") else BF16X3


# The switches of the package are plain constants unless they read the environment: the tests flip them with monkeypatch;
# round 4 removed the environment knobs of everything that was measured and decided.
# hipops.SPLITK: split-K form of the streamed kernel when a launch has too few pixel tiles to fill the chip
# (egz_conv3x3_streamed_splits): batch-1 inference runs its 28 x 28 / 14 x 14 layers on 8-28 of 512 block slots otherwise
# (tests: test_conv3x3_streamed_splitk, the whole-model gradient tests pin the summation order with it).


def conv_weight(w: torch.Tensor, role: str, dtype: int, x: torch.Tensor, gemm_out: int):
    """The packed weight a plain 3x3 conv launch over the NHWC operand ``x`` needs -> (packed buffer, streamed flag).
    Split-half launches whose geometry the streamed-weight kernel covers (egz_conv3x3_streamed_ok) use the MFMA-fragment-
    ordered packing; everything else the plane-ordered one.  role: 'fwd' | 'dgrad' | 'ups_dgrad' (x = the hi-res dy) |
    'ups_fwd' (x = the low-res input of [upsample x2 -> conv]; four phase convolutions, f16 x3 only)."""
    if dtype:
        B, H, W, C = x.shape
        if role == "ups_fwd":
            if dtype == F16X3 and LIB.egz_conv3x3_streamed_ok(B, 2 * H, 2 * W, C, gemm_out, 2):
                return _H.packed_weight(w, "ups_fwd_frag", dtype), True
        elif LIB.egz_conv3x3_streamed_ok(B, H, W, C, gemm_out, 1 if role == "ups_dgrad" else 0):
            return _H.packed_weight(w, role + "_frag", dtype), True
    return _H.packed_weight(w, role, dtype), False


# Pre-split activations (round 5).  Every split-half launch re-derives the f16 hi / lo pair of each staged
# activation from fp32 on the vector ALU -- ~3.5 instructions per staged float inside kernels that sit at the chip's power limit
# (timing-only builds without the split: conv fwd / dgrad -4 ... -5 %, weight gradient -7.5 % on the microbenchmark, more inside
# the step: profiles/r05_presplit_gonogo.txt).  Where the producer of an activation is a streaming pass that knows the
# tensor's EXACT abs-max before it writes the first element, it stores the pair instead of the fp32 value (same 4 bytes per
# element): the [BatchNorm -> ReLU (-> pool)] pass of an encoder block whose consumer is the next block's convolution.  The
# abs-max comes from the per-channel max / min of the conv output (atomic max in the conv's statistics epilogue) pushed through
# the BatchNorm's monotonic map by egz_bn_finalize_bound.  Consumers (the next conv's forward and weight gradient) then stage
# the pair without touching the vector ALU; the pair is bit-identical to the one they would have formed, so every result is.
# hipops.PRESPLIT = False keeps fp32 activations everywhere (test_presplit_activations_bit_identical flips it; the A/B was decided
# in round 5: -0.24 ms, bit-identical).
# Backward arithmetic (hipops.BWD_PRODUCTS).  Default (3): THREE MFMA products per MAC in the data and weight gradients too -- a_hi b_hi + a_hi b_lo +
# a_lo b_hi, both operands with 22 significant bits, fp32-class gradients (2e-7 per op): the arithmetic class of the reference's
# fp32 autograd (SP.py:132-138), and what every headline number is timed on.
# EGAZE_BWD_PRODUCTS=2 is an OPT-IN (like EGAZE_GRAD_SPLIT=bf16): the backward convolutions of the wide layers issue TWO products
# per MAC -- the operand that goes through LDS as a halo image (dy in a data gradient, x in a weight gradient) enters with its
# f16 hi half only, rounded to nearest (11 significant bits); the other keeps its 22 (csrc/egz_common.h, egz_f16p2).  Gradients
# move by ~2e-4 relative L2 per convolution, <= 1e-3 through the whole backward chain; the forward pass and with it every
# predicted map is untouched.  tests: test_backward_two_products, test_two_product_backward_whole_model, the `two_products`
# fixture; bench.py reports it as extra.bwd2, never as `value`.
P2_DTYPE = 0x10          # egz_conv3x3_fwd_streamed: dtype | 0x10
P2_WGRAD = 0x20000       # egz_conv3x3_wgrad: flags | 0x20000


def _note_p2(dtype: int, flops: float) -> None:
    """bench.py's roofline leg: algorithmic FLOPs of the conv launches that ran on two products (to price the family's MFMA work)."""
    if _p2(dtype) != dtype:
        PROF.note_flops("two_product_conv", flops)


def _p2(dtype: int) -> int:
    """dtype of a data-gradient launch on the streamed kernel: the two-product bit where the knob and the type allow it."""
    return dtype | P2_DTYPE if (_H.BWD_PRODUCTS == 2 and dtype == F16X3) else dtype


PRESPLIT_STATS = {"produced": 0, "fwd": 0, "wgrad": 0, "grad_produced": 0, "dgrad": 0, "wgrad_dy": 0}


def presplit_ok(B: int, H: int, W: int, C: int, K_next: int) -> bool:
    """Can the (B, H, W, C) output of a train-mode [BN -> ReLU (-> pool)] block be stored pre-split for a consuming 3x3 conv
    with K_next filters?  Needs the f16 x3 policy with forward scaling, the streamed kernel's 64- / 128-column tiles without
    split-K for the consumer's forward and the split-half 9-tap kernel for its weight gradient."""
    if not (_H.PRESPLIT and _H.PRECISION == "split" and _H.GRAD_SPLIT == "f16" and _H.FWD_SCALE):
        return False
    if C % 64 != 0 or K_next % 64 != 0 or C > 512 or 4 * B * H * W * C >= _H._SPLIT_MAX_BYTES:
        return False
    if not LIB.egz_conv3x3_streamed_ok(B, H, W, C, K_next, 0):
        return False
    if _H.SPLITK and LIB.egz_conv3x3_streamed_splits(B, H, W, C, K_next) > 1:
        return False
    return bool(LIB.egz_conv3x3_wgrad_presplit_ok(B, H, W, C, K_next))


# ... and the GRADIENT the BatchNorm backward of an encoder block writes (the dy operand of that block's data gradient and weight
# gradient).  Its maximum is not known before the apply pass runs, so the pairs are scaled by a BOUND instead: |dy| <= |sc| (max
# |dout| + |mean dz| + max |xhat| |mean dz xhat|) per channel, from the abs-max the data-gradient kernel above emits for dout, the
# per-channel max / min of y the forward conv left behind and the two backward sums (egz_bn_relu_pool_bwd_presplit).  A bound that
# is 2^b above the true maximum only moves the f16 window: elements more than 2^(16 - b) below the maximum lose low-order bits
# of their lo half (absolute error <= 2^-37 of the bound), nothing saturates.  Unlike the forward activations this is not
# bit-identical to the fp32-gradient path (another power-of-two scale rounds sub-window elements differently): the step's
# gradients move by ~1e-7 relative (hipops.PRESPLIT_GRAD; A/B decided in round 5: -0.19 ms; test_presplit_gradients_match
# flips it).


def presplit_grad_ok(B: int, H: int, W: int, C: int, K: int) -> bool:
    """Can the gradient w.r.t. the (B, H, W, K) output of a C -> K conv (written by that block's BatchNorm backward) be stored
    pre-split?  Its consumers: the conv's data gradient (reduction over K, C output columns, unsplit streamed launch on the
    64- / 128-column tiles) and its weight gradient (the split-half 9-tap kernel)."""
    if not (_H.PRESPLIT_GRAD and _H.PRESPLIT and _H.PRECISION == "split" and _H.GRAD_SPLIT == "f16" and _H.FWD_SCALE):
        return False
    if C % 64 != 0 or K % 64 != 0 or K > 512 or 4 * B * H * W * K >= _H._SPLIT_MAX_BYTES:
        return False
    if not LIB.egz_conv3x3_streamed_ok(B, H, W, K, C, 0):
        return False
    if _H.SPLITK and LIB.egz_conv3x3_streamed_splits(B, H, W, K, C) > 1:
        return False
    return bool(LIB.egz_conv3x3_wgrad_presplit_ok(B, H, W, C, K))


# FLOP accounting of a launch over a zero-PADDED operand (the 20-channel flow stack runs as 32 channels): the algorithmic count
# prices the real channels (the padded count over-stated the step's FLOPs by 0.3 %).  Set around the launch.
ALGO_CHANNELS = [None]


def _conv3x3_streamed(label: str, x, wq, y, B: int, H: int, W: int, C: int, K: int, *, bias=None, stat=None, epi: int = 0,
                      dtype: int, mode: int = 0, pre: bool = False, absmax=None, mask=None, absmax_out=None, bn=None,
                      minmax=None) -> None:
    """One launch of egz_conv3x3_fwd_streamed (GEMM view: x (B, H, W, C) gathered, K columns; mode 0 plain, 1 upsample data
    gradient, 2 upsample forward; ``pre``: x holds pre-split pairs).  ``label``: the family name check() reports."""
    check(LIB.egz_conv3x3_fwd_streamed(x.data_ptr(), wq.data_ptr(), _p(bias), y.data_ptr(), _p(stat), B, H, W, C, K, epi, dtype,
                                       mode | (0x100 if pre else 0), _p(absmax), _p(mask), _p(absmax_out), _p(bn), _p(minmax),
                                       _stream()), label)


def conv3x3_fwd(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], K: int, ups=False,
                epi: int = EPI_BIAS, tile_flag: int = 0, dtype: int = 0, p2: bool = False, absmax: Optional[torch.Tensor] = None,
                streamed: bool = False, bn_in: Optional[torch.Tensor] = None, want_minmax: bool = False,
                pre_in: bool = False, want_bound: bool = False, want_amax: bool = False):
    """x: (B, Hin, Win, C) NHWC.  Returns (y (B,H,W,K), stat_partial or None); H,W = 2*Hin,2*Win if ups.
    ups: False | 'fold' (3x3 taps on the virtual upsampled image, wp = 'fwd' packing) | 'phase' or True (four 2x2
    phase convolutions on the low-res input, 4/9 of the MACs, wp = 'ups_fwd' packing).
    ``bn_in``: x is the PRE-BatchNorm output of the block below and bn_in its (4, C) coefficients -- the kernel normalises +
    ReLUs while staging x (deferred BatchNorm; narrow streamed geometry only, x must carry the abs-max of the normalised
    values).  ``want_minmax``: with EPI_BIAS_STATS on the narrow kernel, also return y's per-channel max / min rows as
    ``y._egz_minmax`` (what the deferred BatchNorm of THIS layer needs).
    ``pre_in``: x holds PRE-SPLIT activations (bn_relu_pool_fwd(presplit_am=...); x must carry the abs-max they were scaled
    with) -- plain streamed f16 x3 launch with the statistics epilogue only.  ``want_bound`` (EPI_BIAS_STATS on the streamed
    kernel's 64- / 128-column tiles, unsplit): also fold y's per-channel max / min into a 2 K-uint buffer, returned as
    ``y._egz_mm`` (input of bn_finalize(..., mm=...)); absent when the launch took another route."""
    _req(x, "x")
    if pre_in and not (dtype == F16X3 and streamed and not ups and epi in (EPI_BIAS_STATS, EPI_BIAS) and bn_in is None
                       and getattr(x, "_egz_absmax", None) is not None):
        raise RuntimeError("a pre-split activation reached a launch that cannot take it")
    if (bn_in is not None or want_minmax) and not (dtype and streamed and not ups):
        raise RuntimeError("deferred BatchNorm operands exist on the streamed narrow kernel only")
    B, Hin, Win, C = x.shape
    H, W = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    y = torch.empty((B, H, W, K), dtype=torch.float32, device=x.device)
    stat = None
    if dtype == F16X3 and absmax is None and _H.FWD_SCALE:
        absmax = _H.absmax_of(x)               # forward operand: the producer's max |x| (or one standalone pass)
    amo = None                              # max |y| of a bias + ReLU launch, for the convolution that consumes y
    if dtype and epi == EPI_BIAS_RELU and _want_fwd_absmax() and K % 64 == 0:
        amo = _new_absmax(x.device)
        y._egz_absmax = amo
    # ... or of a data gradient (epi EPI_BIAS without a bias): max |dx| bounds the BatchNorm backward of the block below
    # (hipops.PRESPLIT_GRAD); only the unsplit streamed launch on the 64- / 128-column tiles emits it
    amax_dgrad = bool(want_amax and dtype and streamed and not ups and epi == EPI_BIAS and K % 64 == 0)
    uflag = 0 if not ups else (1 if ups == "fold" else 3)
    flags = uflag | (epi << 4) | (0x200 if dtype else tile_flag)      # split kernels: 128-row tiles
    if epi == EPI_BIAS_STATS and not (dtype and streamed):
        rows = LIB.egz_conv3x3_stat_rows(B, H, W, K, flags)
        stat = torch.empty((rows, 2, K), dtype=torch.float64, device=x.device)
    if dtype and streamed and ups:      # wp = the 'ups_fwd_frag' packing: four phase convolutions on the streamed-weight kernel
        if ups == "fold" or epi not in (EPI_BIAS, EPI_BIAS_RELU) or bn_in is not None:
            raise RuntimeError("the streamed upsample forward is the phase form with a bias / bias + ReLU epilogue")
        PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
        _conv3x3_streamed("egz_conv3x3_fwd_split", x, wp, y, B, H, W, C, K, bias=bias, epi=epi, dtype=dtype, mode=2,
                          absmax=absmax, absmax_out=amo)
        return y, None
    if dtype and streamed:       # wp = fragment-ordered packing (conv_weight): weights L2 -> registers, halo through LDS
        PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * (ALGO_CHANNELS[0] or C))
        ns = LIB.egz_conv3x3_streamed_splits(B, H, W, C, K) if (_H.SPLITK and epi <= EPI_BIAS_STATS) else 1
        if ns > 1 and pre_in:
            raise RuntimeError("a pre-split activation reached a split-K launch (hipops.presplit_ok excludes them)")
        if ns > 1:      # few pixel tiles (batch-1 inference, 14 x 14 layers at small batches): split the channel blocks
            if epi == EPI_BIAS_STATS:   # the fix-up pass emits one partial row per 32 pixels
                stat = torch.empty((LIB.egz_conv3x3_fwd_streamed_splitk_stat_rows(B, H, W), 2, K), dtype=torch.float64,
                                   device=x.device)
            nb = LIB.egz_conv3x3_fwd_streamed_splitk_ws_bytes(B, H, W, K, ns)
            ws = _H.workspace(nb, x.device)
            check(LIB.egz_conv3x3_fwd_streamed_splitk(x.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), _p(stat), B, H, W,
                                                      C, K, epi, dtype, _p(absmax), ws.data_ptr(), nb, ns, _p(amo), _stream()),
                  "egz_conv3x3_fwd_streamed_splitk")
            return y, stat
        mm = None
        if epi == EPI_BIAS_STATS:
            rows = LIB.egz_conv3x3_streamed_stat_rows(B, H, W, C, K)
            stat = torch.empty((rows, 2, K), dtype=torch.float64, device=x.device)
            if want_minmax:
                mm = torch.empty((rows, 2, K), dtype=torch.float32, device=x.device)
                y._egz_minmax = mm
            elif want_bound and K % 64 == 0 and K <= 512:
                mm = _new_absmax(x.device)              # 2 K <= 1024 zero-filled uints: per-channel max of y and of -y
                y._egz_mm = mm
        if pre_in:
            PRESPLIT_STATS["fwd" if epi == EPI_BIAS_STATS else "dgrad"] += 1
        if amax_dgrad:
            amo = _new_absmax(x.device)
            y._egz_absmax = amo
        if p2:
            _note_p2(dtype, 2.0 * B * H * W * K * 9 * C)
        _conv3x3_streamed("egz_conv3x3_fwd_split", x, wp, y, B, H, W, C, K, bias=bias, stat=stat, epi=epi,
                          dtype=_p2(dtype) if p2 else dtype, pre=pre_in, absmax=absmax, absmax_out=amo, bn=bn_in, minmax=mm)
        return y, stat
    if pre_in:
        raise RuntimeError("a pre-split activation reached a launch that is not on the streamed kernel")
    if dtype:
        PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
        sflags = (flags & 0x33) | (tile_flag & 0x6000)      # 0x4000: split-K tail schedule, 0x2000: no halo-tile kernel
        nb = LIB.egz_conv3x3_fwd_split_ws_bytes(B, H, W, C, K, sflags)
        ws = _H.workspace(nb, x.device) if nb else None
        check(LIB.egz_conv3x3_fwd_split(x.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), _p(stat), B, H, W, C, K,
                                        sflags, dtype, _p(ws), nb, _p(absmax), _p(amo), _stream()), "egz_conv3x3_fwd_split")
        return y, stat
    PROF.note_flops("egz_conv3x3_fwd", 2.0 * B * H * W * K * 9 * C)
    check(LIB.egz_conv3x3_fwd(x.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), _p(stat), B, H, W, C, K, flags,
                              _stream()), "egz_conv3x3_fwd")
    return y, stat


def conv3x3_dgrad(dy: torch.Tensor, wp_dgrad: torch.Tensor, C: int, dtype: int = 0, streamed: bool = False,
                  pre_in: bool = False) -> torch.Tensor:
    """dy: (B,H,W,K) -> dx (B,H,W,C) (for an upsampled conv this is the gradient of the upsampled input).
    dtype F16X3: dy is scaled by a power of two derived from its abs-max so that the f16 halves carry it.
    ``pre_in``: dy holds pre-split pairs (bn_relu_pool_bwd(presplit=...)).  dx carries max |dx| (``_egz_absmax``) where the launch
    can emit it."""
    y, _ = _H.conv3x3_fwd(dy, wp_dgrad, None, C, ups=False, epi=EPI_BIAS, dtype=dtype,
                       absmax=_H.absmax_of(dy) if dtype == F16X3 else None, streamed=streamed, pre_in=pre_in,
                       want_amax=_want_absmax() and _H.PRESPLIT_GRAD, p2=True)
    return y


def conv3x3_ups_dgrad(dy: torch.Tensor, wp_ups_dgrad: torch.Tensor, C: int, dtype: int = 0, streamed: bool = False) -> torch.Tensor:
    """Data gradient of [upsample x2 -> conv3x3] w.r.t. the LOW-res input: dy (B,H,W,K) -> dx (B,H/2,W/2,C).
    streamed: wp = the 'ups_dgrad_frag' packing (conv_weight(..., 'ups_dgrad', ...)), polyphase streamed-weight kernel."""
    _req(dy, "dy")
    B, H, W, K = dy.shape
    dx = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=dy.device)
    if dtype and streamed:
        PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
        am = _H.absmax_of(dy) if dtype == F16X3 else None
        _note_p2(dtype, 2.0 * B * H * W * K * 9 * C)
        _conv3x3_streamed("egz_conv3x3_fwd_streamed(ups_dgrad)", dy, wp_ups_dgrad, dx, B, H, W, K, C, dtype=_p2(dtype), mode=1,
                          absmax=am)
        return dx
    if dtype:      # GEMM roles: reduction over the conv's K, output channels = the conv's C
        PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
        nb = LIB.egz_conv3x3_fwd_split_ws_bytes(B, H, W, K, C, 4)
        ws = _H.workspace(nb, dy.device) if nb else None
        am = _H.absmax_of(dy) if dtype == F16X3 else None
        check(LIB.egz_conv3x3_fwd_split(dy.data_ptr(), wp_ups_dgrad.data_ptr(), None, dx.data_ptr(), None, B, H, W, K, C,
                                        4, dtype, _p(ws), nb, _p(am), None, _stream()), "egz_conv3x3_fwd_split(ups_dgrad)")
        return dx
    PROF.note_flops("egz_conv3x3_ups_dgrad", 2.0 * B * H * W * K * 9 * C)     # algorithmic (reference) FLOPs
    check(LIB.egz_conv3x3_ups_dgrad(dy.data_ptr(), wp_ups_dgrad.data_ptr(), dx.data_ptr(), B, H, W, C, K,
                                    0, _stream()), "egz_conv3x3_ups_dgrad")
    return dx


EPI_MASK_SUMS = 3
# ReLU backward of a decoder block folded into the epilogue of the dgrad kernel above it (functions.ConvReLU): it removes 11
# passes over the decoder gradients (relu_bwd_bias, 1.0 ms per step).  Round 2 measured it slower (35.56 vs 35.39 ms,
# profiles/r02_bench_ab_knobs.txt) -- with the mask load inside a per-lane branch every epilogue element waited for its own
# load.  With the branch-free epilogue (buffer loads / stores with out-of-range offsets for invalid rows, round 3) the step
# is 0.55 ms faster with it (32.6 vs 33.15 ms, profiles/r03_ab_notes.txt), so it is the default
# (hipops.MASK_FUSE; off position: test_relu_backward_folded_into_dgrad_above).
MASK_FUSE_STATS = {"produced": 0, "consumed": 0}                 # how often the fused form ran / was picked up (tests)


def conv3x3_dgrad_masked(dy: torch.Tensor, wq: torch.Tensor, C: int, dtype: int, mask_src: torch.Tensor, ups: bool):
    """Data gradient of a plain (``ups`` False) or upsample-fused (True) 3x3 conv on the streamed-weight kernel, with the
    ReLU backward of the layer BELOW folded into the epilogue: ``mask_src`` (B, H', W', C) is that layer's post-ReLU output
    (= this conv's input).  Returns (dx masked, stat rows (rows, 2, C) fp64 whose plane 0 sums to the bias gradient of the
    layer below, abs-max buffer of dx)."""
    _req(dy, "dy"); _req(mask_src, "mask_src")
    B, H, W, K = dy.shape
    Ho, Wo = (H // 2, W // 2) if ups else (H, W)
    if tuple(mask_src.shape) != (B, Ho, Wo, C):
        raise RuntimeError(f"mask_src {tuple(mask_src.shape)} does not match the gradient {(B, Ho, Wo, C)}")
    dx = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=dy.device)
    rows = (B * Ho * Wo + 127) // 128
    stat = torch.empty((rows, 2, C), dtype=torch.float64, device=dy.device)
    MASK_FUSE_STATS["produced"] += 1
    amo = _new_absmax(dy.device)
    PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
    am = _H.absmax_of(dy) if dtype == F16X3 else None
    _note_p2(dtype, 2.0 * B * H * W * K * 9 * C)
    _conv3x3_streamed("egz_conv3x3_fwd_streamed(masked dgrad)", dy, wq, dx, B, H, W, K, C, stat=stat, epi=EPI_MASK_SUMS,
                      dtype=_p2(dtype), mode=1 if ups else 0, absmax=am, mask=mask_src, absmax_out=amo)
    return dx, stat, amo


EPI_BNSUMS = 5
# BatchNorm-backward sums of the layer below folded into the narrow data-gradient kernel (late_fusion.py:10-12 chain at
# 32 channels): removes that layer's reduce pass (two reads of its 205 MB tensors at B = 32, 224 x 224).
# hipops.BNSUMS_FUSE = False keeps the separate pass (A/B runs, and the parity test compares the two).
BNSUMS_STATS = {"produced": 0, "consumed": 0}


# ... and for the wide layers (the VGG encoders: conv -> BN -> ReLU -> conv without a pool in between, utils.py:64-76): the same
# epilogue on the 128- / 64-column tiles of the streamed kernel.  hipops.BNSUMS_WIDE = False keeps the reduce pass there
# (test_bn_backward_sums_folded_into_encoder_dgrad compares the two).


def bnsums_ok(B: int, H: int, W: int, C: int, K: int, dtype: int) -> bool:
    """Can the data gradient of a K <- C channel conv (dy (B,H,W,K) -> dx (B,H,W,C)) also produce the BatchNorm-backward sums
    of the C-channel block below?  The persistent narrow kernel (C, K <= 32), or the streamed kernel's 64- / 128-column
    tiles (C % 64 == 0)."""
    if not (_H.BNSUMS_FUSE and dtype and 4 * B * H * W * C < 2 ** 32 and LIB.egz_conv3x3_streamed_ok(B, H, W, K, C, 0)):
        return False
    if C <= 32 and K <= 32:
        return C % 4 == 0 and K % 4 == 0 and H % 16 == 0 and W % 16 == 0
    return bool(_H.BNSUMS_WIDE and C % 64 == 0 and K % 32 == 0
                and (not _H.SPLITK or LIB.egz_conv3x3_streamed_splits(B, H, W, K, C) <= 1))      # (few-tile launches stay split-K)


def conv3x3_dgrad_bnsums(dy: torch.Tensor, wq: torch.Tensor, C: int, dtype: int, bn_y: torch.Tensor, coef: torch.Tensor,
                         pre_in: bool = False):
    """Data gradient of a plain 3x3 conv (dy (B,H,W,K) -> dx (B,H,W,C)) whose input is the output of a train-mode
    [BatchNorm -> ReLU]: ``bn_y`` (B,H,W,C) is that layer's pre-BN conv output and ``coef`` its (4, C) batch coefficients
    (mean, 1/std, scale, shift).  Returns (dx, sums) with sums (rows, 2, C) fp64 = partial rows of (sum dz, sum dz * xhat),
    the ``sums`` argument of bn_relu_pool_bwd for that layer."""
    _req(dy, "dy"); _req(bn_y, "bn_y"); _req(coef, "coef")
    B, H, W, K = dy.shape
    if tuple(bn_y.shape) != (B, H, W, C) or tuple(coef.shape) != (4, C):
        raise RuntimeError(f"bn_y {tuple(bn_y.shape)} / coef {tuple(coef.shape)} do not match the gradient {(B, H, W, C)}")
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device=dy.device)
    stat = torch.empty((LIB.egz_conv3x3_streamed_stat_rows(B, H, W, K, C), 2, C), dtype=torch.float64, device=dy.device)
    BNSUMS_STATS["produced"] += 1
    PROF.note_flops("egz_conv3x3_fwd_split", 2.0 * B * H * W * K * 9 * C)
    am = _H.absmax_of(dy) if dtype == F16X3 else None
    amo = None
    if _want_absmax() and _H.PRESPLIT_GRAD and C % 64 == 0:       # max |dx|: bounds the BatchNorm backward of the block below
        amo = _new_absmax(dy.device)
        dx._egz_absmax = amo
    if pre_in:
        if not (dtype == F16X3 and C % 64 == 0 and getattr(dy, "_egz_absmax", None) is not None):
            raise RuntimeError("a pre-split gradient reached a data-gradient launch that cannot take it")
        PRESPLIT_STATS["dgrad"] += 1
    if C % 64 == 0:        # (the narrow late-fusion form of this launch stays three-product)
        _note_p2(dtype, 2.0 * B * H * W * K * 9 * C)
    _conv3x3_streamed("egz_conv3x3_fwd_streamed(dgrad + BN sums)", dy, wq, dx, B, H, W, K, C, stat=stat, epi=EPI_BNSUMS,
                      dtype=_p2(dtype), pre=pre_in, absmax=am, mask=bn_y, absmax_out=amo, bn=coef)
    return dx, stat


def colsum_f64(stat: torch.Tensor, ncols_out: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stat: (rows, cols...) fp64 partial rows -> fp32 sums of the first ``ncols_out`` columns (fixed order)."""
    rows = stat.shape[0]
    cols = stat.numel() // rows
    res = _out(out, (ncols_out,), stat.device)
    ws = _H.workspace(64 * cols * 8, stat.device)
    check(LIB.egz_colsum_f64(stat.data_ptr(), rows, cols, ncols_out, res.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "egz_colsum_f64")
    return res


# egz_conv3x3_wgrad flags (include/egaze_hip.h; P2_WGRAD above is the last of them)
WGRAD_UPS = 1              # the conv input was the nearest-x2 upsampling of x
WGRAD_BT64, WGRAD_PERTAP, WGRAD_FOLD9 = 0x100, 0x800, 0x1000      # A/B variants (variant_flag; tools/bench_conv.py --wflag)
WGRAD_SPLIT = 0x2000       # split-half arithmetic (bf16 x3, or f16 x3 when dy_absmax is passed)
WGRAD_NINETILE = 0x4000    # A/B: what WGRAD_TAPPACK = False sends
WGRAD_XPRE, WGRAD_DPRE = 0x8000, 0x10000      # x / dy holds pre-split pairs# hipops.WGRAD_TAPPACK: K <= 8 filters on the narrow kernel run with (tap, k) pairs as GEMM columns (False: nine zero-padded
# 32-column tiles; test_conv3x3_wgrad_split flips it)


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, ups: bool = False, variant_flag: int = 0,
                  precision: Optional[str] = None, out: Optional[torch.Tensor] = None,
                  x_bn: Optional[torch.Tensor] = None, x_pre: bool = False, dy_pre: bool = False) -> torch.Tensor:
    """-> dw (K, C, 3, 3); ``out`` = a contiguous K*C*9 destination (a gradient sink) written instead of a fresh tensor.
    ``x_bn``: x is a pre-BatchNorm tensor, normalised + ReLU'd while it is staged (deferred BatchNorm, narrow kernel only)."""
    _req(x, "x"); _req(dy, "dy")
    B, H, W, K = dy.shape
    C = x.shape[3]
    dw = _out(out, (K, C, 3, 3), x.device)
    flags = (WGRAD_UPS if ups else 0) | variant_flag | (0 if _H.WGRAD_TAPPACK else WGRAD_NINETILE)
    am = xam = None
    prec = precision or _H.PRECISION
    if prec in ("split", "split_bf16", "split_f16"):
        flags |= WGRAD_SPLIT
        if prec == "split_f16" or (prec == "split" and _H.GRAD_SPLIT == "f16"):
            am = _H.absmax_of(dy)             # f16 x3 with dy scaled by its abs-max; bf16 x3 otherwise
            if _H.FWD_SCALE:
                xam = _H.absmax_of(x)         # ... and the activation operand by its own (the forward pass left it on x)
    if x_pre:      # x holds pre-split activations (see PRESPLIT): the split-half 9-tap kernel copies the pairs into its LDS image
        if not (flags & WGRAD_SPLIT and am is not None and getattr(x, "_egz_absmax", None) is not None and not ups and x_bn is None
                and LIB.egz_conv3x3_wgrad_presplit_ok(B, H, W, C, K)):
            raise RuntimeError("a pre-split activation reached a weight-gradient launch that cannot take it")
        xam = x._egz_absmax
        flags |= WGRAD_XPRE
        PRESPLIT_STATS["wgrad"] += 1
    if dy_pre:     # dy holds pre-split pairs scaled by the bound in dy._egz_absmax (bn_relu_pool_bwd(presplit=...))
        if not (flags & WGRAD_SPLIT and am is not None and xam is not None and not ups and x_bn is None
                and LIB.egz_conv3x3_wgrad_presplit_ok(B, H, W, C, K)):
            raise RuntimeError("a pre-split gradient reached a weight-gradient launch that cannot take it")
        flags |= WGRAD_DPRE
        PRESPLIT_STATS["wgrad_dy"] += 1
    if _H.BWD_PRODUCTS == 2 and am is not None:
        flags |= P2_WGRAD          # two products per MAC on the wide split-half kernels (ignored by the others)
    nb = LIB.egz_conv3x3_wgrad_ws_bytes(B, H, W, C, K, flags)
    ws = _H.workspace(nb, x.device)
    PROF.note_flops("egz_conv3x3_wgrad", 2.0 * B * H * W * K * 9 * (ALGO_CHANNELS[0] or C))
    check(LIB.egz_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, C, K, flags, ws.data_ptr(),
                                ws.numel(), _p(am), _p(xam), _p(x_bn), _stream()), "egz_conv3x3_wgrad")
    return dw


def conv_first_fwd(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stats: bool,
                   want_minmax: bool = False, want_bound: bool = False):
    """``want_minmax`` (direct kernel, C <= 3 -> 32 filters, with stats): y's per-channel max / min rows as y._egz_minmax.
    ``want_bound`` (direct kernel, with stats): the 2 K-uint atomic form as y._egz_mm (see conv3x3_fwd)."""
    _req(x_nchw, "x"); _req(w, "weight")
    B, C, H, W = x_nchw.shape
    K = w.shape[0]
    y = torch.empty((B, H, W, K), dtype=torch.float32, device=x_nchw.device)
    stat = mm = mmo = None
    if stats:
        rows = LIB.egz_conv_first_stat_rows_for(B, H, W, C, K)
        stat = torch.empty((rows, 2, K), dtype=torch.float64, device=y.device)
        if want_minmax:
            mm = torch.empty((rows, 2, K), dtype=torch.float32, device=y.device)
            y._egz_minmax = mm
        if want_bound and C <= 3 and K in (32, 64) and B * H * W * K < 2 ** 31:
            mmo = _new_absmax(y.device)
            y._egz_mm = mmo
    PROF.note_flops("egz_conv_first_fwd", 2.0 * B * H * W * K * 9 * C)
    check(LIB.egz_conv_first_fwd(x_nchw.data_ptr(), w.data_ptr(), _p(bias), y.data_ptr(), _p(stat), B, H, W, C, K,
                                 _p(mm), _p(mmo), _stream()), "egz_conv_first_fwd")
    return y, stat


def conv_first_wgrad(x_nchw: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x_nchw, "x"); _req(dy, "dy")
    B, C, H, W = x_nchw.shape
    K = dy.shape[3]
    dw = _out(out, (K, C, 3, 3), dy.device)
    ws = _H.workspace(LIB.egz_conv_first_wgrad_ws_bytes(B, H, W, C), dy.device)
    PROF.note_flops("egz_conv_first_wgrad", 2.0 * B * H * W * K * 9 * C)
    check(LIB.egz_conv_first_wgrad(x_nchw.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, C, K, ws.data_ptr(),
                                   ws.numel(), _stream()), "egz_conv_first_wgrad")
    return dw
