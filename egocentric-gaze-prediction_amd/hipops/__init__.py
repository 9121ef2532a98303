"""Tensor-level wrappers over the C-ABI (``include/egaze_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every wrapper passes raw
``data_ptr()``s, explicit shapes and ``torch.cuda.current_stream()`` to ``libegaze_hip.so``.
Activations are NHWC fp32 (``(B, H, W, C)`` contiguous tensors); weights keep the reference layout
``(Cout, Cin, 3, 3)`` and are re-packed on the device when they change.
All wrappers raise on CPU tensors -- there is no CPU fallback.

One module per op family (``_core``, ``packing``, ``sinks``, ``absmax``, ``conv``, ``bn``, ``layout``, ``loss``, ``lstm``,
``metrics``, ``dataprep``, ``jpeg``, ``vis``, ``flow``, ``handover``); every name is re-exported here, and callers use ``hipops.NAME``.

This file holds the SWITCHES: every name that a driver or a test rebinds on this module (``hipops.PRECISION = "f32"``,
``monkeypatch.setattr(hipops, "SPLITK", False)``).  The family modules never bind them; they read ``_H.NAME`` (``_H`` = this
package) inside their function bodies, so a rebind takes effect at the next call.  A public hipops function calls another
one as ``_H.name(...)`` for the same reason: replacing a function on this module intercepts the calls made from inside it.
What each switch was measured at is written beside the code it steers, in its family module.
"""
import os

# --- arithmetic (conv.py)
# Wide convolutions: "split" (default) = split-half f16 x3 MFMA, "f32" = exact-f32 MFMA.  bench.py, test_hip_ops and
# test_hip_model_sp set it.
PRECISION = os.environ.get("EGAZE_PRECISION", "split")
# Operand type of the split-half gradient kernels: "f16" (default; f16 x3, abs-max scaled) or "bf16" (opt-in).  test_hip_ops,
# test_hip_model_sp.
GRAD_SPLIT = os.environ.get("EGAZE_GRAD_SPLIT", "f16")
# MFMA products per MAC in the backward convolutions: 3 (default, fp32-class) or 2 (opt-in).  conftest's `two_products`
# fixture, test_backward_two_products, bench.py (extra.bwd2).
BWD_PRODUCTS = int(os.environ.get("EGAZE_BWD_PRODUCTS", "3"))
if BWD_PRODUCTS not in (2, 3):
    raise ValueError(f"EGAZE_BWD_PRODUCTS={BWD_PRODUCTS}: 3 (default, fp32-class) or 2 (opt-in)")
# Operands of this many bytes or more stay on the 64-bit-addressed f32 kernels (the split kernels fetch through 32-bit
# buffer offsets).  Default just under 4 GiB; test_large_operand_routes_to_the_64bit_addressed_kernels lowers it.
_SPLIT_MAX_BYTES = (1 << 32) - (1 << 24)

# --- 3x3 convolution forms (conv.py)
# Split-K form of the streamed kernel for launches with few pixel tiles.  Default on; test_conv3x3_streamed_splitk and the
# whole-model gradient tests (which pin the summation order) turn it off.
SPLITK = True
# Encoder activations stored as pre-split f16 pairs by their BN -> ReLU (-> pool) pass.  Default on;
# test_presplit_activations_bit_identical turns it off.
PRESPLIT = True
# ... and the gradient a BatchNorm backward writes, scaled by a bound.  Default on; test_presplit_gradients_match.
PRESPLIT_GRAD = True
# ReLU backward of a decoder block folded into the data-gradient epilogue above it (read by functions.ConvReLU).  Default
# on; test_relu_backward_folded_into_dgrad_above.
MASK_FUSE = True
# BatchNorm-backward sums folded into the data-gradient kernel: narrow layers / BNSUMS_WIDE: the wide encoder layers too.
# Default on; test_hip_lf flips the first, test_bn_backward_sums_folded_into_encoder_dgrad the second.
BNSUMS_FUSE = True
BNSUMS_WIDE = True
# Narrow weight gradient with K <= 8 filters: (tap, k) pairs as GEMM columns (False: nine zero-padded 32-column tiles).
# Default on; test_conv3x3_wgrad_split.
WGRAD_TAPPACK = True

# --- abs-max (absmax.py)
# Forward activations carry their abs-max and are scaled before the f16 split.  Default on;
# test_forward_scaling_off_loses_the_small_range.
FWD_SCALE = True

# --- BatchNorm (bn.py)
# Late-fusion stack: a narrow block's BN -> ReLU is applied by the next block's kernels while they stage its input.  Default
# on; test_deferred_batchnorm_matches_materialised (test_hip_lf).
BN_DEFER = True
# Inference: eval-mode BatchNorm folded into the convolution's weights (read by functions / utils).  Default on;
# test_eval_batchnorm_folded_into_conv compares the two.
EVAL_FOLD = True
# True only while utils.conv_bn_relu_pool calls ConvBNReLUPool.apply under torch.no_grad(); utils.py sets and clears it.
INFER_CALL = False

# --- optimizer hand-over (packing.py, sinks.py)
# FusedAdam.step() rebuilds the stale fragment-ordered packings of its parameters in one launch (False: lazily, per layer).
# Default on; test_pack_frag_batch_matches_per_layer.
BATCH_REPACK = True
# Backward kernels write gradients straight into the fused optimizer's flat buffer (False: autograd's AccumulateGrad).
# Default on; AT._GraphedSampleStep honours the off position.
DIRECT_GRADS = True

# --- AT network (lstm.py)
# The LSTM recurrence as one persistent launch per direction where the geometry allows; EGAZE_LSTM_PERSIST=0, `with
# lstm_persistent(False)` (bench.py) and lstm_persist_check() after a lost hand-off select the wavefront launches.
LSTM_PERSIST = os.environ.get("EGAZE_LSTM_PERSIST", "1") != "0"

from .absmax import _AbsmaxArena  # noqa: E402

# The one arena the abs-max buffers are cut from; test_hip_stream_order swaps in an arena of its own.
ABSMAX_ARENA = _AbsmaxArena()

REBINDABLE = ("PRECISION", "GRAD_SPLIT", "BWD_PRODUCTS", "_SPLIT_MAX_BYTES", "SPLITK", "PRESPLIT", "PRESPLIT_GRAD",
              "MASK_FUSE", "BNSUMS_FUSE", "BNSUMS_WIDE", "WGRAD_TAPPACK", "FWD_SCALE", "BN_DEFER", "EVAL_FOLD", "INFER_CALL",
              "BATCH_REPACK", "DIRECT_GRADS", "LSTM_PERSIST", "ABSMAX_ARENA")

from .._lib import LIB as _RAW_LIB, check  # noqa: E402,F401
from ._core import (  # noqa: E402,F401
    EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_STATS, LIB, LaunchStatus, PROF, _LibProxy, _Profiler, _WS, _out, _p, _ptr_table,
    _raw_stream, _req, _stream, drain_status, finish_launch, workspace,
)
from .packing import (  # noqa: E402,F401
    _BATCH_PINNED, _BATCH_TABLES, _CAPTURE_LOG, _PACKED, _PACK_FN, _UID, _USED, _WEIGHT_EPOCH, _drop_packed, _tag, _uid,
    bump_weight_epoch, note_replay, packed_weight, refresh_packings, repack_stale, touch_params,
)
from .sinks import (  # noqa: E402,F401
    GradSink, PENDING_PRODUCER, grad_done, grad_sink,
)
from .absmax import (  # noqa: E402,F401
    ABSMAX_STATS, _new_absmax, _want_absmax, _want_fwd_absmax, absmax_of, absmax_value, capture, carry_absmax,
)
from .conv import (  # noqa: E402,F401
    ALGO_CHANNELS, BF16X3, BNSUMS_STATS, EPI_BNSUMS, EPI_MASK_SUMS, F16X3, F32, MASK_FUSE_STATS, P2_DTYPE, P2_WGRAD,
    PRESPLIT_STATS, WGRAD_BT64, WGRAD_DPRE, WGRAD_FOLD9, WGRAD_NINETILE, WGRAD_PERTAP, WGRAD_SPLIT, WGRAD_UPS,
    WGRAD_XPRE, _conv3x3_streamed, _note_p2, _p2, bnsums_ok, colsum_f64, conv3x3_dgrad, conv3x3_dgrad_bnsums,
    conv3x3_dgrad_masked, conv3x3_fwd, conv3x3_ups_dgrad, conv3x3_wgrad, conv_dtype, conv_first_fwd,
    conv_first_wgrad, conv_weight, precision_banner, presplit_grad_ok, presplit_ok,
)
from .bn import (  # noqa: E402,F401
    BN_DEFER_STATS, EVAL_FOLD_STATS, _stream_device, bn_bwd_first_wgrad, bn_bwd_first_wgrad_ok, bn_defer_ok,
    bn_eval_coeffs, bn_finalize, bn_finalize_deferred, bn_fold_is_warm, bn_fold_key, bn_folded_conv,
    bn_relu_pool_bwd, bn_relu_pool_fwd, pairmax_bwd, pairmax_fwd,
)
from .layout import (  # noqa: E402,F401
    cat2_planes, channel_stats, colsum, fill_zero, nchw_to_nhwc, nchw_to_nhwc_pad, nhwc_to_nchw,
    prepare_network_input, relu_bwd, relu_bwd_bias, stack2, take_prepared_input, upsample2x_bwd,
)
from .loss import (  # noqa: E402,F401
    adam_step, adam_step_dev, conv1x1_sigmoid_bwd, conv1x1_sigmoid_bwd_masked, conv1x1_sigmoid_fwd, floss_bwd,
    floss_fwd, mse_bwd, mse_fwd, mse_fwd_grad,
)
from .lstm import (  # noqa: E402,F401
    LSTM_POOL_STATUS, _PERSIST_SYNC, _lstm_b1_dims, _persist_sync, add, check_lstm_pool_status, copy_into, gemm,
    linear_fwd, lstm_b1_bwd, lstm_b1_fwd, lstm_cell_bwd, lstm_cell_fwd, lstm_persist_bwd, lstm_persist_check,
    lstm_persist_errors, lstm_persist_fwd, lstm_persist_ok, lstm_persist_status, lstm_persistent, lstm_pool_fetch,
    lstm_wave_bwd, lstm_wave_fwd, matmul_nn, matmul_tn, matmul_tn_batched, tanh_bwd, tanh_fwd, transpose2d,
)
from .metrics import _GAUSS_W, _gauss_weights, aae_auc  # noqa: E402,F401
from .dataprep import (  # noqa: E402,F401
    AFFINE_STATUS, AugSpec, RESIDENT_STATUS, _AREA_T, _NORM_CONST, _RESIDENT_FIELDS, _area_tables, area_table, bilinear_up,
    check_resident_status, crop_mean, gaze_gt_maps, judge_resident_status, late_gather, pixel_weighted_sum, resident_gather,
    resident_gather_aug, u8_center_of_mass, u8_normalize, weighted_minmax, window_mean,
)
from .jpeg import (  # noqa: E402,F401
    JPEG_ENCODE_STATUS, JPEG_STATUS, _SUBSAMPLING, _dev_table, _jpeg_encode_args, _jpeg_encode_scan, jpeg_decode,
    jpeg_encode, jpeg_encode_into, JPEG_ROUNDTRIP_STATUS, jpeg_roundtrip,
)
from .vis import (  # noqa: E402,F401
    _JET, _JET_WARNED, _LINEAR_T, _linear_tables, _u8_dev, cell_argmax_u8, heatmap_overlay, jet_lut,
    jet_table_restated, linear_table, resize_linear_u8,
)
from .flow import (  # noqa: E402,F401
    FLOW_FUSED, FLOW_MAX_LEVELS, FLOW_PRESMOOTH_SIGMA, _FLOW_TAPS, _FLOW_WS, _flow_dev, _flow_hw, _flow_k, _flow_params, _flow_taps,
    bgr_to_gray_u8, flow_gauss, flow_grad, flow_level_sizes, flow_pyramid_sigma, flow_resample, flow_to_u8,
    tvl1_flow, tvl1_iterate, tvl1_warp,
)
from .handover import (  # noqa: E402,F401
    LATE_INPUT_STATUS, LATE_STORE_STATUS, LSTM_STORE_STATUS, _map_dev, check_late_store_status, check_lstm_store_status,
    check_rows, draw_ring, late_input, late_input_status, late_store, late_store_status, lstm_store, lstm_store_status,
)
