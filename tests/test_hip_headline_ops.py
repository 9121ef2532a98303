"""The BatchNorm / ReLU / max-pool, head and GEMM kernels in the launch geometry bench.py times, against torch-CPU float64.

test_hip_ops.py pins every convolution of the SP step entry by entry at batch 32, 224 x 224, but tests the rest of the step at
toy sizes, where the paths the headline runs never execute: the grid-stride loop of the capped BatchNorm-backward reduce
(BWD_BLOCKS), the two-stage finalize over thousands of conv-epilogue stat rows (colsum_partial), the sums the encoders' data
gradient folds in (BNSUMS_WIDE), the pre-split forms.  The whole-model test only bounds encoder tensors in cosine / relative L2,
which a dropped grid-stride chunk would not move.  Here every block of utils.cfg['D'] (one per distinct (H, K, pool)), the two
first blocks, the fusion block and the 1x1 head run at B = 32 on the route functions.py picks, and the AT step's GEMMs run on
the fast path with every tile / stride variant and epilogue.

References are computed in float64 from the exact fp32 operands the kernels received.  Element-wise errors are
max |got - ref| / max |ref|.  Each reduction assertion also measures, from the same fp64 data, the error that the smallest
realistic defect would cause: one block's grid-stride chunk dropped (or counted twice).  The test requires that this defect is
at least 10x the bar, so the bar can see it."""
import gc
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 32
EPS, MOM = 1e-5, 0.1

# (C, H, K, pool, K of the next conv-BN-ReLU block): the first block of utils.make_layers(cfg['D'], C) for each distinct
# (H, K, pool), without the first conv of the stack (FIRST_BLOCKS, C = 3 RGB / 20 flow)
ENC_BLOCKS = [(64, 224, 64, True, 128), (64, 112, 128, False, 128), (128, 112, 128, True, 256), (128, 56, 256, False, 256),
              (256, 56, 256, True, 512), (256, 28, 512, False, 512), (512, 28, 512, True, 512), (512, 14, 512, False, 512)]
FIRST_BLOCKS = [(3, 224, 64, False, 64), (20, 224, 64, False, 64)]
BN_BLOCKS = FIRST_BLOCKS + ENC_BLOCKS


def H():
    import egaze_amd.hipops as h
    return h


def cfg_blocks(c0):
    """(C, H, K, pool, next K) of every conv-BN-ReLU block of utils.make_layers(cfg['D'], c0) at 224 x 224."""
    from egaze_amd.utils import cfg
    items, out, hh, c = cfg['D'], [], 224, c0
    for i, v in enumerate(items):
        if v == 'M':
            continue
        pool = i + 1 < len(items) and items[i + 1] == 'M'
        nxt = next((u for u in items[i + 1:] if u != 'M'), 0)
        out.append((c, hh, v, pool, nxt))
        c = v
        hh = hh // 2 if pool else hh
    return out


@pytest.fixture(autouse=True)
def cpu_threads():
    """fp64 references on at most 16 host threads; each geometry's tensors are freed before the next one."""
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        torch.set_num_threads(keep)
        gc.collect()
        torch.cuda.empty_cache()


def rel(got, ref):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def chunk_defect(contrib, unit, ref):
    """Error max |d| / max |ref| that dropping ONE chunk of ``unit`` consecutive rows of the per-row contributions ``contrib``
    (rows, K) fp64 would cause -- the smallest over the first, a middle and the last chunk."""
    n = contrib.shape[0]
    starts = {0, (n // 2) // unit * unit, (n - unit) // unit * unit}
    scale = ref.abs().max().item()
    return min(contrib[s:s + unit].sum(0).abs().max().item() for s in starts) / scale


def bwd_rows_per_block(K):
    """Pixels one block of the BatchNorm-backward reduce / relu_bwd_bias handles per grid-stride trip (csrc/bn_pool.hip)."""
    return max(256, K // 4) // (K // 4)


def dev_gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def bn_params(K, seed):
    """gamma with every third channel negative (the bound's max / min roles swap there), beta, running mean and variance."""
    g = torch.Generator().manual_seed(seed)
    gamma = (0.5 + torch.rand(K, generator=g)) * torch.where(torch.arange(K) % 3 == 1, -1.0, 1.0)
    beta = 0.2 * torch.randn(K, generator=g)
    rm0, rv0 = 0.1 * torch.randn(K, generator=g), 0.5 + torch.rand(K, generator=g)
    return gamma, beta, rm0, rv0


def route(h, C, Hh, K, pool, next_k):
    """The forward / backward route functions.ConvBNReLUPool takes for this block at B = 32."""
    from egaze_amd import functions as Fn
    first = C in (3, 20)
    padded = first and Fn._first_conv_on_split(C, K)
    Ho = Hh // 2 if pool else Hh
    presplit_out = bool(next_k and h.presplit_ok(B, Ho, Ho, K, next_k))
    gpre = bool(not first and not padded and h.presplit_grad_ok(B, Hh, Hh, C, K))
    first_wgrad = bool(first and not padded and h.bn_bwd_first_wgrad_ok(C, K, pool))
    return first, padded, presplit_out, gpre, first_wgrad


def conv_y(h, C, Hh, K, want_mm, offsets, seed):
    """y and the stat rows of the block's own convolution (the producer functions.py uses), bias = per-channel offsets."""
    g = dev_gen(seed)
    w = torch.randn(K, C, 3, 3, generator=g, device=DEV) * (2.0 / (9 * C)) ** 0.5
    b = offsets.to(DEV)
    first = C in (3, 20)
    if first:
        x = torch.randn(B, C, Hh, Hh, generator=g, device=DEV)
    else:
        x = torch.randn(B, Hh, Hh, C, generator=g, device=DEV).clamp_(min=0)        # post-ReLU-like NHWC activation
    from egaze_amd import functions as Fn
    if first and Fn._first_conv_on_split(C, K):
        xin = h.nchw_to_nhwc_pad(x, 32)
        wp, st = h.conv_weight(w, "fwd", h.F16X3, xin, K)
        y, stat = h.conv3x3_fwd(xin, wp, b, K, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=st, want_bound=want_mm)
    elif first:
        y, stat = h.conv_first_fwd(x, w, b, True, want_bound=want_mm)
    else:
        dt = h.conv_dtype("fwd", K, C, x)
        wp, st = h.conv_weight(w, "fwd", dt, x, K)
        y, stat = h.conv3x3_fwd(x, wp, b, K, epi=h.EPI_BIAS_STATS, dtype=dt, streamed=st, want_bound=want_mm)
    return y, stat


# ------------------------------------------------------------------------------------------------ 1. BatchNorm statistics
@pytest.mark.parametrize("C,Hh,K,pool,next_k", BN_BLOCKS)
def test_bn_statistics_and_presplit_forms_at_batch_32(C, Hh, K, pool, next_k):
    """Train-mode BatchNorm statistics of the block's real convolution output at B = 32 (1.6 M pixels at 224 x 224, thousands of
    stat rows through colsum_partial), channel means spread over +-8 std (the SP step at batch 2, 224 x 224, has |mean| / std up
    to 4.2, features_t.24; median 0.4 - 1.1), every third gamma negative.  Against fp64 evaluated on the GPU's own y: mean and
    the other coefficient rows, the running statistics (unbiased variance, count 1.6 M), num_batches_tracked, colsum_f64 of the
    stat rows.  Where the step takes them: the bound (EXACT max of the block output), the pre-split output (consumer conv
    bit-identical to the fp32-input conv) and the pre-split gradient (max |dy| <= bound <= 8 max |dy|, dgamma / dbeta
    untouched).
    Observed on MI355X (worst block): mean 5.2e-8 of |mean| + std, invstd 5.1e-8, scale 9.8e-8, shift 1.9e-7 (per entry),
    running_mean 1.2e-7, running_var 1.1e-7, colsum_f64 5.2e-8; bars 5x that.  One dropped stat row moves the mean by >= 6.9e-5
    and colsum_f64 by >= 8.0e-5 (20 -> 64 at 224, 12544 rows); the pre-split gradient bound is 1.10 - 1.28x max |dy|."""
    h = H()
    assert (C, Hh, K, pool, next_k) in cfg_blocks(C if C in (3, 20) else 3)
    first, padded, presplit_out, gpre, _ = route(h, C, Hh, K, pool, next_k)
    want_mm = presplit_out or (not first and not padded and h.presplit_grad_ok(B, Hh, Hh, C, K))
    offsets = torch.linspace(-8.0, 8.0, K)[torch.randperm(K, generator=torch.Generator().manual_seed(K))]
    y, stat = conv_y(h, C, Hh, K, want_mm, offsets, seed=600 + C + K)
    mm = getattr(y, "_egz_mm", None)
    assert (mm is not None) == want_mm, "the conv did not take the bound route functions.py relies on"
    N = B * Hh * Hh
    gamma, beta, rm0, rv0 = bn_params(K, seed=601)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    nbt = torch.full((), 5, dtype=torch.int64, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    res = h.bn_finalize(stat, float(N), gd, bd, rm, rv, MOM, EPS, nbt, mm=mm if presplit_out else None)
    coef, am = res if presplit_out else (res, None)
    coef_plain = h.bn_finalize(stat, float(N), gd, bd, None, None, MOM, EPS)
    assert torch.equal(coef, coef_plain)                    # the bound form computes the same coefficients

    y64 = y.cpu().double().view(-1, K)
    mean = y64.mean(0)
    var = ((y64 - mean) ** 2).mean(0)
    std = var.sqrt()
    invstd = 1.0 / (var + EPS).sqrt()
    sc = gamma.double() * invstd
    sh = beta.double() - mean * sc
    c = coef.cpu().double()
    e = {"mean": ((c[0] - mean).abs() / (mean.abs() + std)).max().item(),
         "invstd": ((c[1] - invstd).abs() / invstd).max().item(),
         "scale": ((c[2] - sc).abs() / sc.abs()).max().item(),
         "shift": ((c[3] - sh).abs() / (beta.double().abs() + (mean * sc).abs())).max().item()}
    rm_ref = (1 - MOM) * rm0.double() + MOM * mean
    rv_ref = (1 - MOM) * rv0.double() + MOM * var * N / (N - 1)
    e["running_mean"] = ((rm.cpu().double() - rm_ref).abs() / ((1 - MOM) * rm0.double().abs() + MOM * (mean.abs() + std))).max().item()
    e["running_var"] = ((rv.cpu().double() - rv_ref).abs() / rv_ref).max().item()
    assert int(nbt.item()) == 6
    # colsum_f64 over the stat rows (the reduction behind the decoder's bias gradients): both planes
    rows = stat.shape[0]
    cs = h.colsum_f64(stat, 2 * K)
    e["colsum_f64"] = max(rel(cs[:K], y64.sum(0)), rel(cs[K:], (y64 * y64).sum(0)))
    # smallest defect: one stat row dropped (or counted twice) moves the mean by |row sum| / N
    d_mean = min((stat[r, 0].cpu().double().abs() / N / (mean.abs() + std)).max().item() for r in {0, rows // 2, rows - 1})
    d_cs = chunk_defect(stat[:, 0].cpu().double(), 1, y64.sum(0))
    print(f"B=32 {C}->{K} @{Hh}{' pool' if pool else ''} ({rows} stat rows): " + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + f"  | one stat row: mean {d_mean:.1e} std, colsum {d_cs:.1e}")
    bars = {"mean": 3e-7, "invstd": 3e-7, "scale": 5e-7, "shift": 1e-6, "running_mean": 6e-7, "running_var": 6e-7,
            "colsum_f64": 3e-7}
    for name, bar in bars.items():
        assert e[name] < bar, (name, e[name], bar)
    assert d_mean >= 10 * bars["mean"] and d_cs >= 10 * bars["colsum_f64"], (d_mean, d_cs)

    if presplit_out:
        # (a) the bound is the exact maximum of the block output
        out_ref = h.bn_relu_pool_fwd(y, coef, pool)
        bound = float(h.absmax_value(am))
        assert bound == float(out_ref.max()) == float(h.absmax_value(out_ref._egz_absmax))
        # (b) the pre-split output feeds the consumer's forward and weight gradient bit-identically to the fp32 output
        out_pre = h.bn_relu_pool_fwd(y, coef, pool, presplit_am=am)
        Ho = out_ref.shape[1]
        g = dev_gen(602)
        w1 = torch.randn(next_k, K, 3, 3, generator=g, device=DEV) * (2.0 / (9 * K)) ** 0.5
        b1 = 0.1 * torch.randn(next_k, generator=g, device=DEV)
        wp1, st1 = h.conv_weight(w1, "fwd", h.F16X3, out_ref, next_k)
        assert st1 and h.conv_dtype("fwd", next_k, K, out_ref) == h.F16X3
        y_ref, s_ref = h.conv3x3_fwd(out_ref, wp1, b1, next_k, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True)
        y_pre, s_pre = h.conv3x3_fwd(out_pre, wp1, b1, next_k, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True, pre_in=True)
        assert torch.equal(y_ref, y_pre) and torch.equal(s_ref, s_pre)
        del y_ref, y_pre
        dyn = torch.randn(B, Ho, Ho, next_k, generator=g, device=DEV) * 1e-3
        assert torch.equal(h.conv3x3_wgrad(out_ref, dyn, precision="split_f16"),
                           h.conv3x3_wgrad(out_pre, dyn, precision="split_f16", x_pre=True))
        del out_ref, out_pre, dyn
    if gpre:
        # (c) the pre-split gradient: a bound of max |dy| derived before the apply pass, dgamma / dbeta unchanged
        Ho = Hh // 2 if pool else Hh
        dout = torch.randn(B, Ho, Ho, K, generator=dev_gen(603), device=DEV) * 3e-4
        dy_ref, dg_ref, db_ref = h.bn_relu_pool_bwd(y, dout, coef, pool)
        dy_pre, dg_pre, db_pre = h.bn_relu_pool_bwd(y, dout, coef, pool, presplit=(h.absmax_of(dout), mm))
        assert torch.equal(dg_ref, dg_pre) and torch.equal(db_ref, db_pre)
        true_max, bound = float(dy_ref.abs().max()), float(h.absmax_value(dy_pre._egz_absmax))
        print(f"  pre-split gradient: max |dy| {true_max:.3e}, bound {bound:.3e} ({bound / true_max:.2f}x)")
        assert true_max <= bound <= 8 * true_max


# ------------------------------------------------------------------------------------------------ 1b. forward / backward
def grid_block_input(K, shape, seed):
    """Values on the 1/64 grid, +-4 around per-channel offsets of up to +-10 (about 4.3 std): exact in fp32, ties in pool
    windows at a rate of ~1 / 512 per pair."""
    g = dev_gen(seed)
    lv = torch.randint(-256, 256, shape, generator=g, device=DEV)
    off = torch.randint(-640, 641, (K,), generator=g, device=DEV)
    return (lv + off).float() / 64.0


def crossing_beta(y64, gamma, seed):
    """beta that puts each channel's ReLU zero crossing half a grid step between two levels (at mean + q std, |q| < 1), so that
    relu(y * scale + shift) and every pool decision are the same in fp32 and fp64: |z| >= |scale| / 128 everywhere."""
    K = y64.shape[-1]
    v = y64.reshape(-1, K)
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    q = 2 * torch.rand(K, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 1
    y0 = (torch.floor((mean + q * var.sqrt()) * 64) + 0.5) / 64
    return (-gamma.double() * (y0 - mean) / (var + EPS).sqrt()).float()


def bn_reference(y64, gamma, beta, pool, dout64):
    """fp64 [BN(train) -> ReLU (-> 2x2 max-pool)] forward and backward on NHWC y: (out, dy, dgamma, dbeta, per-row sums of dz
    and dz * xhat over the reduce kernel's pixel rows (output pixels when pooled), min |z| / |scale|)."""
    Bb, Hh, Ww, K = y64.shape
    v = y64.reshape(-1, K)
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    invstd = 1.0 / (var + EPS).sqrt()
    sc = gamma.double() * invstd
    sh = beta.double() - mean * sc
    z = y64 * sc + sh
    margin = (z.abs() / sc.abs()).min().item()
    if pool:
        Ho, Wo = Hh // 2, Ww // 2
        zz = z.view(Bb, Ho, 2, Wo, 2, K).permute(0, 1, 3, 5, 2, 4).reshape(Bb, Ho, Wo, K, 4)     # torch's scan order
        idx = zz.argmax(-1, keepdim=True)                                                     # first maximum wins
        mx = zz.gather(-1, idx)
        out = mx.squeeze(-1).clamp(min=0)
        dzz = torch.zeros_like(zz).scatter_(-1, idx, (dout64 * (out > 0)).unsqueeze(-1))
        dz = dzz.view(Bb, Ho, Wo, K, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(Bb, Hh, Ww, K)
        del zz, dzz, idx, mx
    else:
        out = z.clamp(min=0)
        dz = torch.where(z > 0, dout64, torch.zeros_like(dout64))
    del z
    xhat = (y64 - mean) * invstd
    dzx = dz * xhat
    del xhat
    dbeta, dgamma = dz.sum((0, 1, 2)), dzx.sum((0, 1, 2))
    n = Bb * Hh * Ww
    dy = sc * (dz - dbeta / n - (y64 - mean) * invstd * (dgamma / n))
    if pool:
        r1 = dz.view(Bb, Hh // 2, 2, Ww // 2, 2, K).sum((2, 4)).reshape(-1, K)
        r2 = dzx.view(Bb, Hh // 2, 2, Ww // 2, 2, K).sum((2, 4)).reshape(-1, K)
    else:
        r1, r2 = dz.reshape(-1, K), dzx.reshape(-1, K)
    return out, dy, dgamma, dbeta, r1, r2, margin


@pytest.mark.parametrize("C,Hh,K,pool,next_k", BN_BLOCKS + [("fusion", 14, 512, False, 0)])
def test_bn_relu_pool_elementwise_at_batch_32(C, Hh, K, pool, next_k):
    """[BN(train) -> ReLU (-> max-pool)] forward and backward entry by entry at B = 32 on grid-quantised inputs that no ReLU or
    pool decision can flip (exact ties still route to the first in scan order, at scale), on the route functions.py takes:
    the reduce pass (grid-stride, BWD_BLOCKS-capped), the sums the consumer's data gradient folds in (non-pooled encoder
    blocks, BNSUMS_WIDE), the one-pass BN backward + weight gradient of the RGB first block, the pair max of the fusion block.
    relu_bwd_bias and colsum run on the same geometry.
    Observed on MI355X (worst block): fwd 2.0e-7, dy 1.6e-7, dw (RGB) 1.9e-7, dgamma 2.1e-7, dbeta 1.6e-7, with the folded sums
    alike, relu_bwd_bias 2.0e-7, colsum 4.9e-8; bars 5x that.  One dropped grid-stride chunk moves dgamma / dbeta by >= 1.7e-3,
    the relu_bwd_bias sums by >= 2.9e-3 and colsum by >= 1.7e-3 of max |ref|."""
    h = H()
    fusion = C == "fusion"
    first, padded, _, _, first_wgrad = route(h, 512 if fusion else C, Hh, K, pool, next_k)
    Ho = Hh // 2 if pool else Hh
    shape = (B, Hh, Hh, K)
    if fusion:
        y2 = grid_block_input(K, (2 * B, Hh, Hh, K), seed=700)
        y = h.pairmax_fwd(y2)
        a, b = y2[:B].cpu(), y2[B:].cpu()
        assert torch.equal(y.cpu(), torch.where(a >= b, a, b))
        assert int((a == b).sum()) > 1000                      # ties: the s stream wins
    else:
        y = grid_block_input(K, shape, seed=701 + K + (C if isinstance(C, int) else 0))
    y64 = y.cpu().double()
    gamma, _, rm0, rv0 = bn_params(K, seed=702)
    beta = crossing_beta(y64, gamma, seed=703)
    stat = h.channel_stats(y)
    coef = h.bn_finalize(stat, float(B * Hh * Hh), gamma.to(DEV), beta.to(DEV), rm0.to(DEV), rv0.to(DEV), MOM, EPS)
    out = h.bn_relu_pool_fwd(y, coef, pool)
    g = dev_gen(704)
    sums = None
    if not fusion and not pool and next_k and h.bnsums_ok(B, Hh, Hh, K, next_k, h.conv_dtype("dgrad", K, next_k, y)):
        # dout as the step produces it: the data gradient of the next conv, which also accumulates this block's two sums
        dt = h.conv_dtype("dgrad", K, next_k, y)
        dyn = torch.randn(B, Hh, Hh, next_k, generator=g, device=DEV) * 1e-3
        wn = torch.randn(next_k, K, 3, 3, generator=g, device=DEV) * (2.0 / (9 * next_k)) ** 0.5
        wq, sq = h.conv_weight(wn, "dgrad", dt, dyn, K)
        assert sq
        dout, sums = h.conv3x3_dgrad_bnsums(dyn, wq, K, dt, y, coef)
        del dyn
    else:
        dout = torch.randn(B, Ho, Ho, K, generator=g, device=DEV)
    dout64 = dout.cpu().double()
    out_ref, dy_ref, dg_ref, db_ref, r1, r2, margin = bn_reference(y64, gamma, beta, pool, dout64)
    assert margin >= 1.0 / 256, margin                          # the construction keeps every decision away from a flip
    e = {"fwd": rel(out, out_ref)}
    del out_ref
    unit = bwd_rows_per_block(K)
    defect = min(chunk_defect(r1, unit, db_ref), chunk_defect(r2, unit, dg_ref))
    if first_wgrad:
        # RGB first block: BatchNorm backward + the conv's weight gradient in one pass (dy never stored)
        x = torch.randn(B, C, Hh, Hh, generator=g, device=DEV)
        dw, dg, db = h.bn_bwd_first_wgrad(y, dout, coef, x)
        dw_ref = torch.nn.grad.conv2d_weight(x.cpu().double(), (K, C, 3, 3), dy_ref.permute(0, 3, 1, 2), padding=1)
        e["dw"], e["dgamma"], e["dbeta"] = rel(dw, dw_ref), rel(dg, dg_ref), rel(db, db_ref)
        if sums is not None:
            dws, dgs, dbs = h.bn_bwd_first_wgrad(y, dout, coef, x, sums=sums)
            e["dw(sums)"], e["dgamma(sums)"], e["dbeta(sums)"] = rel(dws, dw_ref), rel(dgs, dg_ref), rel(dbs, db_ref)
        del x, dw_ref
    else:
        dy, dg, db = h.bn_relu_pool_bwd(y, dout, coef, pool)
        e["dy"], e["dgamma"], e["dbeta"] = rel(dy, dy_ref), rel(dg, dg_ref), rel(db, db_ref)
        if sums is not None:
            dys, dgs, dbs = h.bn_relu_pool_bwd(y, dout, coef, pool, sums=sums)
            e["dy(sums)"], e["dgamma(sums)"], e["dbeta(sums)"] = rel(dys, dy_ref), rel(dgs, dg_ref), rel(dbs, db_ref)
            del dys
        if fusion:
            dy2 = h.pairmax_bwd(y2, dy).cpu()
            dyc, zero = dy.cpu(), torch.zeros(B, Hh, Hh, K)
            assert torch.equal(dy2[:B], torch.where(a >= b, dyc, zero)) and torch.equal(dy2[B:], torch.where(a >= b, zero, dyc))
            del dy2, dyc
        del dy
    del dy_ref, r1, r2
    # ReLU backward + bias gradient and the plain column sum on the block output's geometry
    go = torch.randn(out.shape, generator=g, device=DEV)
    dyr, dbr = h.relu_bwd_bias(out, go)
    go64 = go.cpu().double()
    masked = go64 * (out.cpu() > 0)
    assert torch.equal(dyr.cpu(), masked.float())
    Kr = out.shape[-1]
    e["relu_bwd_bias"] = rel(dbr, masked.sum((0, 1, 2)))
    e["colsum"] = rel(h.colsum(go), go64.sum((0, 1, 2)))
    d_rb = chunk_defect(masked.view(-1, Kr), bwd_rows_per_block(Kr), masked.sum((0, 1, 2)))
    d_cs = chunk_defect(go64.view(-1, Kr), 8, go64.sum((0, 1, 2)))
    print(f"B=32 {C}->{K} @{Hh}{' pool' if pool else ''}{' (sums)' if sums is not None else ''}: "
          + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + f"  | one chunk: BN sums {defect:.1e}, relu_bwd_bias {d_rb:.1e}, colsum {d_cs:.1e}")
    bars = {"fwd": 1e-6, "dy": 1e-6, "dy(sums)": 1e-6, "dw": 1e-6, "dw(sums)": 1e-6, "dgamma": 1e-6, "dbeta": 1e-6,
            "dgamma(sums)": 1e-6, "dbeta(sums)": 1e-6, "relu_bwd_bias": 1e-6, "colsum": 3e-7}
    for name, err in e.items():
        assert err < bars[name], (name, err, bars[name])
    assert defect >= 10 * bars["dgamma"] and d_rb >= 10 * bars["relu_bwd_bias"] and d_cs >= 10 * bars["colsum"], (defect, d_rb, d_cs)


# ------------------------------------------------------------------------------------------------ head
def test_head_sigmoid_at_batch_32():
    """conv1x1 (64 -> 1) + sigmoid forward, backward and the backward with the ReLU mask of the block below folded in, at
    32 x 224 x 224 against fp64 from the same fp32 operands (the backward from the kernel's own fp32 output).
    Observed on MI355X: out 1.2e-7, dx 1.2e-7, dw 4.6e-8, db 7.6e-8, masked bias-gradient sums 1.5e-7; bars 5x that.  One
    dropped 16-pixel chunk moves dw by 3.6e-3, db by 4.7e-4, the masked sums by 1.9e-3."""
    h = H()
    C, Hh = 64, 224
    g = dev_gen(800)
    x = torch.randn(B, Hh, Hh, C, generator=g, device=DEV).clamp_(min=0)
    w = 0.2 * torch.randn(1, C, 1, 1, generator=g, device=DEV)
    bias = torch.full((1,), 0.1, device=DEV)
    out, _ = h.conv1x1_sigmoid_fwd(x, w, bias)
    x64, w64 = x.cpu().double().view(-1, C), w.cpu().double().view(C)
    out_ref = torch.sigmoid(x64 @ w64 + 0.1)
    e = {"out": rel(out.view(-1), out_ref)}
    dout = torch.randn(B, Hh, Hh, generator=g, device=DEV)
    o64 = out.cpu().double().view(-1)
    dl = dout.cpu().double().view(-1) * o64 * (1 - o64)
    del o64, out_ref
    dx, dw, db = h.conv1x1_sigmoid_bwd(x, w, out, dout)
    dx_ref = dl[:, None] * w64
    prod = dl[:, None] * x64
    dw_ref, db_ref = prod.sum(0), dl.sum().view(1)
    d_w = chunk_defect(prod, 16, dw_ref)
    del prod
    e["dx"], e["dw"], e["db"] = rel(dx.view(-1, C), dx_ref), rel(dw.view(C), dw_ref), rel(db, db_ref)
    dxm, dwm, dbm, mstat, am = h.conv1x1_sigmoid_bwd_masked(x, w, out, dout)
    mask = x64 > 0
    dxm_ref = dx_ref * mask
    assert torch.equal(dxm.view(-1, C).cpu(), (dx.view(-1, C).cpu() * mask).float())
    assert torch.equal(dwm, dw) and torch.equal(dbm, db)
    e["masked_bias"] = rel(h.colsum_f64(mstat, C), dxm_ref.sum(0))
    assert float(h.absmax_value(am)) == float(dxm.abs().max())
    d_b = chunk_defect(dl[:, None], 16, db_ref)
    d_m = chunk_defect(dxm_ref, 16, dxm_ref.sum(0))
    print("B=32 head 64->1 @224: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + f"  | one 16-pixel chunk: dw {d_w:.1e}, db {d_b:.1e}, masked bias {d_m:.1e}")
    bars = {"out": 6e-7, "dx": 6e-7, "dw": 3e-7, "db": 4e-7, "masked_bias": 8e-7}
    for name, err in e.items():
        assert err < bars[name], (name, err, bars[name])
    assert d_w >= 10 * bars["dw"] and d_b >= 10 * bars["db"] and d_m >= 10 * bars["masked_bias"], (d_w, d_b, d_m)


# ------------------------------------------------------------------------------------------------ 2. GEMM fast path
def gemm_operands(M, N, K, a_kfast, b_nfast, seed):
    """op(A) (M, K) and op(B) (K, N) stored with the unit stride along k / m (A) and n / k (B): (a, a_strides, b, b_strides)."""
    g = dev_gen(seed)
    a = torch.randn(M, K, generator=g, device=DEV) if a_kfast else torch.randn(K, M, generator=g, device=DEV)
    b = torch.randn(K, N, generator=g, device=DEV) if b_nfast else torch.randn(N, K, generator=g, device=DEV)
    return a, ((K, 1) if a_kfast else (1, M)), b, ((N, 1) if b_nfast else (1, K))


def misaligned(t):
    """A copy of t whose storage starts 4 bytes past a 16-byte boundary: egz_gemm's alignment test fails -> generic kernel."""
    buf = torch.empty(t.numel() + 4, device=t.device)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def op64(t, strides, rows, cols):
    return t.cpu().double().reshape(-1).as_strided((rows, cols), strides)


GEMM_BAR = 6e-6           # observed 1.1e-6 (K <= 512)
GEMM_BAR_K2048 = 1.2e-5   # observed 2.3e-6 (matmul_nn, K = 2048)


@pytest.mark.parametrize("a_kfast,b_nfast", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("MN", [1024, 512])          # t64 = 256 tiles: 2 x 2 waves of 32 x 32; 64 tiles: one wave per block
def test_gemm_fast_path_variants(MN, a_kfast, b_nfast):
    """egz_gemm's fast path in every (A_KFAST, B_NFAST) variant and both tiles, K = 64 .. 512 (nk = 1, 2, 3, 4, 8 slabs: the
    two-set prefetch schedule at its edges), against fp64; bias + ReLU, accumulate and a column-slice destination (ldc != N,
    neighbouring columns untouched).  Every result is also BIT-IDENTICAL to the generic kernel (the same operands copied to a
    4-byte offset fail the alignment test): same exact-f32 MFMA, same k order.
    Observed on MI355X: worst 1.1e-6 of max |ref| per variant; fast and generic kernels bit-identical everywhere."""
    h = H()
    M = N = MN
    worst = 0.0
    for K in (64, 128, 192, 256, 512):
        a, sa, b, sb = gemm_operands(M, N, K, a_kfast, b_nfast, seed=900 + K)
        am, bm = misaligned(a), misaligned(b)
        ref = op64(a, sa, M, K) @ op64(b, sb, K, N)
        bias = torch.randn(N, generator=dev_gen(901), device=DEV)
        c0 = torch.randn(M, N, generator=dev_gen(902), device=DEV)
        # plain
        got = h.gemm(a, b, M, N, K, sa, sb)
        assert torch.equal(got, h.gemm(am, bm, M, N, K, sa, sb))
        worst = max(worst, rel(got, ref))
        # bias + ReLU
        got = h.gemm(a, b, M, N, K, sa, sb, bias=bias, relu=True)
        assert torch.equal(got, h.gemm(am, bm, M, N, K, sa, sb, bias=bias, relu=True))
        worst = max(worst, rel(got, (ref + bias.cpu().double()).clamp(min=0)))
        # accumulate
        got = c0.clone()
        h.gemm(a, b, M, N, K, sa, sb, out=got, accumulate=True)
        gen = c0.clone()
        h.gemm(am, bm, M, N, K, sa, sb, out=gen, accumulate=True)
        assert torch.equal(got, gen)
        worst = max(worst, rel(got, ref + c0.cpu().double()))
        # destination = a column slice of a wider matrix (ldc = N + 128)
        wide = torch.randn(M, N + 128, generator=dev_gen(903), device=DEV)
        keep = wide.clone()
        dst = wide[:, 64:64 + N]
        h.gemm(a, b, M, N, K, sa, sb, out=dst, bias=bias)
        assert torch.equal(wide[:, :64], keep[:, :64]) and torch.equal(wide[:, 64 + N:], keep[:, 64 + N:])
        worst = max(worst, rel(dst, ref + bias.cpu().double()))
        wide2 = keep.clone()
        h.gemm(am, bm, M, N, K, sa, sb, out=wide2[:, 64:64 + N], bias=bias)
        assert torch.equal(wide, wide2)
    print(f"fast-path gemm {M}x{N} a_kfast={a_kfast} b_nfast={b_nfast}: worst {worst:.1e}")
    assert worst < GEMM_BAR


@pytest.mark.parametrize("R", [64, 128, 192, 512])
def test_gemm_at_step_shapes(R):
    """The AT step's products through the wrappers lstmnet uses, against fp64 and bit-identical to the generic kernel:
    gate projection 512 x 2048 x 512 (linear_fwd), Linear 512 x 512 x 512 with bias + ReLU, data gradient dY W
    (matmul_nn, K = 2048) and the weight gradients dgates^T [x | h] = 2048 x 512 x R (matmul_tn, R = T B).
    Observed on MI355X: <= 9.6e-7 of max |ref| for K = 512, <= 2.3e-6 for matmul_nn (K = 2048)."""
    h = H()
    g = dev_gen(950 + R)
    x = torch.randn(512, 512, generator=g, device=DEV)
    w_ih = torch.randn(2048, 512, generator=g, device=DEV) * 0.05
    w_lin = torch.randn(512, 512, generator=g, device=DEV) * 0.05
    b_lin = torch.randn(512, generator=g, device=DEV)
    dg = torch.randn(R, 2048, generator=g, device=DEV)
    xr = torch.randn(R, 512, generator=g, device=DEV)
    x64, wih64, wl64, bl64, dg64, xr64 = (t.cpu().double() for t in (x, w_ih, w_lin, b_lin, dg, xr))
    cases = [("linear 512x2048x512", lambda m: h.linear_fwd(m(x), m(w_ih)), x64 @ wih64.t()),
             ("linear+relu 512x512x512", lambda m: h.linear_fwd(m(x), m(w_lin), bias=b_lin, relu=True), (x64 @ wl64.t() + bl64).clamp(min=0)),
             (f"matmul_nn {R}x512x2048", lambda m: h.matmul_nn(m(dg), m(w_ih)), dg64 @ wih64),
             (f"matmul_tn 2048x512x{R}", lambda m: h.matmul_tn(m(dg), m(xr)), dg64.t() @ xr64)]
    errs = {}
    for name, fn, ref in cases:
        got = fn(lambda t: t)
        assert torch.equal(got, fn(misaligned)), name
        errs[name] = rel(got, ref)
    print("AT gemms: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < (GEMM_BAR_K2048 if "matmul_nn" in k else GEMM_BAR) for k, v in errs.items()), errs


def test_gemm_batched_matches_single_products():
    """egz_gemm_batched (matmul_tn_batched) with 1 .. 8 products, on the fast geometry (one launch) and on fallback geometries
    (K = 70, a misaligned operand: per-product egz_gemm), is bit-identical to the per-product egz_gemm; 9 products, the ReLU
    flag and mixed shapes are refused."""
    h = H()
    g = dev_gen(970)
    for R, M, N, mis in ((128, 256, 512, False), (512, 2048, 512, False), (70, 256, 128, False), (128, 256, 512, True)):
        a_list = [torch.randn(R, M, generator=g, device=DEV) for _ in range(8)]
        b_list = [torch.randn(R, N, generator=g, device=DEV) for _ in range(8)]
        if mis:
            a_list[3] = misaligned(a_list[3])
        singles = [h.matmul_tn(a, b) for a, b in zip(a_list, b_list)]
        for count in range(1, 9):
            res = h.matmul_tn_batched(a_list[:count], b_list[:count])
            for i in range(count):
                assert torch.equal(res[i], singles[i]), (R, M, N, mis, count, i)
        ref = a_list[0].cpu().double().t() @ b_list[0].cpu().double()
        assert rel(singles[0], ref) < GEMM_BAR
    a = [torch.randn(128, 256, device=DEV) for _ in range(9)]
    b = [torch.randn(128, 256, device=DEV) for _ in range(9)]
    with pytest.raises(RuntimeError):
        h.matmul_tn_batched(a, b)
    res = [torch.empty(256, 256, device=DEV) for _ in range(2)]
    with pytest.raises(RuntimeError):
        h.check(h.LIB.egz_gemm_batched(h._ptr_table(a[:2]), h._ptr_table(b[:2]), h._ptr_table(res), 2, 256, 256, 128, 1, 256,
                                       256, 1, 256, 2, h._stream()), "egz_gemm_batched(relu)")
    with pytest.raises(RuntimeError):
        h.matmul_tn_batched([a[0], torch.randn(128, 192, device=DEV)], [b[0], b[1]])
