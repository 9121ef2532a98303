"""The kernels of the late-fusion (LF) training step at the batch bench.py and LF.py train at (B = 32, 224 x 224), at
gaze_full.py's B = 64 and at a trailing partial batch, against float64.

test_hip_headline_ops.py pins the SP step's kernels at this geometry; the LF step runs its own code, which the whole-model LF
tests only bound loosely (per-tensor L2 2e-2, max-rel 0.1): the deferred BatchNorm of blocks 1 and 2 (the next conv applies
[BN -> ReLU] while it stages the pre-BN tensor, bn_finalize_deferred bounds the output nobody writes), the narrow conv and
data-gradient kernels with the BatchNorm-backward sums folded in, and the narrow weight gradients (32 x 32 and tap-packed
K = 8), which at B = 32 sum 512 splits of 49 patches through wgrad_fold_kernel -- one lost split moves dw by ~1/512, below
those bars.

Every operand comes from a real late_fusion training step (forward, floss, backward) on LF-like inputs: u8/255 maps of smooth
gaze-like blobs over large flat regions.  The step's hipops entry points are wrapped to record what each launch received and
returned, and each kernel is checked against float64 computed from exactly those fp32 operands and coefficients, so ReLU
decisions agree by construction.  Errors are max |got - ref| / max |ref|.  Each reduction assertion also computes, from the same
fp64 data, the error that dropping ONE chunk of that reduction would cause (a weight-gradient split, a stat row, a reduce
chunk) and requires it to be at least 10x the bar.

No kernel needed a fix.  One weakness is measured and bounded rather than fixed: on channels whose mean is large against their
spread, the one-pass variance of the BatchNorm finalize amplifies the fp32 rounding of the sum y^2 stat rows, so invstd is off
by up to 2.7e-5 here (test_lf_forward_chain).  On MI355X the file runs in 69 s with a peak host memory of 7.5 GB."""
import gc
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import egaze_oracle as O
from oracle import synth
from stream_perturb import poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S224 = 224
EPS, MOM = 1e-5, 0.1
CONV = (0, 3, 6)               # late_fusion.fusion child indices: the three 3x3 convs, their BatchNorms, the 1x1 head
BN = (1, 4, 7)
HEAD = 9


def H():
    import egaze_amd.hipops as h
    return h


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


def l2(got, ref):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def chunk_defect(contrib, unit, ref):
    """Error max |d| / max |ref| that dropping ONE chunk of ``unit`` consecutive rows of the per-row contributions ``contrib``
    (rows, K) fp64 would cause -- the smallest over the first, a middle and the last chunk."""
    n = contrib.shape[0]
    starts = {0, (n // 2) // unit * unit, (n - unit) // unit * unit}
    scale = ref.abs().max().item()
    return min(contrib[s:s + unit].sum(0).abs().max().item() for s in starts) / scale


def row_defect(rows, ref):
    """The same for partial rows a kernel wrote itself ((rows, K) fp64 that sum to ``ref``): one row dropped."""
    n = rows.shape[0]
    scale = ref.abs().max().item()
    return min(rows[r].abs().max().item() for r in {0, n // 2, n - 1}) / scale


def same(a, b):
    """a and b are the same fp32 buffer (autograd hands saved tensors / re-laid-out views back as new tensor objects)."""
    return a.data_ptr() == b.data_ptr() and a.numel() == b.numel()


def nchw64(t):
    """(B, H, W, C) fp32 device tensor -> (B, C, H, W) fp64 host view."""
    return t.detach().cpu().double().permute(0, 3, 1, 2)


def conv64(x, w, b=None):
    """fp64 3x3 / pad 1 convolution, NCHW, eight images at a time (bounded host memory)."""
    return torch.cat([torch.nn.functional.conv2d(x[i:i + 8], w, b, padding=1) for i in range(0, x.shape[0], 8)])


def dgrad64(w, dy):
    return torch.cat([torch.nn.grad.conv2d_input((d.shape[0], w.shape[1]) + tuple(d.shape[2:]), w, d, padding=1)
                      for d in dy.split(8)])


def wgrad64(x, dy, shape):
    return sum(torch.nn.grad.conv2d_weight(a, shape, d, padding=1) for a, d in zip(x.split(8), dy.split(8)))


def bn_relu64(y64, coef):
    """relu(fma(y, scale, shift)) as the kernels stage it (coefficient rows as received; the exact fp64 product + shift
    rounded once to fp32), in fp64."""
    c = coef.detach().cpu().double()
    return torch.addcmul(c[3], y64, c[2]).float().clamp_(min=0).double()


# ------------------------------------------------------------------------------------------------ narrow wgrad geometry
def narrow_wgrad_geometry(B, Hh=S224, W=S224, C=32, K=32):
    """(run width WD, patch rows R, patches, splits S, patches per split) of the narrow weight-gradient launch: a restatement
    of pick_narrow_x3 / npatch_x3n / pick_splits9 (csrc/conv3x3_wgrad.hip, X3_BLOCKS = 512)."""
    WD = 32 if W % 32 == 0 else 16
    R = 64 // WD
    npatch = B * ((Hh + R - 1) // R) * (W // WD)
    tiles = ((C + 63) // 64) * ((K + 63) // 64)
    S = max(1, min((512 + tiles - 1) // tiles, (npatch + 7) // 8))
    return WD, R, npatch, S, (npatch + S - 1) // S


def assert_narrow_wgrad_geometry(h, B, C, K):
    WD, R, npatch, S, pps = narrow_wgrad_geometry(B, C=C, K=K)
    n = 9 * C * K
    want = (S * n + ((S + 31) // 32 * n if S > 32 else 0)) * 4        # [S][n] partial tiles + the folded rows
    assert int(h.LIB.egz_conv3x3_wgrad_ws_bytes(B, S224, S224, C, K, h.WGRAD_SPLIT)) == want, (B, C, K, S)
    return WD, R, npatch, S, pps


def split_defect(x64, dy64, ref, B, C, K):
    """Error one dropped split of the narrow weight gradient would cause: dw of the patches of the first, a middle and the
    last non-empty split alone (x64, dy64: NCHW fp64), the smallest of the three, relative to max |ref|."""
    WD, R, npatch, S, pps = narrow_wgrad_geometry(B, C=C, K=K)
    cpr, rpi = S224 // WD, (S224 + R - 1) // R
    yy = torch.arange(S224).view(S224, 1)
    xx = torch.arange(S224).view(1, S224)
    out = []
    for s in {0, S // 2, (npatch - 1) // pps}:
        g0, g1 = s * pps, min(s * pps + pps, npatch)
        b0, b1 = g0 // (rpi * cpr), (g1 - 1) // (rpi * cpr)
        bs = torch.arange(b0, b1 + 1).view(-1, 1, 1)
        pidx = (bs * rpi + yy // R) * cpr + xx // WD
        mask = ((pidx >= g0) & (pidx < g1)).double().unsqueeze(1)
        d = torch.nn.grad.conv2d_weight(x64[b0:b1 + 1], (K, C, 3, 3), dy64[b0:b1 + 1] * mask, padding=1)
        out.append(d.abs().max().item())
    return min(out) / ref.abs().max().item()


def pixel_chunk_defect(x64, dy64, ref, K, C, rows=8):
    """Error of one dropped chunk of ``rows`` image rows of a weight-gradient reduction over the network input (NCHW fp64): the
    band through the brightest row of the first, a middle and the last image (the LF maps are exactly 0 outside their blobs,
    where a chunk contributes nothing), the smallest of the three."""
    out = []
    n = x64.shape[0]
    for b in {0, n // 2, n - 1}:
        r0 = min(max(int(x64[b].sum((0, 2)).argmax()) - rows // 2, 0), S224 - rows)
        mask = torch.zeros(1, 1, S224, S224, dtype=torch.float64)
        mask[..., r0:r0 + rows, :] = 1
        d = torch.nn.grad.conv2d_weight(x64[b:b + 1], (K, C, 3, 3), dy64[b:b + 1] * mask, padding=1)
        out.append(d.abs().max().item())
    return min(out) / ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ inputs and the real step
def lf_inputs(B, seed):
    """(im, feat, gt) as lateDataset yields them: u8/255 maps.  im and feat are smooth gaze-like blobs (1-3 per map, sigma
    8-24 px) over large exactly-flat regions, which gives the first conv's channels a large |mean| / std; gt is
    oracle.synth's quantised fixation Gaussian."""
    rs = np.random.RandomState(seed)
    r = np.arange(S224, dtype=np.float64)[:, None]
    c = np.arange(S224, dtype=np.float64)[None, :]

    def maps():
        out = np.zeros((B, 1, S224, S224))
        for b in range(B):
            for _ in range(rs.randint(1, 4)):
                cr, cc = rs.uniform(10, S224 - 10, 2)
                s, a = rs.uniform(8, 24), rs.uniform(0.4, 1.0)
                np.maximum(out[b, 0], a * np.exp(-((r - cr) ** 2 + (c - cc) ** 2) / (2 * s * s)), out=out[b, 0])
        return torch.from_numpy((np.round(255 * out) / 255).astype(np.float32))
    im, feat = maps(), maps()
    gt = torch.from_numpy(synth.synth_gt(B, S224, rs))
    return im, feat, gt


def lf_net(dead=None):
    """late_fusion with oracle.synth weights; every third BatchNorm gamma negative (the bound's max / min roles swap), conv
    biases of O(1).  ``dead``: block-1 channels whose beta is -1e4 (entirely ReLU-dead; |gamma xhat| < 1.5 sqrt(N) < 1e4)."""
    from egaze_amd.models.late_fusion import late_fusion
    net = late_fusion()
    sd = synth.synth_state_dict(O.lf_shapes(), seed=3, head_gain=0.5)
    for i in BN:
        K = sd[f"fusion.{i}.weight"].numel()
        sd[f"fusion.{i}.weight"] = sd[f"fusion.{i}.weight"] * torch.where(torch.arange(K) % 3 == 1, -1.0, 1.0)
    for i in CONV:
        sd[f"fusion.{i}.bias"] = sd[f"fusion.{i}.bias"] * 20
    if dead is not None:
        sd["fusion.1.bias"][dead] = -1e4
    net.load_state_dict(sd)
    return net.to(DEV)


# the hipops entry points of the LF step (and of the routes it could take instead)
TRACKED = ("cat2_planes", "conv_first_fwd", "conv3x3_fwd", "bn_finalize", "bn_finalize_deferred", "bn_eval_coeffs",
           "bn_relu_pool_fwd", "conv1x1_sigmoid_fwd", "floss_fwd", "floss_bwd", "conv1x1_sigmoid_bwd",
           "conv1x1_sigmoid_bwd_masked", "bn_relu_pool_bwd", "conv3x3_dgrad_bnsums", "conv3x3_dgrad", "conv3x3_wgrad",
           "bn_bwd_first_wgrad", "conv_first_wgrad", "channel_stats", "relu_bwd_bias")
INPLACE = ("running_mean", "running_var", "num_batches_tracked")


class Recorder:
    """Wraps the TRACKED hipops entry points (monkeypatch): each outermost call is recorded as (name, bound arguments, result,
    copies of the running statistics it updates in place).  ``poison``: poison() before every recorded launch."""

    def __init__(self, monkeypatch, poison_each=False):
        self.h = H()
        self.calls, self.depth, self.active, self.poison_each = [], 0, True, poison_each
        for name in TRACKED:
            fn = getattr(self.h, name)
            monkeypatch.setattr(self.h, name, self._wrap(name, fn, inspect.signature(fn)))

    def _wrap(self, name, fn, sig):
        def wrapped(*a, **kw):
            if not self.active or self.depth:
                return fn(*a, **kw)
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = dict(args.arguments)
            pre = {k: args[k].clone() for k in INPLACE if isinstance(args.get(k), torch.Tensor)}
            if self.poison_each:
                poison(self.h)
            self.depth += 1
            try:
                res = fn(*a, **kw)
            finally:
                self.depth -= 1
            self.calls.append({"name": name, "args": args, "pre": pre, "out": res})
            return res
        return wrapped

    def route(self):
        return [describe(c) for c in self.calls]


def describe(c):
    """The route-relevant key arguments of one recorded call."""
    n, a = c["name"], c["args"]
    if n == "conv_first_fwd":
        return f"{n}({a['x_nchw'].shape[1]}->{a['w'].shape[0]}, stats={a['stats']}, minmax={a['want_minmax']})"
    if n == "conv3x3_fwd":
        return (f"{n}({a['x'].shape[-1]}->{a['K']}, epi={a['epi']}, streamed={a['streamed']}, bn_in={a['bn_in'] is not None}, "
                f"minmax={a['want_minmax']})")
    if n in ("bn_finalize", "bn_finalize_deferred"):
        return f"{n}(K={a['stat'].shape[-1]})"
    if n == "bn_eval_coeffs":
        return f"{n}(K={a['running_mean'].numel()})"
    if n == "bn_relu_pool_fwd":
        return f"{n}(K={a['y'].shape[-1]}, pool={a['pool']})"
    if n == "bn_relu_pool_bwd":
        return f"{n}(K={a['y'].shape[-1]}, sums={a['sums'] is not None})"
    if n in ("conv1x1_sigmoid_fwd", "conv1x1_sigmoid_bwd", "conv1x1_sigmoid_bwd_masked"):
        return f"{n}(C={a['x'].shape[-1]})"
    if n == "conv3x3_dgrad_bnsums":
        return f"{n}({a['dy'].shape[-1]}->{a['C']})"
    if n == "conv3x3_dgrad":
        return f"{n}({a['dy'].shape[-1]}->{a['C']})"
    if n == "conv3x3_wgrad":
        return f"{n}(C={a['x'].shape[-1]}, K={a['dy'].shape[-1]}, x_bn={a['x_bn'] is not None})"
    if n == "bn_bwd_first_wgrad":
        return f"{n}(C={a['x_nchw'].shape[1]}, K={a['y'].shape[-1]}, sums={a['sums'] is not None})"
    return n


TRAIN_ROUTE = [
    "cat2_planes",
    "conv_first_fwd(2->32, stats=True, minmax=True)",
    "bn_finalize_deferred(K=32)",
    "conv3x3_fwd(32->32, epi=2, streamed=True, bn_in=True, minmax=True)",
    "bn_finalize_deferred(K=32)",
    "conv3x3_fwd(32->8, epi=2, streamed=True, bn_in=True, minmax=False)",
    "bn_finalize(K=8)",
    "bn_relu_pool_fwd(K=8, pool=False)",
    "conv1x1_sigmoid_fwd(C=8)",
    "floss_fwd",
    "floss_bwd",
    "conv1x1_sigmoid_bwd(C=8)",
    "bn_relu_pool_bwd(K=8, sums=False)",
    "conv3x3_wgrad(C=32, K=8, x_bn=True)",
    "conv3x3_dgrad_bnsums(8->32)",
    "bn_relu_pool_bwd(K=32, sums=True)",
    "conv3x3_wgrad(C=32, K=32, x_bn=True)",
    "conv3x3_dgrad_bnsums(32->32)",
    "bn_bwd_first_wgrad(C=2, K=32, sums=True)",
]
EVAL_ROUTE = [
    "cat2_planes",
    "conv_first_fwd(2->32, stats=False, minmax=False)",
    "bn_eval_coeffs(K=32)",
    "bn_relu_pool_fwd(K=32, pool=False)",
    "conv3x3_fwd(32->32, epi=0, streamed=True, bn_in=False, minmax=False)",
    "bn_eval_coeffs(K=32)",
    "bn_relu_pool_fwd(K=32, pool=False)",
    "conv3x3_fwd(32->8, epi=0, streamed=True, bn_in=False, minmax=False)",
    "bn_eval_coeffs(K=8)",
    "bn_relu_pool_fwd(K=8, pool=False)",
    "conv1x1_sigmoid_fwd(C=8)",
]


def train_step(rec, B, seed=41, dead=None):
    """One late_fusion training step (LF.py:90-100 without the optimizer) under the recorder -> (net, im, feat, gt, calls by
    route position)."""
    from egaze_amd.floss import floss
    im, feat, gt = lf_inputs(B, seed)
    net = lf_net(dead)
    net.train()
    rec.calls.clear()
    rec.active = True
    out = net(feat.to(DEV), im.to(DEV))                       # LF.py:90 argument order
    floss()(out, gt.to(DEV)).backward()
    torch.cuda.synchronize()
    rec.active = False
    return net, im, feat, gt, rec.calls


# ------------------------------------------------------------------------------------------------ 1. route pin
@pytest.mark.parametrize("B", [32, 64])
def test_lf_step_route(B, monkeypatch):
    """The launches of one late_fusion training step at B = 32 (LF.py, bench.py's extra.lf_step) and 64 (gaze_full.py), with
    their key arguments: deferred BatchNorm for blocks 1 and 2 (min / max rows, bn_finalize_deferred, the next conv and weight
    gradient normalising on load), folded BatchNorm-backward sums in both narrow data gradients, the one-pass first-block
    backward.  The per-kernel tests below follow this route; if it changes, they need extending.  With hipops.BN_DEFER or
    hipops.BNSUMS_FUSE off the step takes another route, which this assertion tells apart."""
    h = H()
    rec = Recorder(monkeypatch)
    d0, s0 = h.BN_DEFER_STATS["deferred"], dict(h.BNSUMS_STATS)
    train_step(rec, B)
    assert rec.route() == TRAIN_ROUTE, "\n".join(rec.route())
    assert h.BN_DEFER_STATS["deferred"] - d0 == 2
    assert (h.BNSUMS_STATS["produced"] - s0["produced"], h.BNSUMS_STATS["consumed"] - s0["consumed"]) == (2, 2)
    for knob in ("BN_DEFER", "BNSUMS_FUSE"):
        with monkeypatch.context() as m:
            m.setattr(h, knob, False)
            train_step(rec, B)
            other = rec.route()
        print(f"B={B} {knob}=False route:\n  " + "\n  ".join(other))
        assert other != TRAIN_ROUTE
        assert not any("bn_finalize_deferred" in r or "bn_in=True" in r for r in other)
        if knob == "BNSUMS_FUSE":
            assert not any("dgrad_bnsums" in r or "sums=True" in r for r in other)


def test_narrow_wgrad_geometry():
    """The narrow weight gradient's launch geometry (restated from csrc/conv3x3_wgrad.hip and confirmed through
    egz_conv3x3_wgrad_ws_bytes, which grows with the split count): 224-wide rows take the 2 x 32 patch; B = 32 -> 25,088
    patches in 512 splits of 49, B = 64 -> 50,176 in 512 of 98 (both > RG = 32: wgrad_fold_kernel, then the tile reduce for
    K = 32 / the generic reduce for K = 8); the trailing batch of 7 -> 5,488 patches, 11 per split, splits 499-511 empty."""
    h = H()
    for K in (32, 8):
        assert assert_narrow_wgrad_geometry(h, 32, 32, K) == (32, 2, 25088, 512, 49)
        assert assert_narrow_wgrad_geometry(h, 64, 32, K) == (32, 2, 50176, 512, 98)
        assert assert_narrow_wgrad_geometry(h, 7, 32, K) == (32, 2, 5488, 512, 11)
    _, _, npatch, S, pps = narrow_wgrad_geometry(7)
    assert [s for s in range(S) if s * pps >= npatch] == list(range(499, 512))


# ------------------------------------------------------------------------------------------------ 2. forward chain
FWD_BARS = {"y1": 1.1e-6, "y2": 3.3e-6, "y3": 3e-6, "stat_sum": 1.1e-9, "stat_sumsq": 5.5e-8, "mean": 2.7e-7,
            "invstd/cond": 3e-7, "scale/cond": 4.5e-7, "shift/cond": 6.5e-7, "running_mean": 4.4e-7, "running_var": 5e-7,
            "out3": 1e-7, "head": 6e-7, "invstd_raw": float("inf"), "cond": float("inf")}


def check_forward(net, im, feat, calls, B, defects=True):
    """Forward chain of a recorded training step (TRAIN_ROUTE positions 1-8) against fp64: each block's conv output element
    by element, its stat rows (sum y, sum y^2), its min / max rows (bit-equal), the finalize coefficients / running statistics
    / num_batches_tracked / abs-max bound.  Returns (errors, defects)."""
    h = H()
    N = B * S224 * S224
    e, d = {}, {}
    x64 = torch.cat((feat, im), 1).double()
    assert torch.equal(calls[0]["out"].cpu(), torch.cat((feat, im), 1))
    prev = None                                         # (pre-BN y, coef) of the deferred block below
    for blk, pos in enumerate((1, 3, 5)):
        c = calls[pos]
        conv, bn = net.fusion[CONV[blk]], net.fusion[BN[blk]]
        y, stat = c["out"]
        K = y.shape[-1]
        w64, b64 = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
        xin = x64 if blk == 0 else bn_relu64(prev[0].detach().cpu().double(), prev[1]).permute(0, 3, 1, 2)
        if blk:
            assert same(c["args"]["bn_in"], prev[1]) and same(c["args"]["x"], prev[0])
        y_ref = conv64(xin, w64, b64)
        del xin
        e[f"y{blk + 1}"] = rel(y.permute(0, 3, 1, 2), y_ref)
        del y_ref
        y64 = y.detach().cpu().double().view(-1, K)
        s1, s2 = y64.sum(0), (y64 * y64).sum(0)
        e["stat_sum"] = max(e.get("stat_sum", 0), rel(stat[:, 0].sum(0), s1))
        e["stat_sumsq"] = max(e.get("stat_sumsq", 0), rel(stat[:, 1].sum(0), s2))
        if defects:
            st = stat.cpu()
            d[f"stat rows {blk + 1}"] = min(row_defect(st[:, 0], s1), row_defect(st[:, 1], s2))
        mm = getattr(y, "_egz_minmax", None)
        if blk < 2:
            yd = y.view(-1, K)
            assert torch.equal(mm[:, 0].amax(0), yd.amax(0)) and torch.equal(mm[:, 1].amin(0), yd.amin(0)), f"block {blk + 1} min / max rows"
        # finalize: coefficients from the stat rows, running statistics, the counter, the bound
        f = calls[pos + 1]
        coef = f["out"][0] if f["name"] == "bn_finalize_deferred" else f["out"]
        mean = s1 / N
        var = ((y64 - mean) ** 2).mean(0)
        std, invstd = var.sqrt(), 1.0 / (var + EPS).sqrt()
        g64, bt64 = bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()
        sc = g64 * invstd
        sh = bt64 - mean * sc
        cc = coef.cpu().double()
        # var = sum y^2 / N - mean^2 from the stat rows: a relative error d of the sum y^2 rows (fp32 within a tile) moves
        # invstd by d / 2 * cond, cond = (var + mean^2) / (var + eps), large on these flat-background channels
        cond = (var + mean * mean) / (var + EPS)
        e["cond"] = max(e.get("cond", 0), cond.max().item())
        raw = ((cc[1] - invstd).abs() / invstd)
        e["invstd_raw"] = max(e.get("invstd_raw", 0), raw.max().item())
        e["mean"] = max(e.get("mean", 0), ((cc[0] - mean).abs() / (mean.abs() + std)).max().item())
        e["invstd/cond"] = max(e.get("invstd/cond", 0), (raw / cond).max().item())
        e["scale/cond"] = max(e.get("scale/cond", 0), ((cc[2] - sc).abs() / sc.abs() / cond).max().item())
        e["shift/cond"] = max(e.get("shift/cond", 0), ((cc[3] - sh).abs() / (bt64.abs() + (mean * sc).abs()) / cond).max().item())
        rm0, rv0 = f["pre"]["running_mean"].cpu().double(), f["pre"]["running_var"].cpu().double()
        rm_ref = (1 - MOM) * rm0 + MOM * mean
        rv_ref = (1 - MOM) * rv0 + MOM * var * N / (N - 1)
        e["running_mean"] = max(e.get("running_mean", 0), ((bn.running_mean.cpu().double() - rm_ref).abs()
                                                           / ((1 - MOM) * rm0.abs() + MOM * (mean.abs() + std))).max().item())
        e["running_var"] = max(e.get("running_var", 0), ((bn.running_var.cpu().double() - rv_ref).abs() / rv_ref).max().item())
        assert int(bn.num_batches_tracked) == int(f["pre"]["num_batches_tracked"]) + 1 == 1
        if defects:
            d[f"finalize mean {blk + 1}"] = min((st[r, 0].double().abs() / N / (mean.abs() + std)).max().item()
                                                for r in {0, st.shape[0] // 2, st.shape[0] - 1})
        if f["name"] == "bn_finalize_deferred":
            am = f["out"][1]
            out_mat = h.bn_relu_pool_fwd(y, coef, False)
            assert float(h.absmax_value(am)) == float(out_mat.max()), f"block {blk + 1} deferred bound"
            del out_mat
        else:
            a = calls[pos + 2]
            assert same(a["args"]["coef"], coef) and same(a["args"]["y"], y)
            e["out3"] = rel(a["out"], bn_relu64(y.cpu().double(), coef))
        prev = (y, coef)
        del y64
    # the 1x1 head + sigmoid on block 3's output (conv1x1_sigmoid_fwd)
    hc = calls[8]
    a3 = hc["args"]["x"]
    assert same(a3, calls[7]["out"])
    w = net.fusion[HEAD].weight.detach().cpu().double().view(-1)
    b = net.fusion[HEAD].bias.detach().cpu().double()
    ref = torch.sigmoid(a3.cpu().double().view(-1, w.numel()) @ w + b)
    e["head"] = rel(hc["out"][0].view(-1), ref)
    return e, d


@pytest.mark.parametrize("B", [32, 64])
def test_lf_forward_chain(B, monkeypatch):
    """Forward pass of the LF training step at B = 32 / 64 along TRAIN_ROUTE, block by block against fp64: conv_first_fwd with
    min / max rows, the deferred-input narrow conv (BatchNorm + ReLU applied while staging) with and without min / max rows,
    the stat rows (summed), bn_finalize_deferred (mean, invstd, scale, shift, running statistics, num_batches_tracked; its
    bound BIT-EQUAL to the max of the materialised bn_relu_pool_fwd output), bn_finalize + bn_relu_pool_fwd for K = 8, the 1x1
    head.  Observed on MI355X (worst of B = 32 / 64 / 7 / 8): y1 2.2e-7, y2 6.5e-7, y3 5.6e-7, stat rows 2.1e-10 (sum y) and
    1.1e-8 (sum y^2), mean 5.4e-8 of |mean| + std, running_mean 8.8e-8, running_var 1.0e-7, head 1.2e-7, the K = 8 apply pass
    bit-exact; bars 5x that.  invstd / scale / shift are off by up to 2.7e-5 raw, above the 3e-7 of the SP statistics test,
    for a stated reason: the finalize forms var = sum y^2 / N - mean^2, and these flat-background channels have (var + mean^2) /
    (var + eps) up to 5.0e3, which multiplies the ~1e-8 rounding of the sum y^2 rows.  The bars therefore apply to the error
    divided by that factor (observed 4.5e-8 / 8.9e-8 / 1.3e-7; bars 3e-7 / 4.5e-7 / 6.5e-7).  One dropped stat row moves the
    sums or the mean by >= 1.5e-3."""
    rec = Recorder(monkeypatch)
    net, im, feat, gt, calls = train_step(rec, B)
    assert rec.route() == TRAIN_ROUTE
    e, d = check_forward(net, im, feat, calls, B)
    print(f"B={B} LF forward: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + " | one chunk: " + "  ".join(f"{k} {v:.1e}" for k, v in d.items()))
    for k, v in e.items():
        assert v < FWD_BARS[k], (k, v, FWD_BARS[k])
    for k, v in d.items():
        bar = FWD_BARS["mean"] if "mean" in k else FWD_BARS["stat_sum"]
        assert v >= 10 * bar, (k, v, bar)


# ------------------------------------------------------------------------------------------------ 3. eval forward
def test_lf_eval_forward(monkeypatch):
    """The validation loop's forward (LF.py's val loop, model.eval() under no_grad) at B = 32: bn_eval_coeffs (scale, shift
    from the running statistics), the narrow conv with the bias epilogue (EPI_BIAS), bn_relu_pool_fwd and the head, each
    against fp64 of its own operands.  Observed on MI355X: y1 1.7e-7, y2 3.6e-7, y3 6.0e-7, scale 1.2e-7, shift 8.9e-8,
    bn_relu_pool_fwd bit-exact, head 1.0e-7; bars about 5x that."""
    B = 32
    rec = Recorder(monkeypatch)
    im, feat, _ = lf_inputs(B, 43)
    net = lf_net()
    net.eval()
    with torch.no_grad():
        net(feat.to(DEV), im.to(DEV))
    torch.cuda.synchronize()
    rec.active = False
    calls = rec.calls
    assert rec.route() == EVAL_ROUTE, "\n".join(rec.route())
    e = {}
    xin = torch.cat((feat, im), 1).double()
    for blk, (pc, pcoef, pbn) in enumerate(((1, 2, 3), (4, 5, 6), (7, 8, 9))):
        conv, bn = net.fusion[CONV[blk]], net.fusion[BN[blk]]
        y = calls[pc]["out"][0]
        y_ref = conv64(xin, conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double())
        e[f"y{blk + 1}"] = rel(y.permute(0, 3, 1, 2), y_ref)
        del y_ref
        coef = calls[pcoef]["out"]
        inv = 1.0 / (bn.running_var.cpu().double() + EPS).sqrt()
        sc = bn.weight.detach().cpu().double() * inv
        sh = bn.bias.detach().cpu().double() - bn.running_mean.cpu().double() * sc
        e["eval_scale"] = max(e.get("eval_scale", 0), rel(coef[2], sc))
        e["eval_shift"] = max(e.get("eval_shift", 0), ((coef[3].cpu().double() - sh).abs()
                                                      / (bn.bias.detach().cpu().double().abs() + (bn.running_mean.cpu().double() * sc).abs())).max().item())
        out = calls[pbn]["out"]
        assert same(calls[pbn]["args"]["y"], y) and same(calls[pbn]["args"]["coef"], coef)
        ref = bn_relu64(y.cpu().double(), coef)
        e["bn_relu"] = max(e.get("bn_relu", 0), rel(out, ref))
        xin = ref.permute(0, 3, 1, 2)
        if blk < 2:
            assert same(calls[pc + 3]["args"]["x"], out)
    hc = calls[10]
    w = net.fusion[HEAD].weight.detach().cpu().double().view(-1)
    ref = torch.sigmoid(xin.permute(0, 2, 3, 1).reshape(-1, 8) @ w + net.fusion[HEAD].bias.detach().cpu().double())
    e["head"] = rel(hc["out"][0].view(-1), ref)
    print("B=32 LF eval forward: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
    bars = {"y1": 1e-6, "y2": 3e-6, "y3": 3e-6, "eval_scale": 6e-7, "eval_shift": 5e-7, "bn_relu": 1e-7, "head": 6e-7}
    for k, v in e.items():
        assert v < bars[k], (k, v, bars[k])


# ------------------------------------------------------------------------------------------------ 4. head and loss
def test_lf_head_and_floss(monkeypatch):
    """The 1x1 head (C = 8) and floss at B = 32 on the step's own tensors: conv1x1_sigmoid_fwd, floss_fwd against the oracle's
    fp64 floss_forward on the same fp32 map, floss_bwd against its fp64 autograd gradient, conv1x1_sigmoid_bwd (dx, the
    8-entry dw, db) against fp64 from the kernel's own fp32 output and gradient.  Observed on MI355X: out 1.1e-7, loss 7.6e-9,
    floss_bwd 1.5e-7, dx 9.8e-8, dw 1.9e-8, db 2.2e-8; bars about 5x that.  One dropped 16-pixel chunk of the head reduce moves
    dw by 8.4e-6 and db by 5.7e-6."""
    B = 32
    rec = Recorder(monkeypatch)
    net, im, feat, gt, calls = train_step(rec, B)
    assert rec.route() == TRAIN_ROUTE
    e = {}
    fc, lf, lb, hb = calls[8], calls[9], calls[10], calls[11]
    x = fc["args"]["x"]
    out = fc["out"][0]
    C = x.shape[-1]
    x64 = x.cpu().double().view(-1, C)
    w64 = net.fusion[HEAD].weight.detach().cpu().double().view(C)
    b64 = net.fusion[HEAD].bias.detach().cpu().double()
    e["out"] = rel(out.view(-1), torch.sigmoid(x64 @ w64 + b64))
    # floss on the kernel's own fp32 map
    assert lf["args"]["inp"].data_ptr() == out.data_ptr()
    o64 = out.detach().cpu().double().view(B, 1, S224, S224).requires_grad_(True)
    loss_ref = O.floss_forward(o64, gt.double())
    loss_ref.backward()
    e["loss"] = abs(float(lf["out"][0]) - loss_ref.item()) / abs(loss_ref.item())
    e["floss_bwd"] = rel(lb["out"].view(-1), o64.grad.view(-1))
    # head backward from the floss gradient the step fed it
    dout = hb["args"]["dout"]
    assert dout.data_ptr() == lb["out"].data_ptr()
    dx, dw, db = hb["out"]
    ov = o64.detach().view(-1)
    dl = dout.cpu().double().view(-1) * ov * (1 - ov)
    e["dx"] = rel(dx.view(-1, C), dl[:, None] * w64)
    prod = dl[:, None] * x64
    dw_ref, db_ref = prod.sum(0), dl.sum().view(1)
    e["dw"], e["db"] = rel(dw.view(C), dw_ref), rel(db, db_ref)
    d_w, d_b = chunk_defect(prod, 16, dw_ref), chunk_defect(dl[:, None], 16, db_ref)
    print("B=32 LF head + floss: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + f"  | one 16-pixel chunk: dw {d_w:.1e}, db {d_b:.1e}")
    bars = {"out": 6e-7, "loss": 4e-8, "floss_bwd": 8e-7, "dx": 5e-7, "dw": 1e-7, "db": 1.2e-7}
    for k, v in e.items():
        assert v < bars[k], (k, v, bars[k])
    assert d_w >= 10 * bars["dw"] and d_b >= 10 * bars["db"], (d_w, d_b)


# ------------------------------------------------------------------------------------------------ 5. backward chain
BWD_BARS = {"dy3": 6e-7, "dgamma3": 3e-7, "dbeta3": 1.5e-7, "dw3": 1.5e-5, "dx3": 1.6e-6, "sums3_dz": 9e-7, "sums3_dzx": 2.5e-7,
            "dy2": 5e-7, "dgamma2": 2.6e-7, "dbeta2": 1e-6, "dw2": 7e-6, "dx2": 3e-6, "sums2_dz": 8e-8, "sums2_dzx": 1.5e-7,
            "dw1": 4e-7, "dgamma1": 2.5e-7, "dbeta1": 2.2e-7}
TWO_PRODUCT_BARS = (2e-3, 1e-3)          # per entry, relative L2 (test_conv_ops_elementwise_at_the_headline_geometry)


def bn_bwd64(y, dout, coef):
    """fp64 BatchNorm(train) + ReLU backward from the fp32 operands and the coefficient rows the kernel received:
    (dy NHWC, dgamma, dbeta, per-pixel dz, dz * xhat as (N, K))."""
    K = y.shape[-1]
    y64, d64 = y.detach().cpu().double(), dout.detach().cpu().double()
    c = coef.detach().cpu().double()
    mean, invstd, sc, sh = c
    live = torch.addcmul(sh, y64, sc).float() > 0
    dz = torch.where(live, d64, torch.zeros((), dtype=torch.float64))
    del d64, live
    xhat = (y64 - mean) * invstd
    del y64
    dzx = dz * xhat
    n = dz.numel() // K
    dbeta, dgamma = dz.view(-1, K).sum(0), dzx.view(-1, K).sum(0)
    dy = sc * (dz - dbeta / n - xhat * (dgamma / n))
    return dy, dgamma, dbeta, dz.view(-1, K), dzx.view(-1, K)


def bnsums64(dx, y, coef):
    """fp64 (sum dz, sum dz * xhat) of the BatchNorm below, from the data gradient the kernel itself wrote."""
    K = y.shape[-1]
    c = coef.detach().cpu().double()
    y64 = y.detach().cpu().double()
    dz = torch.where(torch.addcmul(c[3], y64, c[2]).float() > 0, dx.detach().cpu().double(), torch.zeros((), dtype=torch.float64))
    return dz.view(-1, K).sum(0), (dz * ((y64 - c[0]) * c[1])).view(-1, K).sum(0)


def check_backward(net, im, feat, calls, B, defects=True, two_products=None):
    """Backward chain of a recorded training step (TRAIN_ROUTE positions 12-18) against fp64.  ``two_products``: a callable that
    switches hipops to the opt-in two-product backward; the narrow dgrad / wgrad launches are then repeated on the same operands.
    Returns (errors, defects, two-product errors)."""
    h = H()
    e, d, e2 = {}, {}, {}
    ys = [calls[p]["out"][0] for p in (1, 3, 5)]
    coefs = [calls[2]["out"][0], calls[4]["out"][0], calls[6]["out"]]
    # block 3 (K = 8): own reduce
    c = calls[12]
    assert same(c["args"]["y"], ys[2]) and same(c["args"]["coef"], coefs[2]) and c["args"]["sums"] is None
    assert same(c["args"]["dout"], calls[11]["out"][0])
    dy3, dg3, db3 = c["out"]
    dref, gref, bref, r1, r2 = bn_bwd64(ys[2], c["args"]["dout"], coefs[2])
    e["dy3"], e["dgamma3"], e["dbeta3"] = rel(dy3, dref), rel(dg3, gref), rel(db3, bref)
    if defects:
        d["bn reduce K=8"] = min(chunk_defect(r1, 128, bref), chunk_defect(r2, 128, gref))
    del dref, r1, r2
    dy_by_blk = {3: dy3}
    for blk, (pw, pd) in ((3, (13, 14)), (2, (16, 17))):
        K = 8 if blk == 3 else 32
        cw, cd = calls[pw], calls[pd]
        y_in, coef_in = ys[blk - 2], coefs[blk - 2]               # the deferred input of this block: block (blk - 1)'s pre-BN y
        dy = dy_by_blk[blk]
        assert same(cw["args"]["x"], y_in) and same(cw["args"]["x_bn"], coef_in) and same(cw["args"]["dy"], dy)
        assert same(cd["args"]["dy"], dy) and same(cd["args"]["bn_y"], y_in) and same(cd["args"]["coef"], coef_in)
        w64 = net.fusion[CONV[blk - 1]].weight.detach().cpu().double()
        dy64 = nchw64(dy)
        # weight gradient with the deferred input
        xn = bn_relu64(y_in.detach().cpu().double(), coef_in).permute(0, 3, 1, 2)
        dw_ref = wgrad64(xn, dy64, (K, 32, 3, 3))
        e[f"dw{blk}"] = rel(cw["out"], dw_ref)
        if defects:
            d[f"wgrad split K={K}"] = split_defect(xn, dy64, dw_ref, B, 32, K)
        del xn
        # data gradient + the folded BatchNorm-backward sums of the block below
        dx, sums = cd["out"]
        dx_ref = dgrad64(w64, dy64)
        e[f"dx{blk}"] = rel(dx.permute(0, 3, 1, 2), dx_ref)
        del dx_ref
        s_dz, s_dzx = bnsums64(dx, y_in, coef_in)
        ss = sums.cpu()
        e[f"sums{blk}_dz"], e[f"sums{blk}_dzx"] = rel(ss[:, 0].sum(0), s_dz), rel(ss[:, 1].sum(0), s_dzx)
        if defects:
            d[f"bn sums rows {blk}"] = min(row_defect(ss[:, 0], s_dz), row_defect(ss[:, 1], s_dzx))
        if two_products is not None:
            two_products()
            dw_p2 = h.conv3x3_wgrad(**cw["args"])
            dx_p2, sums_p2 = h.conv3x3_dgrad_bnsums(**cd["args"])
            dx_ref = dgrad64(w64, dy64)
            e2[f"dw{blk}"] = (rel(dw_p2, dw_ref), l2(dw_p2, dw_ref))
            e2[f"dx{blk}"] = (rel(dx_p2.permute(0, 3, 1, 2), dx_ref), l2(dx_p2.permute(0, 3, 1, 2), dx_ref))
            del dx_ref
            p_dz, p_dzx = bnsums64(dx_p2, y_in, coef_in)
            sp = sums_p2.cpu()
            e2[f"sums{blk}"] = (max(rel(sp[:, 0].sum(0), p_dz), rel(sp[:, 1].sum(0), p_dzx)), 0.0)
            del dx_p2
        del dy64, dw_ref
        # the BatchNorm backward of the block below with the folded sums (block 2), or the one-pass first block
        if blk == 3:
            c = calls[15]
            assert same(c["args"]["y"], ys[1]) and same(c["args"]["dout"], dx) and same(c["args"]["sums"], sums)
            dy2, dg2, db2 = c["out"]
            dref, gref, bref, _, _ = bn_bwd64(ys[1], dx, coefs[1])
            e["dy2"], e["dgamma2"], e["dbeta2"] = rel(dy2, dref), rel(dg2, gref), rel(db2, bref)
            del dref
            dy_by_blk[2] = dy2
        else:
            c = calls[18]
            assert same(c["args"]["y"], ys[0]) and same(c["args"]["dout"], dx) and same(c["args"]["sums"], sums)
            dw1, dg1, db1 = c["out"]
            dref, gref, bref, _, _ = bn_bwd64(ys[0], dx, coefs[0])
            x64 = torch.cat((feat, im), 1).double()
            assert torch.equal(c["args"]["x_nchw"].cpu(), torch.cat((feat, im), 1))
            d1 = dref.permute(0, 3, 1, 2)
            dw1_ref = wgrad64(x64, d1, (32, 2, 3, 3))
            e["dw1"], e["dgamma1"], e["dbeta1"] = rel(dw1, dw1_ref), rel(dg1, gref), rel(db1, bref)
            if defects:
                d["first wgrad 8-row chunk"] = pixel_chunk_defect(x64, d1, dw1_ref, 32, 2, rows=8)
            del dref, d1, x64
    return e, d, e2


@pytest.mark.parametrize("B", [32, 64])
def test_lf_backward_chain(B, monkeypatch, request):
    """Backward pass of the LF training step at B = 32 / 64 along TRAIN_ROUTE, from the real floss gradient, against fp64 of each
    kernel's own operands: bn_relu_pool_bwd for K = 8 (own grid-stride reduce) and for K = 32 with the folded sums, both
    conv3x3_dgrad_bnsums (dx entry by entry, both BatchNorm-backward sums), both narrow weight gradients with the deferred input
    (x_bn: against fp64 of relu(y * scale + shift) (x) dy; 512 splits through wgrad_fold_kernel, the tile reduce for K = 32, the
    tap-packed kernel and the generic reduce for K = 8), bn_bwd_first_wgrad with sums (dw, dgamma, dbeta).  The narrow dgrad /
    wgrad launches are then repeated under the opt-in two-product arithmetic (`two_products`) with the headline bars.
    Observed on MI355X (worst of B = 32 / 64 / 7 / 8): dy 1.1e-7, dgamma 6.2e-8, dbeta 2.0e-7, dx 5.7e-7, BatchNorm-backward
    sums 1.8e-7, dw (K = 8) 3.0e-6 at B = 64, dw (K = 32) 1.4e-6, first-block dw 8.0e-8; bars about 5x that, within the 2e-5 /
    5e-5 of the per-op convolution tests.  Two products: dx 3.1e-4, dw 1.3e-4 per entry, L2 <= 2.2e-4.  One dropped chunk
    moves: a wgrad split >= 3.0e-3, a BatchNorm-sums row >= 3.8e-3, a K = 8 reduce chunk >= 1.5e-5, an 8-row chunk of the
    first-block weight gradient >= 2.9e-3."""
    rec = Recorder(monkeypatch)
    net, im, feat, gt, calls = train_step(rec, B)
    assert rec.route() == TRAIN_ROUTE
    e, d, e2 = check_backward(net, im, feat, calls, B, two_products=lambda: request.getfixturevalue("two_products"))
    print(f"B={B} LF backward: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items())
          + " | one chunk: " + "  ".join(f"{k} {v:.1e}" for k, v in d.items())
          + " | two products (entry, L2): " + "  ".join(f"{k} {a:.1e} {b:.1e}" for k, (a, b) in e2.items()))
    for k, v in e.items():
        assert v < BWD_BARS[k], (k, v, BWD_BARS[k])
    bar_of = {"bn reduce K=8": BWD_BARS["dgamma3"], "wgrad split K=8": BWD_BARS["dw3"], "wgrad split K=32": BWD_BARS["dw2"],
              "bn sums rows 3": BWD_BARS["sums3_dz"], "bn sums rows 2": BWD_BARS["sums2_dz"],
              "first wgrad 8-row chunk": BWD_BARS["dw1"]}
    for k, v in d.items():
        assert v >= 10 * bar_of[k], (k, v, bar_of[k])
    for k, (a, b) in e2.items():
        if k.startswith("sums"):
            assert a < BWD_BARS["sums2_dz"] * 10, (k, a)
        else:
            assert a < TWO_PRODUCT_BARS[0] and b < TWO_PRODUCT_BARS[1], (k, a, b)


# ------------------------------------------------------------------------------------------------ 6. edges
def assert_finite(calls):
    for c in calls:
        outs = c["out"] if isinstance(c["out"], tuple) else (c["out"],)
        for t in outs:
            if isinstance(t, torch.Tensor) and t.is_floating_point():
                assert bool(torch.isfinite(t).all()), f"{describe(c)}: non-finite output"
            mm = getattr(t, "_egz_minmax", None)
            if mm is not None:
                assert bool(torch.isfinite(mm).all()), f"{describe(c)}: non-finite min / max rows"


def test_lf_trailing_batch_poisoned(monkeypatch):
    """A trailing partial batch of 7 (LF._run ends every epoch with one): 5,488 narrow-wgrad patches at 11 per split leave
    splits 499-511 with no patch at all.  Every launch of the step runs with the hipops workspaces and freed allocator blocks
    poisoned with NaN, so any stat row, min / max row, partial tile or split a kernel forgets to write shows up.  Every output
    is finite and the whole chain meets the B = 32 bars."""
    B = 7
    assert narrow_wgrad_geometry(B)[2:] == (5488, 512, 11)
    rec = Recorder(monkeypatch, poison_each=True)
    net, im, feat, gt, calls = train_step(rec, B, seed=47)
    assert rec.route() == TRAIN_ROUTE
    assert_finite(calls)
    e, _ = check_forward(net, im, feat, calls, B, defects=False)
    eb, _, _ = check_backward(net, im, feat, calls, B, defects=False)
    print("B=7 poisoned: " + "  ".join(f"{k} {v:.1e}" for k, v in {**e, **eb}.items()))
    for k, v in e.items():
        assert v < FWD_BARS[k], (k, v)
    for k, v in eb.items():
        assert v < BWD_BARS[k], (k, v)


@pytest.mark.parametrize("mode", ["some", "all"])
def test_lf_relu_dead_block1_channels(mode, monkeypatch):
    """Block-1 channels that are entirely ReLU-dead (beta = -1e4): every fourth channel, or all of them.  The deferred path must
    treat a dead channel as zeros everywhere: its dgamma, dbeta and conv weight gradient are exactly 0, as is block 2's weight
    gradient from it.  With all channels dead the deferred bound is 0 (absmax scale 1, not a division by zero): block 2 outputs
    exactly its bias, its weight gradient is exactly 0, and nothing is NaN.  The rest of the step meets the B = 32 bars."""
    h = H()
    B = 8
    dead = torch.arange(32) % 4 == 2 if mode == "some" else torch.ones(32, dtype=torch.bool)
    rec = Recorder(monkeypatch)
    net, im, feat, gt, calls = train_step(rec, B, seed=53, dead=dead)
    assert rec.route() == TRAIN_ROUTE
    assert_finite(calls)
    am1 = float(h.absmax_value(calls[2]["out"][1]))
    dw2 = calls[16]["out"]
    dw1, dg1, db1 = calls[18]["out"]
    assert bool((dw2[:, dead.to(DEV)] == 0).all())
    assert bool((dw1[dead.to(DEV)] == 0).all()) and bool((dg1[dead.to(DEV)] == 0).all()) and bool((db1[dead.to(DEV)] == 0).all())
    if mode == "all":
        assert am1 == 0.0
        y2 = calls[3]["out"][0]
        assert torch.equal(y2, net.fusion[3].bias.detach().view(1, 1, 1, 32).expand_as(y2))
        assert bool((dw2 == 0).all()) and bool((dw1 == 0).all())
    else:
        assert am1 > 0
    e, _ = check_forward(net, im, feat, calls, B, defects=False)
    eb, _, _ = check_backward(net, im, feat, calls, B, defects=False)
    print(f"B=8 dead block-1 channels ({mode}): " + "  ".join(f"{k} {v:.1e}" for k, v in {**e, **eb}.items()))
    for k, v in e.items():
        assert v < FWD_BARS[k], (k, v)
    for k, v in eb.items():
        if mode == "all" and k in ("dw1", "dgamma1", "dbeta1", "dw2"):
            continue                                # (the reference is exactly 0 and so is the result: asserted above)
        assert v < BWD_BARS[k], (k, v)
