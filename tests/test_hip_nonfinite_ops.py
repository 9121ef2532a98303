"""Non-finite propagation, op by op: one operand of a hipops call carries a planted NaN / +inf / -inf, the outputs are compared
with the same op in torch fp64 on the CPU (tests/nonfinite_ref.py: the cases, the plants, the two rules).

  mask rule        NaN in the reference -> NaN on the device, +-inf -> non-finite, finite -> finite
  clean-twin rule  (NaN plants) where the fp64 reference is bit-identical with and without the plant, the device's poisoned
                   run equals its clean run bit for bit: a poison may not leak into its neighbours, a tile may not be skipped

The abs-max reductions that scale the f16 split ignore a NaN on purpose (fmaxf): the NaN element stays NaN through the split and
every other element keeps its scale, which is what the clean-twin rule checks on the split-half legs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import nonfinite_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def nhwc(t):   # (B,C,H,W) cpu -> (B,H,W,C) cuda contiguous
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):   # (B,H,W,C) cuda -> (B,C,H,W) cpu
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def _conv_out(y, stat, epi):
    out = {"y": nchw(y)}
    if epi == 2:
        out["stat"] = stat.sum(0).cpu()
    return out


def conv_f32(epi, ups=False):
    def run(h, o, mp):
        K = o["w"].shape[0]
        wp = h.packed_weight(o["w"].to(DEV), "ups_fwd" if ups == "phase" else "fwd")
        y, stat = h.conv3x3_fwd(nhwc(o["x"]), wp, o["b"].to(DEV), K, ups=ups, epi=epi)
        return _conv_out(y, stat, epi)
    return run


def conv_split(dtype, epi):
    def run(h, o, mp):
        K = o["w"].shape[0]
        y, stat = h.conv3x3_fwd(nhwc(o["x"]), h.packed_weight(o["w"].to(DEV), "fwd", dtype), o["b"].to(DEV), K, epi=epi, dtype=dtype)
        return _conv_out(y, stat, epi)
    return run


def conv_streamed(epi, splitk=False, ups=False, narrow=False):
    def run(h, o, mp):
        K, C = o["w"].shape[0], o["w"].shape[1]
        xd = nhwc(o["x"])
        B, Hh, Ww, _ = xd.shape
        mp.setattr(h, "SPLITK", splitk)
        if splitk:
            assert h.LIB.egz_conv3x3_streamed_splits(B, Hh, Ww, C, K) >= 2, "geometry expected to be split"
        wp, st = h.conv_weight(o["w"].to(DEV), "ups_fwd" if ups else "fwd", h.F16X3, xd, K)
        assert st, "geometry expected on the streamed kernel"
        y, stat = h.conv3x3_fwd(xd, wp, o["b"].to(DEV), K, ups="phase" if ups else False, epi=epi, dtype=h.F16X3, streamed=True)
        if narrow and epi == 2:      # the persistent narrow kernel writes one partial row per block (test_conv3x3_streamed)
            assert C <= 32 and K <= 32 and Hh % 16 == 0 and Ww % 16 == 0
            assert stat.shape[0] == h.LIB.egz_conv3x3_streamed_stat_rows(B, Hh, Ww, C, K) <= 256 and stat.shape[0] % 8 == 0
            assert stat.shape[0] != (B * Hh * Ww + 127) // 128
        return _conv_out(y, stat, epi)
    return run


def conv_padded_first(h, o, mp):
    xp = h.nchw_to_nhwc_pad(o["x"].to(DEV), 32)
    wd = torch.nn.Parameter(o["w"].to(DEV))
    y, stat = h.conv3x3_fwd(xp, h.packed_weight(wd, "fwd", 1), o["b"].to(DEV), 64, epi=2, dtype=1)
    return _conv_out(y, stat, 2)


def conv_first(h, o, mp):
    xd = o["x"].to(DEV)
    y, stat = h.conv_first_fwd(xd, o["w"].to(DEV), o["b"].to(DEV), True)
    dw = h.conv_first_wgrad(xd, nhwc(o["dy"]))
    return {"y": nchw(y), "stat": stat.sum(0).cpu(), "dw": dw.cpu()}


def bn_train(pool):
    def run(h, o, mp):
        yd = nhwc(o["y"])
        B, Hh, Ww, K = yd.shape
        rm, rv = o["rm"].to(DEV), o["rv"].to(DEV)
        coef = h.bn_finalize(h.channel_stats(yd), float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), rm, rv, 0.1, 1e-5)
        out = h.bn_relu_pool_fwd(yd, coef, pool)
        dy, dg, db = h.bn_relu_pool_bwd(yd, nhwc(o["dout_pool"] if pool else o["dout"]), coef, pool)
        return {"out": nchw(out), "dy": nchw(dy), "dgamma": dg.cpu(), "dbeta": db.cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu()}
    return run


def bn_eval(h, o, mp):
    ce = h.bn_eval_coeffs(o["gamma"].to(DEV), o["beta"].to(DEV), o["rm"].to(DEV), o["rv"].to(DEV), 1e-5)
    return {"out": nchw(h.bn_relu_pool_fwd(nhwc(o["y"]), ce, False))}


def presplit_chain(h, o, mp):
    """conv (statistics + per-channel max / min) -> bn_finalize(mm=...) -> bn_relu_pool_fwd(presplit) -> the consumer's forward
    and weight gradient on the stored pairs."""
    mp.setattr(h, "SPLITK", False)
    xd, w0 = nhwc(o["x"]), o["w"].to(DEV)
    B, Hh, Ww, _ = xd.shape
    C = K = 64
    wp0, st0 = h.conv_weight(w0, "fwd", h.F16X3, xd, C)
    assert st0
    y, stat = h.conv3x3_fwd(xd, wp0, o["b"].to(DEV), C, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True, want_bound=True)
    coef, am = h.bn_finalize(stat, float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), None, None, 0.1, 1e-5, mm=y._egz_mm)
    a = h.bn_relu_pool_fwd(y, coef, False, presplit_am=am)
    assert a._egz_presplit and h.presplit_ok(B, Hh, Ww, C, K)
    w1 = o["w2"].to(DEV)
    wp1, st1 = h.conv_weight(w1, "fwd", h.F16X3, a, K)
    assert st1
    y2, s2 = h.conv3x3_fwd(a, wp1, o["b2"].to(DEV), K, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True, pre_in=True)
    dw2 = h.conv3x3_wgrad(a, nhwc(o["dy2"]), precision="split_f16", x_pre=True)
    return {"y2": nchw(y2), "stat2": s2.sum(0).cpu(), "dw2": dw2.cpu()}


def conv_bn_prologue(h, o, mp):
    """The consumer normalises + ReLUs the pre-BatchNorm tensor while it stages it (forward and weight gradient, narrow kernels)."""
    y0 = nhwc(o["y0"])
    B, Hh, Ww, C = y0.shape
    K = o["w2"].shape[0]
    coef = h.bn_finalize(h.channel_stats(y0), float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), None, None, 0.1, 1e-5)
    y0._egz_absmax = h.absmax_of(h.bn_relu_pool_fwd(y0, coef, False))       # the operand carries the abs-max of the normalised values
    wp, st = h.conv_weight(o["w2"].to(DEV), "fwd", h.F16X3, y0, K)
    assert st
    y2, s2 = h.conv3x3_fwd(y0, wp, o["b2"].to(DEV), K, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True, bn_in=coef)
    dw2 = h.conv3x3_wgrad(y0, nhwc(o["dy2"]), precision="split_f16", x_bn=coef)
    return {"y2": nchw(y2), "stat2": s2.sum(0).cpu(), "dw2": dw2.cpu()}


def pairmax(h, o, mp):
    y2 = torch.cat((nhwc(o["a"]), nhwc(o["b"])), 0)
    B = o["a"].shape[0]
    z = h.pairmax_fwd(y2)
    dy2 = h.pairmax_bwd(y2, nhwc(o["dz"]))
    return {"z": nchw(z), "da": nchw(dy2[:B]), "db": nchw(dy2[B:])}


def relu_bwd(h, o, mp):
    out, g = nhwc(o["out"]), nhwc(o["g"])
    dyb, db = h.relu_bwd_bias(out, g)
    return {"dy": nchw(h.relu_bwd(out, g)), "dy_bias_form": nchw(dyb), "db": db.cpu()}


def upsample2x_bwd(h, o, mp):
    return {"dx": nchw(h.upsample2x_bwd(nhwc(o["g"])))}


def gemm_bias_relu(h, o, mp):
    return {"out": h.linear_fwd(o["x"].to(DEV), o["w"].to(DEV), bias=o["b"].to(DEV), relu=True).cpu()}


def head(h, o, mp):
    xd, w, b = nhwc(o["x"]), o["w"].to(DEV), o["b"].to(DEV)
    out, _ = h.conv1x1_sigmoid_fwd(xd, w, b)
    dd = o["dout"][:, 0].contiguous().to(DEV)
    dx, dw, db = h.conv1x1_sigmoid_bwd(xd, w, out, dd)
    none, dw2, db2 = h.conv1x1_sigmoid_bwd(xd, w, out, dd, need_dx=False)
    assert none is None
    return {"out": out.cpu(), "dx": nchw(dx), "dw": dw.cpu(), "db": db.cpu(), "dw_nodx": dw2.cpu(), "db_nodx": db2.cpu()}


def head_masked(h, o, mp):
    a, w, b = nhwc(o["x"]), o["w"].to(DEV), o["b"].to(DEV)
    out, _ = h.conv1x1_sigmoid_fwd(a, w, b)
    dx, dw, db, stat, _ = h.conv1x1_sigmoid_bwd_masked(a, w, out, o["dout"][:, 0].contiguous().to(DEV))
    assert stat.shape[0] == h.LIB.egz_conv1x1_sigmoid_bwd_rows(a.numel() // a.shape[-1], a.shape[-1])
    return {"dx": nchw(dx), "dbias": stat.sum(0).cpu(), "dw": dw.cpu(), "db": db.cpu()}


def floss(h, o, mp):
    inp, tgt = o["inp"].to(DEV), o["tgt"].to(DEV)
    loss, weights = h.floss_fwd(inp, tgt)
    return {"loss": loss.reshape(1).cpu(), "dinp": h.floss_bwd(inp, tgt, weights, None).cpu()}


def mse(tanh_t):
    def run(h, o, mp):
        a, b = o["a"].to(DEV), o["b"].to(DEV)
        loss, da = h.mse_fwd(a, b, tanh_t), h.mse_bwd(a, b, None, tanh_t)
        l1, d1 = h.mse_fwd_grad(a, b, tanh_t)                # the one-launch form of the AT sample step
        same = lambda p, q: torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p.nan_to_num(0.0), q.nan_to_num(0.0))
        assert same(loss, l1) and same(da, d1)
        return {"loss": loss.reshape(1).cpu(), "da": da.cpu()}
    return run


def floss_gout(h, o, mp):
    inp, tgt = o["inp"].to(DEV), o["tgt"].to(DEV)
    _, weights = h.floss_fwd(inp, tgt)
    return {"dinp": h.floss_bwd(inp, tgt, weights, o["gout"].to(DEV)).cpu()}


def mse_gout(h, o, mp):
    return {"da": h.mse_bwd(o["a"].to(DEV), o["b"].to(DEV), o["gout"].to(DEV), True).cpu()}


def first_block_bwd(h, o, mp):
    xd = o["x"].to(DEV)
    B, C, Hh, Ww = xd.shape
    assert h.bn_bwd_first_wgrad_ok(C, 32, False)
    y, stat = h.conv_first_fwd(xd, o["w"].to(DEV), None, True)
    coef = h.bn_finalize(stat, float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), None, None, 0.1, 1e-5)
    dw, dg, db = h.bn_bwd_first_wgrad(y, nhwc(o["dout"]), coef, xd)
    return {"dw": dw.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}


def deferred_chain(h, o, mp):
    xd = o["x"].to(DEV)
    B, C, Hh, Ww = xd.shape
    assert h.bn_defer_ok(B, Hh, Ww, 32, 32, True)
    y, stat = h.conv_first_fwd(xd, o["w"].to(DEV), o["b"].to(DEV), True, want_minmax=True)
    rm, rv = o["rm"].to(DEV), o["rv"].to(DEV)
    coef, am = h.bn_finalize_deferred(stat, y._egz_minmax, float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), rm, rv, 0.1, 1e-5)
    y._egz_absmax = am
    wp, st = h.conv_weight(o["w2"].to(DEV), "fwd", h.F16X3, y, 32)
    assert st
    y2, s2 = h.conv3x3_fwd(y, wp, o["b2"].to(DEV), 32, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=True, bn_in=coef)
    return {"y2": nchw(y2), "stat2": s2.sum(0).cpu(), "running_mean": rm.cpu(), "running_var": rv.cpu()}


def dgrad_bnsums(h, o, mp):
    mp.setattr(h, "SPLITK", False)
    dyd, y0 = nhwc(o["dy"]), nhwc(o["bn_y"])
    B, Hh, Ww, C = y0.shape
    K = dyd.shape[-1]
    assert h.bnsums_ok(B, Hh, Ww, C, K, h.F16X3)
    coef = h.bn_finalize(h.channel_stats(y0), float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), None, None, 0.1, 1e-5)
    wq, st = h.conv_weight(o["w"].to(DEV), "dgrad", h.F16X3, dyd, C)
    assert st
    dx, sums = h.conv3x3_dgrad_bnsums(dyd, wq, C, h.F16X3, y0, coef)
    dyb, dg, db = h.bn_relu_pool_bwd(y0, dx, coef, False, sums=sums)
    return {"dx": nchw(dx), "dyb": nchw(dyb), "dgamma": dg.cpu(), "dbeta": db.cpu()}


def presplit_grad_chain(h, o, mp):
    """conv (statistics + max / min) -> BatchNorm backward storing dy as pairs -> the conv's data gradient (pre_in) and weight
    gradient (dy_pre) on them."""
    mp.setattr(h, "SPLITK", False)
    xd, wd = nhwc(o["x"]), o["w"].to(DEV)
    B, Hh, Ww, C = xd.shape
    K = 64
    assert h.presplit_grad_ok(B, Hh, Ww, C, K)
    wp, st = h.conv_weight(wd, "fwd", h.F16X3, xd, K)
    y, stat = h.conv3x3_fwd(xd, wp, o["b"].to(DEV), K, epi=h.EPI_BIAS_STATS, dtype=h.F16X3, streamed=st, want_bound=True)
    coef = h.bn_finalize(stat, float(B * Hh * Ww), o["gamma"].to(DEV), o["beta"].to(DEV), None, None, 0.1, 1e-5)
    dout = nhwc(o["dout"])
    dy, dg, db = h.bn_relu_pool_bwd(y, dout, coef, False, presplit=(h.absmax_of(dout), y._egz_mm))
    assert dy._egz_presplit
    wq, sq = h.conv_weight(wd, "dgrad", h.F16X3, dy, C)
    dx = h.conv3x3_dgrad(dy, wq, C, dtype=h.F16X3, streamed=sq, pre_in=True)
    dw = h.conv3x3_wgrad(xd, dy, precision="split_f16", dy_pre=True)
    return {"dx": nchw(dx), "dw": dw.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}


def ups_dgrad_masked(h, o, mp):
    dyd, wd = nhwc(o["dy"]), o["w"].to(DEV)
    C = o["w"].shape[1]
    wq, st = h.conv_weight(wd, "ups_dgrad", h.F16X3, dyd, C)
    assert st
    dx, stat, _ = h.conv3x3_dgrad_masked(dyd, wq, C, h.F16X3, nhwc(o["a"]), True)
    return {"dx": nchw(dx), "dbias": stat[:, 0].sum(0).cpu()}


def tanh(h, o, mp):
    return {"y": h.tanh_fwd(o["x"].to(DEV)).cpu()}


def dgrad(kind):
    def run(h, o, mp):
        dyd, wd = nhwc(o["dy"]), o["w"].to(DEV)
        C = int(o["xshape"][1])
        if kind == "f32":
            dx = h.conv3x3_dgrad(dyd, h.packed_weight(wd, "dgrad"), C)
        elif kind == "f16":
            dx = h.conv3x3_dgrad(dyd, h.packed_weight(wd, "dgrad", 1), C, dtype=1)
        elif kind == "streamed":
            mp.setattr(h, "SPLITK", False)
            wq, st = h.conv_weight(wd, "dgrad", 1, dyd, C)
            assert st
            dx = h.conv3x3_dgrad(dyd, wq, C, dtype=1, streamed=True)
        elif kind == "ups_f32":
            dx = h.conv3x3_ups_dgrad(dyd, h.packed_weight(wd, "ups_dgrad"), C)
            two = h.upsample2x_bwd(h.conv3x3_dgrad(dyd, h.packed_weight(wd, "dgrad"), C))      # the two-launch form
            assert torch.equal(torch.isfinite(dx), torch.isfinite(two))
        else:
            wq, st = h.conv_weight(wd, "ups_dgrad", 1, dyd, C)
            assert st
            dx = h.conv3x3_ups_dgrad(dyd, wq, C, dtype=1, streamed=True)
        return {"dx": nchw(dx)}
    return run


def dgrad_masked(h, o, mp):
    dyd, wd = nhwc(o["dy"]), o["w"].to(DEV)
    C = o["w"].shape[1]
    wq, st = h.conv_weight(wd, "dgrad", h.F16X3, dyd, C)
    assert st
    dx, stat, _ = h.conv3x3_dgrad_masked(dyd, wq, C, h.F16X3, nhwc(o["a"]), False)
    return {"dx": nchw(dx), "dbias": stat[:, 0].sum(0).cpu()}


def wgrad(prec, narrow=False):
    def run(h, o, mp):
        B, C, Hh, Ww = o["x"].shape
        assert bool(h.LIB.egz_conv3x3_wgrad_narrow_ok(B, Hh, Ww, C, o["dy"].shape[1])) == narrow
        return {"dw": h.conv3x3_wgrad(nhwc(o["x"]), nhwc(o["dy"]), precision=prec).cpu()}
    return run


def lstm_cell(h, o, mp):
    gates, c_prev = o["gates"].to(DEV), o["c_prev"].to(DEV)
    hh, c, act = torch.empty_like(c_prev), torch.empty_like(c_prev), torch.empty_like(gates)
    h.lstm_cell_fwd(gates, c_prev, hh, c, act)
    return {"h": hh.cpu(), "c": c.cpu(), "act": act.cpu()}


def lstm(L, persist, fused=False):
    def run(h, o, mp):
        import egaze_amd.models.LSTMnet as M
        mp.setattr(h, "LSTM_PERSIST", persist)
        mp.setattr(M, "B1_FUSED", fused)
        T, B, _ = o["x"].shape
        if persist:
            assert h.lstm_persist_ok(L, B, 512)
        net = M.lstmnet(num_layer=L).to(DEV)
        with torch.no_grad():
            for l in range(L):
                for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
                    name = ("weight" if k[0] == "w" else "bias") + k[1:] + f"_l{l}"
                    getattr(net.lstm, name).copy_(o[f"{k}{l}"])
            net.lin.weight.copy_(o["lin_w"])
            net.lin.bias.copy_(o["lin_b"])
        xd, hd, cd = (o[k].to(DEV).requires_grad_(not fused) for k in ("x", "h0", "c0"))
        out, (hn, cn) = net(xd, (hd, cd))
        assert type(out.grad_fn).__name__.startswith("_LSTMNetB1Fn" if fused else "_LSTMNetFn")
        ((out * o["wo"].to(DEV)).sum() + (hn * o["wh"].to(DEV)).sum() + (cn * o["wc"].to(DEV)).sum()).backward()
        assert h.lstm_persist_status() == 0
        res = {"pred": out.detach().cpu(), "hn": hn.detach().cpu(), "cn": cn.detach().cpu()}
        if not fused:
            res.update(dx=xd.grad.cpu(), dh0=hd.grad.cpu(), dc0=cd.grad.cpu())
        for name, p in net.lstm.named_parameters():
            res["d_" + name] = p.grad.cpu()
        return res
    return run


RUN = {
    **{f"conv_f32_epi{e}": conv_f32(e) for e in (0, 1, 2)},
    **{f"conv_{t}_epi{e}": conv_split(d, e) for t, d in (("f16", 1), ("bf16", 2)) for e in (0, 1, 2)},
    **{f"conv_streamed_epi{e}": conv_streamed(e) for e in (0, 1, 2)},
    **{f"conv_streamed_narrow_epi{e}": conv_streamed(e, narrow=True) for e in (0, 1, 2)},
    **{f"conv_splitk_epi{e}": conv_streamed(e, splitk=True) for e in (0, 1, 2)},
    **{f"conv_ups_{m}_epi{e}": conv_f32(e, ups=m) for m in ("fold", "phase") for e in (1, 2)},
    **{f"conv_ups_streamed_epi{e}": conv_streamed(e, ups=True) for e in (0, 1)},
    "conv_padded_first": conv_padded_first, "conv_first_c3": conv_first, "conv_first_c20": conv_first,
    **{f"bn_k{K}_pool{int(p)}": bn_train(p) for K in (64, 8) for p in (False, True)},
    "bn_eval": bn_eval, "presplit_chain": presplit_chain, "conv_bn_prologue": conv_bn_prologue, "conv_bn_prologue_k8": conv_bn_prologue,
    "first_block_bwd_c2": first_block_bwd, "first_block_bwd_c3": first_block_bwd, "deferred_chain": deferred_chain,
    "dgrad_bnsums_wide": dgrad_bnsums, "dgrad_bnsums_narrow": dgrad_bnsums, "presplit_grad_chain": presplit_grad_chain,
    "ups_dgrad_masked": ups_dgrad_masked, "floss_gout": floss_gout, "mse_gout": mse_gout, "pairmax": pairmax,
    "relu_bwd": relu_bwd, "upsample2x_bwd": upsample2x_bwd, "gemm_bias_relu": gemm_bias_relu, "head_c8": head, "head_c64": head,
    "head_masked_c8": head_masked, "floss": floss, "mse_tanh0": mse(False), "mse_tanh1": mse(True), "tanh": tanh,
    "dgrad_f32": dgrad("f32"), "dgrad_f16": dgrad("f16"), "dgrad_streamed": dgrad("streamed"), "ups_dgrad_f32": dgrad("ups_f32"),
    "ups_dgrad_streamed": dgrad("ups_streamed"), "dgrad_masked": dgrad_masked,
    "wgrad_split": wgrad("split_f16"), "wgrad_narrow": wgrad("split_f16", narrow=True), "wgrad_f32": wgrad("f32"),
    "lstm_cell": lstm_cell, "lstm_wave_l1": lstm(1, False), "lstm_wave_l2": lstm(2, False), "lstm_persist_t1b1": lstm(2, True),
    "lstm_persist_t3b16": lstm(2, True), "lstm_b1": lstm(2, False, fused=True),
}
_DEV_CLEAN = {}


def _to_dev_float(o):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in o.items()}


@pytest.mark.parametrize("name,op,where,kind", R.case_ids(), ids=["-".join((n, o, w[1], k)) for n, o, w, k in R.case_ids()])
def test_nonfinite_propagation(name, op, where, kind, monkeypatch):
    import egaze_amd.hipops as h
    case = R.CASES_BY_NAME[name]
    ref_clean = case.clean_ref()
    if name not in _DEV_CLEAN:
        _DEV_CLEAN[name] = RUN[name](h, _to_dev_float(case.operands()), monkeypatch)
    dev_clean = _DEV_CLEAN[name]
    ops = R.poisoned_operands(case, op, where, kind)
    ref = case.run_ref(ops)
    dev = RUN[name](h, _to_dev_float(ops), monkeypatch)
    assert set(dev) <= set(ref) and dev, (set(dev), set(ref))
    problems = []
    for k in sorted(dev):
        r = ref[k].reshape(dev[k].shape) if ref[k].numel() == dev[k].numel() else ref[k]
        ok, msg = R.masks_agree(dev[k], r)
        n_bad = int((~torch.isfinite(r)).sum())
        print(f"{name}/{op}/{where[1]}/{kind}: {k}: {n_bad} of {r.numel()} reference elements non-finite, "
              f"{int((~torch.isfinite(dev[k])).sum())} on the device")
        if not ok:
            problems.append(f"{k}: mask rule: {msg}")
        assert torch.isfinite(dev_clean[k]).all(), f"{k}: the clean run is not finite"
        if kind == "nan":
            ok, msg = R.clean_twin(dev[k], dev_clean[k], r, ref_clean[k].reshape(dev[k].shape), tol=case.tol)
            if not ok:
                problems.append(f"{k}: clean-twin rule: {msg}")
    assert not problems, "\n".join(problems)
