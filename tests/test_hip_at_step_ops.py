"""The AT step (lstmnet, T = 16, L = 2, H = 512) launch by launch, and Adam / zero fill / copy at the flat-buffer sizes, against
torch-CPU float64.

test_hip_at.py compares the recurrence with fp64 only at toy (T, B), the persistent kernels only with the wavefront kernels of
the same build, and the real geometry only with the fp32 oracle at 2e-5 / 2e-4 -- 30x to 300x the distance of fp32 arithmetic
from fp64 there.  test_hip_ops.py runs Adam on 4099 elements: the grid-stride loop of the capped grid (8192 blocks = 8,388,608
elements per trip; the SP model's flat buffer takes five to six) never executes under a test that looks at elements.

Part 1 runs ONE real step (lstmnet + MSELoss through the autograd node, gradients into FusedAdam's sinks) per recurrence form
with every hipops call recorded, and checks each launch against fp64 computed from the fp32 operands THAT launch read.  Errors
are max |got - ref| / max |ref| per tensor.  No bar is taken from a kernel's output: for every tensor the same operation is
also run in fp32 on the CPU (torch ops) from the same operands, its distance d_cpu32 from fp64 is measured at run time, and
the bar is FACTOR x d_cpu32 (4 unless raised in FACTORS with a measured reason); exactly-rounded launches must be equal.
Every reduction / recurrence bar must also see the smallest realistic defect, computed in fp64 from the same data
(defect >= 10 x bar): a K-slice of one wave dropped for one batch tile at one step, a stale h / dgates hand-off for one tile,
an 8-row tile missing from a bias gradient, a K-tile missing from a weight-gradient product, a block's 256 elements missing
from the loss.

Part 2 checks every element of an Adam step against fp64 with a per-element bar of half an fp32 ulp + 2 x the distance of
torch.optim.Adam (fp32, CPU, same inputs) at the element's own scale (adam_errors), counts the unchanged elements, and guards
both ends of every buffer."""
import gc
import math
import os

import pytest
import torch

from oracle import egaze_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, HD, L = 16, 512, 2
# csrc/lstm_seq.hip: reduction indices one wave owns (the unit a lost partial sum would take with it) and batch rows per block
WAVE_FWD_KSLICE, WAVE_FWD_TILE = HD // 4, 16          # lstm_wave_fwd_kernel: kw = H / 4 per wave; its tile is 16 x MT rows, the
                                                      # 16 of one MFMA row group are used here (a smaller or equal defect)
PERSIST_FWD_KSLICE, PERSIST_FWD_TILE = 64, 16         # lstm_persist_fwd_kernel: k = 64 wave + ..., b0 = tile * 16
WAVE_BWD_KSLICE, WAVE_BWD_TILE = 4 * HD // 8, 16      # lstm_wave_bwd_kernel: kw = K / 8 per wave of K = 4H, b0 = blockIdx.y * 16
PERSIST_BWD_KSLICE, PERSIST_BWD_TILE = 256, 8         # lstm_persist_bwd_kernel: k = 256 wave + ..., r0 = tile * 8
BIAS_TILE = 8                                         # rows of one step one block folds into a bias gradient
GEMM_KTILES = (32, 64)                                # csrc/gemm_lstm.hip: GK (generic tiles) and FK (fast-path slab depth)
MSE_BLOCK = 256                                       # csrc/head_loss.hip: mse_fwd_kernel, elements per block and trip
ADAM_TRIP = 8192 * 256 * 4                            # csrc/adam.hip: capped grid x block x float4
AT_FLAT = sum((math.prod(s) + 3) // 4 * 4 for s in O.lstm_shapes().values())
BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
SENTINEL = 12345.0
GUARD = 64

# Bars of Part 1 are factor x d_cpu32 with factor 4, except (figures: profiles/at_step_ops_errors.txt, MI355X):
# * dh_in = dgates_l0 (T*B, 2048) @ W_ih_l0, the one product of the step with K = 2048: every MFMA accumulator adds 2048 terms
#   in one serial fp32 chain, the CPU's blocked GEMM does not.  Over the six cases and both forms: error 1.32e-6 - 2.40e-6,
#   d_cpu32 3.43e-7 - 4.50e-7, i.e. 3.36 - 5.33 x; one missing K-tile is a defect of 5.4e-2 or more.  Factor 8.
# * the weight-gradient products at B = 64, whose reduction over T * B rows is 1024 long: d W_ih / d W_hh 2.38 - 6.01 x (error
#   4.58e-7 - 1.52e-6, d_cpu32 1.54e-7 - 3.45e-7), d lin.weight 5.00 x (1.12e-6 / 2.24e-7) and the same gradient in the
#   whole-step comparison 4.38 x (1.10e-6 / 2.51e-7); a missing K-tile is 3.1e-3 or more (asserted >= 10 bars for each,
#   the whole-step ones included).  Factor 8 for these names when T * B >= 1024.
# Everything else stays at 4: the K = 512 products reach 3.40 x, the LSTM weight gradients of the whole step at B = 64 3.83 x,
# the step's input gradient 3.06 x, every recurrence tensor 2.09 x, the bias gradients 0.89 x.
FACTORS = {"dh_in": 8}
LONG_K_FACTORS = {"d W_": 8, "d lin.weight": 8, "e2e lin.weight": 8}


def H():
    import egaze_amd.hipops as h
    return h


@pytest.fixture(autouse=True)
def cpu_threads():
    """fp64 references on at most 16 host threads; each case's tensors are freed before the next one."""
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


def d64(x):
    return None if x is None else x.double()


# =============================================================================================== Part 1: the AT step
class Table:
    """Measured error, yardstick, bar and defect of every checked tensor of one case; asserted after it has been printed."""

    def __init__(self, tag, long_k=False):
        self.tag, self.rows, self.bad, self.long_k = tag, [], [], long_k

    def factor(self, name):
        if self.long_k:
            for prefix, f in LONG_K_FACTORS.items():
                if name.startswith(prefix):
                    return f
        return FACTORS.get(name, 4)

    def check(self, name, got, ref, cpu32, defect=None, extra_bar=0.0, key=None, cpu_ref=None):
        err, dc = rel(got, ref), rel(cpu32, ref if cpu_ref is None else cpu_ref)
        bar = self.factor(key or name) * dc + extra_bar
        self.rows.append(f"{name} {err:.2e}/{dc:.2e}" + ("" if defect is None else f"/{defect:.1e}"))
        if not err <= bar:
            self.bad.append(f"{name}: error {err:.3e} above the bar {bar:.3e} (d_cpu32 {dc:.3e})")
        if defect is not None and not defect >= 10 * bar:
            self.bad.append(f"{name}: the smallest defect {defect:.3e} is below 10 bars ({bar:.3e})")
        return bar

    def exact(self, name, got, ref):
        ok = torch.equal(got, ref)
        self.rows.append(f"{name} {'exact' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append(f"{name}: not bit-identical ({(got != ref).sum().item()} entries differ)")


RECORDED = ("tanh_fwd", "tanh_bwd", "add", "linear_fwd", "lstm_wave_fwd", "lstm_persist_fwd", "mse_fwd", "mse_bwd", "relu_bwd",
            "matmul_tn", "colsum", "matmul_nn", "transpose2d", "lstm_wave_bwd", "lstm_persist_bwd", "matmul_tn_batched",
            "copy_into")


def snap(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, (list, tuple)):
        return type(x)(snap(v) for v in x)
    if isinstance(x, dict):
        return {k: snap(v) for k, v in x.items()}
    return x


def record(h, monkeypatch):
    """Wrap the hipops calls of the step: every call's operands and results, copied to the host right after the launch."""
    rec = {n: [] for n in RECORDED}
    for name in RECORDED:
        orig = getattr(h, name)

        def wrapped(*a, _orig=orig, _name=name, **kw):
            out = _orig(*a, **kw)
            rec[_name].append({"a": snap(a), "kw": snap(kw), "out": snap(out)})
            return out
        monkeypatch.setattr(h, name, wrapped)
    return rec


def cell(pre, c_prev):
    i, f, g, o = pre.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat((i, f, g, o), -1)


def lstm_ref(gxb, w_ih, w_hh, bias, h0, c0):
    """The stacked recurrence written out (gate order i, f, g, o as torch.nn.LSTM) in the dtype of its operands.  gxb (T,B,4H):
    layer 0's input projection with both biases; w_ih / bias: per layer, entry 0 unused."""
    Tn, B, _ = gxb.shape
    Ln, Hd = len(w_hh), h0.shape[-1]
    hs, cs = gxb.new_zeros(Ln, Tn + 1, B, Hd), gxb.new_zeros(Ln, Tn, B, Hd)
    acts, pre = gxb.new_zeros(Ln, Tn, B, 4 * Hd), gxb.new_zeros(Ln, Tn, B, 4 * Hd)
    for l in range(Ln):
        hs[l, 0] = h0[l]
        c = c0[l]
        base = gxb if l == 0 else hs[l - 1, 1:] @ w_ih[l].t() + bias[l]
        for t in range(Tn):
            pre[l, t] = base[t] + hs[l, t] @ w_hh[l].t()
            hs[l, t + 1], c, acts[l, t] = cell(pre[l, t], c)
            cs[l, t] = c
    return {"hs": hs, "cs": cs, "acts": acts, "pre": pre, "hn": hs[:, Tn].clone(), "cn": cs[:, Tn - 1].clone()}


def cell_bwd(a, c, c_prev, dh, dc_in):
    i, f, g, o = a.chunk(4, -1)
    tc = torch.tanh(c)
    dc = dc_in + dh * o * (1 - tc * tc)
    dg = torch.cat((dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), -1)
    return dg, dc * f


def bptt_ref(dh_top, dhn, dcn, acts, cs, c0, w_hh, w_ih):
    """Backward through time from the saved activations, in the dtype of its operands -> dgates, dh0, dc0 (+ the dh and dc that
    entered every cell, for the defect sizes)."""
    Ln, Tn, B, Hd = cs.shape
    dg = cs.new_zeros(Ln, Tn, B, 4 * Hd)
    dh0, dc0 = cs.new_zeros(Ln, B, Hd), cs.new_zeros(Ln, B, Hd)
    dh_in, dc_in = cs.new_zeros(Ln, Tn, B, Hd), cs.new_zeros(Ln, Tn, B, Hd)
    for l in reversed(range(Ln)):
        dh_rec = cs.new_zeros(B, Hd) if dhn is None else dhn[l]
        dc = cs.new_zeros(B, Hd) if dcn is None else dcn[l]
        for t in reversed(range(Tn)):
            up = dh_top[t] if l == Ln - 1 else dg[l + 1, t] @ w_ih[l + 1]
            dh_in[l, t], dc_in[l, t] = up + dh_rec, dc
            dg[l, t], dc = cell_bwd(acts[l, t], cs[l, t], cs[l, t - 1] if t else c0[l], dh_in[l, t], dc)
            dh_rec = dg[l, t] @ w_hh[l]
        dh0[l], dc0[l] = dh_rec, dc
    return {"dgates": dg, "dh0": dh0, "dc0": dc0, "dh_in": dh_in, "dc_in": dc_in}


def tiles(B, tile):
    return [slice(0, min(tile, B)), slice((B - 1) // tile * tile, B)]


def fwd_defects(ref, w_hh, c0, kslice, tile):
    """fp64: per layer, the smallest change of h_t (over max |hs| of the layer) when (a) one wave's K-slice of h_{t-1} W_hh^T is
    lost, (b) h_{t-2} is read in place of h_{t-1}, for one batch tile at one step."""
    Ln, Tn1, B, Hd = ref["hs"].shape
    out = []
    for l in range(Ln):
        scale = ref["hs"][l].abs().max().item()
        dk, dst = [], []
        for t in (1, (Tn1 - 1) // 2, Tn1 - 2):
            c_prev = ref["cs"][l, t - 1]
            for R in tiles(B, tile):
                h_prev, h_stale, h_t = ref["hs"][l, t, R], ref["hs"][l, t - 1, R], ref["hs"][l, t + 1, R]
                for k0 in (0, Hd - kslice):
                    lost = h_prev[:, k0:k0 + kslice] @ w_hh[l][:, k0:k0 + kslice].t()
                    dk.append((cell(ref["pre"][l, t, R] - lost, c_prev[R])[0] - h_t).abs().max().item() / scale)
                stale = (h_prev - h_stale) @ w_hh[l].t()
                dst.append((cell(ref["pre"][l, t, R] - stale, c_prev[R])[0] - h_t).abs().max().item() / scale)
        out.append((min(dk), min(dst)))
    return out


def bwd_defects(ref, acts, cs, c0, w_hh, kslice, tile):
    """fp64: per layer, the smallest change of dgates_t (over max |dgates| of the layer) when (a) one wave's K-slice of
    dgates_{t+1} W_hh is lost, (b) dgates_{t+2} is read in place of dgates_{t+1}, for one batch tile at one step; and (c) the
    smallest change of the bias gradient when one BIAS_TILE-row tile of one step is missing from it."""
    Ln, Tn, B, Hd = cs.shape
    out = []
    for l in range(Ln):
        dg = ref["dgates"][l]
        scale = dg.abs().max().item()
        dk, dst, dbias = [], [], []
        for t in (0, Tn // 2, Tn - 3):
            for R in tiles(B, tile):
                def redo(dh_lost):
                    got = cell_bwd(acts[l, t, R], cs[l, t, R], (cs[l, t - 1] if t else c0[l])[R],
                                   ref["dh_in"][l, t, R] - dh_lost, ref["dc_in"][l, t, R])[0]
                    return (got - dg[t, R]).abs().max().item() / scale
                for k0 in (0, 4 * Hd - kslice):
                    dk.append(redo(dg[t + 1, R][:, k0:k0 + kslice] @ w_hh[l][k0:k0 + kslice]))
                dst.append(redo((dg[t + 1, R] - dg[t + 2, R]) @ w_hh[l]))
        db_scale = dg.sum((0, 1)).abs().max().item()
        for t in (0, Tn // 2, Tn - 1):
            for R in tiles(B, BIAS_TILE):
                dbias.append(dg[t, R].sum(0).abs().max().item() / db_scale)
        out.append((min(dk), min(dst), min(dbias)))
    return out


def ktile_defect(a, b, ref, relu_of=None):
    """fp64: the smallest change of a^T b (over max |ref|) when one K-tile of the reduction over the rows is missing.
    relu_of: the complete pre-activation when the launch applies a ReLU to the product."""
    n, scale, out = a.shape[0], ref.abs().max().item(), []
    for unit in GEMM_KTILES:
        for s in {0, (n // 2) // unit * unit, (n - unit) // unit * unit}:
            lost = a[s:s + unit].t() @ b[s:s + unit]
            if relu_of is not None:
                lost = torch.relu(relu_of) - torch.relu(relu_of - lost)
            out.append(lost.abs().max().item() / scale)
    return min(out)


def rowtile_defect(x, rows, ref):
    """fp64: the smallest change of the column sums of x (over max |ref|) when ``rows`` consecutive rows are missing."""
    n = x.shape[0]
    return min(x[s:s + rows].sum(0).abs().max().item() for s in (0, n // 2, n - rows)) / ref.abs().max().item()


def at_inputs(B, seed):
    """bench.py's AT leg (synthetic.at_batch: |randn| / 2 features and targets) with NON-zero h0, c0.  Drawn on the host, so
    that the fp32 CPU yardstick of a seed can be examined without a GPU."""
    g = torch.Generator().manual_seed(seed)
    atb = {"input": (torch.randn(T, B, HD, generator=g).abs() * 0.5).to(DEV), "gt": (torch.randn(T, B, HD, generator=g).abs() * 0.5).to(DEV)}
    g = torch.Generator().manual_seed(seed + 1)
    h0, c0 = torch.randn(L, B, HD, generator=g) * 0.3, torch.randn(L, B, HD, generator=g) * 0.3
    wh, wc = torch.randn(L, B, HD, generator=g), torch.randn(L, B, HD, generator=g)
    return atb["input"], atb["gt"], h0.to(DEV), c0.to(DEV), wh.to(DEV), wc.to(DEV)


def run_step(h, rec, net, opt, inp, tgt, h0, c0, wh, wc, through_state, persist):
    from egaze_amd.functions import MSELoss
    for v in rec.values():
        v.clear()
    opt.zero_grad()
    x, h0r, c0r = (t.clone().requires_grad_(True) for t in (inp, h0, c0))
    with h.lstm_persistent(persist):
        out, (hn, cn) = net(x, (h0r, c0r))
        assert type(out.grad_fn).__name__.startswith("_LSTMNetFn")
        loss = MSELoss.apply(out, tgt, True)
        total = loss + (hn * wh).sum() * 1e-3 + (cn * wc).sum() * 1e-3 if through_state else loss
        total.backward()
    torch.cuda.synchronize()
    res = {"out": out, "hn": hn, "cn": cn, "loss": loss, "d input": x.grad, "d h0": h0r.grad, "d c0": c0r.grad}
    res.update({k: p.grad for k, p in net.named_parameters()})
    return {k: v.detach().cpu().clone() for k, v in res.items()}, {k: list(v) for k, v in rec.items()}


def check_launches(tb, form, rec, B, h=None):
    """Every launch of one recorded step against fp64 from that launch's own fp32 operands.  Returns the K-tile defects of the
    weight-gradient products, which the whole-step comparison of the same gradients has to see as well."""
    e2e_defects = {}
    persist = form == "persist"
    r = rec["tanh_fwd"][0]
    tb.check("tanh_fwd", r["out"], torch.tanh(d64(r["a"][0])), torch.tanh(r["a"][0]))
    # input projection of all steps: no bias on the persistent route, b_ih + b_hh (egz_add, exactly rounded) on the wavefront route
    r = rec["linear_fwd"][0]
    bias = r["kw"].get("bias")
    assert (bias is None) == persist and tuple(r["out"].shape) == (T * B, 4 * HD)
    x2d, w = r["a"]
    refm = d64(x2d) @ d64(w).t() + (0 if bias is None else d64(bias))
    tb.check("gx0", r["out"], refm, torch.nn.functional.linear(x2d, w, bias), defect=ktile_defect(d64(x2d).t(), d64(w).t(), refm))
    for i, ra in enumerate(rec["add"]):
        tb.exact(f"bsum{i}", ra["out"], ra["a"][0] + ra["a"][1])
    assert len(rec["add"]) == (0 if persist else L)

    # the recurrence, fed the kernel's own gx0
    (r,) = rec["lstm_persist_fwd" if persist else "lstm_wave_fwd"]
    assert not rec["lstm_wave_fwd" if persist else "lstm_persist_fwd"]
    if persist:
        gx0, w_ih, w_hh, b_ih, b_hh, h0, c0 = r["a"]
        ops = lambda cv: (cv(gx0) + cv(b_ih[0]) + cv(b_hh[0]), [None] + [cv(t) for t in w_ih[1:]], [cv(t) for t in w_hh],  # noqa: E731
                          [None] + [cv(b_ih[l]) + cv(b_hh[l]) for l in range(1, L)], cv(h0), cv(c0))
    else:
        gx0, w_ih, w_hh, bsum, h0, c0 = r["a"]
        ops = lambda cv: (cv(gx0), [None] + [cv(t) for t in w_ih[1:]], [cv(t) for t in w_hh],  # noqa: E731
                          [None] + [cv(t) for t in bsum[1:]], cv(h0), cv(c0))
    ref, c32 = lstm_ref(*ops(d64)), lstm_ref(*ops(lambda t: t))
    hs, cs, acts, hn, cn = r["out"]
    w_hh64 = [d64(t) for t in w_hh]
    dfw = fwd_defects(ref, w_hh64, d64(c0), PERSIST_FWD_KSLICE if persist else WAVE_FWD_KSLICE,
                      PERSIST_FWD_TILE if persist else WAVE_FWD_TILE)
    tb.exact("hs slot 0", hs[:, 0], h0)
    for l in range(L):
        bar = tb.check(f"hs{l}", hs[l], ref["hs"][l], c32["hs"][l], defect=min(dfw[l]))
        tb.rows.append(f"[hs{l} defects: K-slice {dfw[l][0]:.1e} stale {dfw[l][1]:.1e} bar {bar:.1e}]")
        tb.check(f"cs{l}", cs[l], ref["cs"][l], c32["cs"][l])
        tb.check(f"acts{l}", acts[l], ref["acts"][l], c32["acts"][l])
    tb.check("hn", hn, ref["hn"], c32["hn"])
    tb.check("cn", cn, ref["cn"], c32["cn"])

    r = rec["linear_fwd"][1]
    x2d, w = r["a"]
    assert r["kw"].get("relu") is True
    pre = d64(x2d) @ d64(w).t() + d64(r["kw"]["bias"])
    tb.check("lin+relu", r["out"], torch.relu(pre), torch.relu(torch.nn.functional.linear(x2d, w, r["kw"]["bias"])),
             defect=ktile_defect(d64(x2d).t(), d64(w).t(), torch.relu(pre), relu_of=pre))

    # loss: n = T * B * 512 (B = 32: exactly LOSS_BLOCKS blocks, B = 64: the second grid-stride trip)
    (r,) = rec["mse_fwd"]
    a, b, tanh_target = r["a"]
    assert tanh_target is True and a.numel() == T * B * HD
    sq = (d64(a) - torch.tanh(d64(b))).flatten() ** 2
    n = sq.numel()
    d_blk = min(sq[s:s + MSE_BLOCK].sum().item() for s in (0, (n // 2) // MSE_BLOCK * MSE_BLOCK, n - MSE_BLOCK)) / sq.sum().item()
    # (a scalar: d_cpu32 can be 0 by chance, so the rounding of the fp32 result itself, half an ulp, is part of the bar)
    tb.check("mse_fwd", r["out"], sq.mean(), ((a - torch.tanh(b)) ** 2).mean(), defect=d_blk, extra_bar=2.0 ** -24)
    (r,) = rec["mse_bwd"]
    a, b, gout, _ = r["a"]
    tb.check("mse_bwd", r["out"], d64(gout) * 2.0 / n * (d64(a) - torch.tanh(d64(b))), gout * 2.0 / n * (a - torch.tanh(b)))

    (r,) = rec["relu_bwd"]
    o, dout = r["a"]
    tb.exact("relu_bwd", r["out"], torch.where(o > 0, dout, torch.zeros_like(dout)))
    (r,) = rec["matmul_tn"]
    a, b = r["a"]
    refm = d64(a).t() @ d64(b)
    e2e_defects["e2e lin.weight"] = ktile_defect(d64(a), d64(b), refm)
    tb.check("d lin.weight", r["out"], refm, a.t() @ b, defect=e2e_defects["e2e lin.weight"])
    r = rec["colsum"][0]
    own = d64(r["a"][0])
    tb.check("d lin.bias", r["out"], own.sum(0), r["a"][0].sum(0), defect=rowtile_defect(own, min(BIAS_TILE, B), own.sum(0)))
    r = rec["matmul_nn"][0]
    a, w = r["a"]
    refm = d64(a) @ d64(w)
    tb.check("dh_top", r["out"], refm, a @ w, defect=ktile_defect(d64(a).t(), d64(w), refm))

    # backward through time from the kernel's saved acts, cs, c0
    (r,) = rec["lstm_persist_bwd" if persist else "lstm_wave_bwd"]
    assert not rec["lstm_wave_bwd" if persist else "lstm_persist_bwd"]
    if persist:
        dh_top, dhn, dcn, acts, cs, c0, w_hh, w_ih, db = r["a"]
        assert len(db) == 2 * L and all(t is not None for t in db)
        w_ih = [None] + list(w_ih[1:])
    else:
        dh_top, dhn, dcn, acts, cs, c0, w_hh_t, w_ih_t = r["a"]
        w_hh, w_ih = [t.t() for t in w_hh_t], [None] + [t.t() for t in w_ih_t[1:]]
        for rt in rec["transpose2d"]:
            tb.exact("transpose2d", rt["out"], rt["a"][0].t().contiguous())
    args = (dh_top.view(T, B, HD), dhn, dcn, acts, cs, c0)
    ref = bptt_ref(*[d64(t) for t in args], [d64(t) for t in w_hh], [d64(t) for t in w_ih])
    c32 = bptt_ref(*args, w_hh, w_ih)
    dgates, dh0, dc0 = r["out"]
    dbw = bwd_defects(ref, d64(acts), d64(cs), d64(c0), [d64(t) for t in w_hh], PERSIST_BWD_KSLICE if persist else WAVE_BWD_KSLICE,
                      PERSIST_BWD_TILE if persist else WAVE_BWD_TILE)
    for l in range(L):
        bar = tb.check(f"dgates{l}", dgates[l], ref["dgates"][l], c32["dgates"][l], defect=min(dbw[l][:2]))
        tb.rows.append(f"[dgates{l} defects: K-slice {dbw[l][0]:.1e} stale {dbw[l][1]:.1e} bar {bar:.1e}]")
    tb.check("dh0", dh0, ref["dh0"], c32["dh0"])
    tb.check("dc0", dc0, ref["dc0"], c32["dc0"])
    if persist:
        # the bias gradients come out of the same launch (every sink its own fold)
        for i, t in enumerate(db):
            l = i // 2
            tb.check(f"db{i} (l{l})", t, ref["dgates"][l].sum((0, 1)), c32["dgates"][l].sum((0, 1)), defect=dbw[l][2], key=f"db l{l}")
        assert len(rec["colsum"]) == 1 and not rec["copy_into"]
        if h is not None:
            # the same launch once more with the sink of b_hh_l0 withheld (db[1] = None): the fold of that sink is skipped, the
            # other three must be complete, the withheld slot of the shared buffer untouched, dgates / dh0 / dc0 the same bits
            dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
            sinks = torch.full((2 * L, 4 * HD), SENTINEL, dtype=torch.float32, device=DEV)
            dbn = [sinks[0], None, sinks[2], sinks[3]]
            dg2, dh02, dc02 = h.lstm_persist_bwd(dv(dh_top), dv(dhn), dv(dcn), dv(acts), dv(cs), dv(c0), [dv(t) for t in w_hh],
                                                 [dv(t) for t in w_ih], dbn)
            torch.cuda.synchronize()
            for i in (0, 2, 3):
                l = i // 2
                tb.check(f"db{i} (l{l}) [db1 None]", sinks[i].cpu(), ref["dgates"][l].sum((0, 1)), c32["dgates"][l].sum((0, 1)),
                         defect=dbw[l][2], key=f"db l{l}")
            tb.exact("withheld sink", sinks[1].cpu(), torch.full((4 * HD,), SENTINEL))
            tb.exact("dgates [db1 None]", dg2.cpu(), dgates)
            tb.exact("dh0 dc0 [db1 None]", torch.stack((dh02, dc02)).cpu(), torch.stack((dh0, dc0)))
    else:
        # colsum of the kernel's own dgates, then a copy for the second bias of the layer
        assert len(rec["colsum"]) == 1 + L and len(rec["copy_into"]) == L
        for l in range(L):
            rc = rec["colsum"][1 + l]
            own = d64(rc["a"][0])
            d_tile = rowtile_defect(own, min(BIAS_TILE, B), own.sum(0))
            tb.check(f"db colsum l{l}", rc["out"], own.sum(0), rc["a"][0].sum(0), defect=d_tile, key=f"db l{l}")
            tb.exact(f"db copy l{l}", rec["copy_into"][l]["a"][0], rec["copy_into"][l]["a"][1])

    # weight gradients: K = T * B reductions into the optimizer's sinks, one batched launch
    (r,) = rec["matmul_tn_batched"]
    a_list, b_list = r["a"][0], r["a"][1]
    assert len(a_list) == 2 * L
    for i, name in enumerate(("d W_ih0", "d W_hh0", "d W_ih1", "d W_hh1")):
        refm = d64(a_list[i]).t() @ d64(b_list[i])
        e2e_defects["e2e lstm.weight_" + name[4:6] + "_l" + name[6]] = ktile_defect(d64(a_list[i]), d64(b_list[i]), refm)
        tb.check(name, r["out"][i], refm, a_list[i].t() @ b_list[i], defect=e2e_defects["e2e lstm.weight_" + name[4:6] + "_l" + name[6]])
    r = rec["matmul_nn"][1]
    a, w = r["a"]
    refm = d64(a) @ d64(w)
    tb.check("dh_in", r["out"], refm, a @ w, defect=ktile_defect(d64(a).t(), d64(w), refm))
    (r,) = rec["tanh_bwd"]
    y, dy = r["a"][0].flatten(), r["a"][1].flatten()
    tb.check("tanh_bwd", r["out"].flatten(), d64(dy) * (1 - d64(y) ** 2), dy * (1 - y * y))
    return e2e_defects


def torch_step(sd, inp, tgt, h0, c0, wh, wc, through_state, dtype, mask_from=None):
    """The whole step with torch.nn.LSTM + Linear on the CPU in ``dtype``.  mask_from = (near, kernel_out): the ReLU mask of the
    outputs flagged in ``near`` is the kernel's own."""
    lstm, lin = torch.nn.LSTM(HD, HD, L).to(dtype), torch.nn.Linear(HD, HD).to(dtype)
    lstm.load_state_dict({k[5:]: v.to(dtype) for k, v in sd.items() if k.startswith("lstm.")})
    lin.load_state_dict({k[4:]: v.to(dtype) for k, v in sd.items() if k.startswith("lin.")})
    x, h0r, c0r = (t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (inp, h0, c0))
    y, (hn, cn) = lstm(torch.tanh(x), (h0r, c0r))
    pre = lin(y)
    mask = pre.detach() > 0
    if mask_from is not None:
        mask = torch.where(mask_from[0], mask_from[1] > 0, mask)
    out = pre * mask
    loss = ((out - torch.tanh(tgt.cpu().to(dtype))) ** 2).mean()
    total = loss + ((hn * wh.cpu().to(dtype)).sum() + (cn * wc.cpu().to(dtype)).sum()) * 1e-3 if through_state else loss
    total.backward()
    res = {"out": out, "hn": hn, "cn": cn, "loss": loss, "d input": x.grad, "d h0": h0r.grad, "d c0": c0r.grad, "pre": pre,
           "y": y}
    res.update({"lstm." + k: p.grad for k, p in lstm.named_parameters()})
    res.update({"lin." + k: p.grad for k, p in lin.named_parameters()})
    return {k: v.detach() for k, v in res.items()}


def check_whole_step(tb, got, r64, r32, rerun64, defects):
    """out, hn, cn, loss and every gradient of the step against torch fp64.  Outputs whose fp64 pre-activation is within the
    forward bar of zero may have the other ReLU sign in fp32: there (at most 8 of T*B*512) the reference takes the kernel's mask.
    The CPU fp32 yardstick itself must need no such help: its ReLU mask equals the fp64 one, and d_cpu32 is its distance from the
    plain fp64 run."""
    assert torch.equal(r32["pre"] > 0, r64["pre"] > 0), "the CPU fp32 path flips a ReLU sign: choose another seed"
    plain = r64
    bar_out = tb.factor("e2e out") * rel(r32["out"], r64["out"])
    near = r64["pre"].abs() <= bar_out * r64["out"].abs().max()
    n_near = int(near.sum())
    tb.rows.append(f"[outputs within the forward bar of 0: {n_near}]")
    assert n_near <= 8, f"{n_near} outputs within {bar_out:.1e} of the ReLU's kink"
    if n_near:
        r64 = rerun64((near, got["out"]))
    for k in got:
        extra = 2.0 ** -24 if k == "loss" else 0.0
        tb.check(f"e2e {k}", got[k], r64[k], r32[k], extra_bar=extra, cpu_ref=plain[k], defect=defects.get(f"e2e {k}"))


@pytest.mark.parametrize("B,through_state", [(32, False), (32, True), (64, False), (64, True), (7, False), (7, True)])
def test_at_step_every_launch_against_fp64(B, through_state, monkeypatch):
    """One SP-bench-shaped AT step (T = 16, L = 2, H = 512; B = 32 headline, 64 wavefront only, 7 ragged tiles; non-zero h0 / c0;
    ``through_state``: gradients also enter through the returned (hn, cn)), on the wavefront launches and on the persistent
    launches from the same operands.  Per form: every launch against fp64 of its own operands (check_launches), then the whole
    step against torch.nn.LSTM + Linear in fp64.  Bars: 4 x d_cpu32 measured at run time (module docstring), equality for
    relu_bwd / slot 0 / copies / transposes / bias sums; defect >= 10 bars for every recurrence tensor, weight-gradient product,
    bias gradient and the loss.  The fp64 reference recurrence is cross-checked against torch.nn.LSTM(...).double() (< 1e-12).
    Seeds 200 + B: on the CPU the fp32 path alone flips NO ReLU sign against fp64 in any of the six cases (asserted), and one of
    the T*B*512 fp64 pre-activations lies within the forward bar of the kink in each (at most 8 allowed).  Those outputs are not
    dropped from the comparison: the fp64 run is repeated with the kernel's own ReLU mask at exactly those positions, so that
    every gradient entry is still compared; d_cpu32 stays the CPU fp32 run's distance from the plain fp64 run."""
    h = H()
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.optim import FusedAdam
    sd = synth.synth_state_dict(O.lstm_shapes(), seed=2)
    net = lstmnet()
    net.load_state_dict(sd)
    net.to(DEV).train()
    opt = FusedAdam(net.parameters(), lr=1e-4)
    assert opt.numel == AT_FLAT
    inp, tgt, h0, c0, wh, wc = at_inputs(B, seed=200 + B)
    rec = record(h, monkeypatch)

    forms = ["wave"]
    ok = h.lstm_persist_ok(L, B, HD)
    if B > 32:
        assert not ok, "lstm_persist_ok must refuse B > 32"
    elif ok:
        forms.append("persist")
    runs = {f: run_step(h, rec, net, opt, inp, tgt, h0, c0, wh, wc, through_state, f == "persist") for f in forms}
    assert h.lstm_persist_status() == 0
    h.lstm_persist_check()

    r64 = torch_step(sd, inp, tgt, h0, c0, wh, wc, through_state, torch.float64)
    r32 = torch_step(sd, inp, tgt, h0, c0, wh, wc, through_state, torch.float32)
    # the written-out fp64 recurrence against torch.nn.LSTM in fp64, from the same tanh'd input
    x64 = torch.tanh(inp.cpu().double())
    s64 = {k: v.double() for k, v in sd.items()}
    mine = lstm_ref(x64 @ s64["lstm.weight_ih_l0"].t() + s64["lstm.bias_ih_l0"] + s64["lstm.bias_hh_l0"],
                    [None, s64["lstm.weight_ih_l1"]], [s64["lstm.weight_hh_l0"], s64["lstm.weight_hh_l1"]],
                    [None, s64["lstm.bias_ih_l1"] + s64["lstm.bias_hh_l1"]], h0.cpu().double(), c0.cpu().double())
    assert rel(mine["hs"][L - 1, 1:], r64["y"]) < 1e-12 and rel(mine["hn"], r64["hn"]) < 1e-12 and rel(mine["cn"], r64["cn"]) < 1e-12

    tables = []
    for f in forms:
        res, recs = runs[f]
        tb = Table(f"AT step B={B} T={T} state-grads={int(through_state)} {f}", long_k=T * B >= 1024)
        defects = check_launches(tb, f, recs, B, h)
        check_whole_step(tb, res, r64, r32,
                         lambda m: torch_step(sd, inp, tgt, h0, c0, wh, wc, through_state, torch.float64, mask_from=m), defects)
        tables.append(tb)
    for tb in tables:
        print(f"\n{tb.tag} [error/d_cpu32(/defect)]: " + "  ".join(tb.rows))
    bad = [f"{tb.tag}: {b}" for tb in tables for b in tb.bad]
    assert not bad, "\n".join(bad)
    if B <= 32 and not ok:
        pytest.skip("wavefront half passed; the persistent LSTM launches are unavailable on this device (lstm_persist_ok refused "
                    "B <= 32 for a reason other than the batch size)")


# =============================================================================================== Part 2: Adam, zero fill, copy
_SP_NUMEL = []


def sp_numel():
    """The real SP flat size: FusedAdam(model_SP().parameters()).numel (about 46.5 M, five to six grid-stride trips)."""
    if not _SP_NUMEL:
        from egaze_amd.models.model_SP import model_SP
        from egaze_amd.optim import FusedAdam
        from egaze_amd.utils import make_layers, cfg
        model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20)).to(DEV)
        _SP_NUMEL.append(FusedAdam(model.parameters()).numel)
        del model
        gc.collect()
        torch.cuda.empty_cache()
    return _SP_NUMEL[0]


SIZES = [1, 3, 4, 5, 4099, AT_FLAT, ADAM_TRIP - 4, ADAM_TRIP, ADAM_TRIP + 4, ADAM_TRIP + 4099, "sp"]


def size_of(n):
    return sp_numel() if n == "sp" else n


def guarded(n, fill=None):
    """n floats with GUARD sentinel floats on either side (the interior stays 16-byte aligned) -> (whole buffer, interior view)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def adam_state(n, seed, zero_every=7):
    """p with |p| in [0.25, 1]; g over six decades of magnitude, either sign; m, v as after earlier steps (m = g x +-[0.5, 1.5],
    v = g^2 x [0.5, 1.5], so |m'| / sqrt(v') stays O(1) and no update can round away); every ``zero_every``-th element has
    g = m = v = 0: its update must be exactly 0."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen, device=DEV)  # noqa: E731
    sign = lambda: torch.where(r() < 0.5, -1.0, 1.0)  # noqa: E731
    p = (0.25 + 0.75 * r()) * sign()
    g = torch.pow(10.0, -6.0 * r()) * sign()
    m = g * (0.5 + r()) * sign()
    v = g * g * (0.5 + r())
    zero = torch.arange(n, device=DEV) % zero_every == 3
    g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    return p, g, m, v, zero


def adam_ref64(p, g, m, v, step, lr=LR):
    """adam.hip's header formulas in fp64 from the fp32 state, with the fp64 bias corrections the host forms -> (update, m, v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m = m + (1.0 - BETA1) * (g - m)
    v = v * BETA2 + (1.0 - BETA2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - BETA2 ** step) + EPS
    return -(lr / (1.0 - BETA1 ** step)) * (m / denom), m, v


def adam_cpu32(p, g, m, v, step, lr=LR):
    """torch.optim.Adam (single-tensor, fp32, CPU) from the same state -> (p, m, v)."""
    P = torch.nn.Parameter(p.clone())
    P.grad = g.clone()
    opt = torch.optim.Adam([P], lr=lr, betas=(BETA1, BETA2), eps=EPS, foreach=False)
    opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return P.detach(), opt.state[P]["exp_avg"], opt.state[P]["exp_avg_sq"]


def half_ulp(x):
    """Half an fp32 ulp at the magnitude of every element of x (fp64 in, fp64 out)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x).exponent - 25)


def one_step_scales(g, m0, ref):
    """The magnitude each new moment is formed at: the sum of the magnitudes of its terms (0.9 |m| + 0.1 |g| >= |m'|; v' itself,
    whose terms are all positive)."""
    return BETA1 * m0.double().abs() + (1.0 - BETA1) * g.double().abs(), ref[2]


def adam_errors(p0, p1, m1, v1, ref, cpu, scales, nsteps=1, pop=None):
    """Worst |got - ref| / bar over the elements of the update, m and v, and the yardsticks for the report.
    update: bar = nsteps half-ulps of the fp32 p + 2 x d_cpu32, d_cpu32 the largest distance of the CPU fp32 step from fp64 (p
    has ONE magnitude, [0.25, 1], and the error of the update is the rounding of p: an absolute yardstick fits every element).
    m, v: the state spans six (v: twelve) decades, so the yardstick scales with the element: bar_i = nsteps half-ulps of the
    fp32 result + 2 x r_cpu32 x S_i, S_i the element's own scale (one_step_scales), r_cpu32 = max_i |cpu_i - ref_i| / S_i.
    pop = {name: yardstick}: taken over a population that has this state as its head, where this state is too small for a
    maximum to mean anything."""
    upd_ref, m_ref, v_ref = ref
    out = {}
    rows = (("update", p1.double() - p0.double(), upd_ref, cpu[0].double() - p0.double(), p1.double(), None),
            ("m", m1.double(), m_ref, cpu[1].double(), m_ref, scales[0]), ("v", v1.double(), v_ref, cpu[2].double(), v_ref, scales[1]))
    for name, got, want, cpu_got, at, S in rows:
        if S is None:
            S = torch.ones_like(want)
        live = S > 0
        y = ((cpu_got - want).abs()[live] / S[live]).max().item() if bool(live.any()) else 0.0
        if pop is not None:
            y = pop[name]
        bar = nsteps * half_ulp(at) + 2 * y * S
        worst_rel = ((got - want).abs()[live] / S[live]).max().item() if bool(live.any()) else 0.0
        out[name] = (((got - want).abs() / bar).max().item(), worst_rel, y)
    return out


def adam_yardsticks(p0, g, m0, v0, step):
    """The yardsticks of adam_errors over a whole population (the CPU fp32 step against fp64)."""
    ref, cpu = adam_ref64(p0, g, m0, v0, step), adam_cpu32(p0, g, m0, v0, step)
    e = adam_errors(p0, cpu[0], cpu[1], cpu[2], ref, cpu, one_step_scales(g, m0, ref))
    return {k: v[2] for k, v in e.items()}


def adam_launch(h, dev_form, p, g, m, v, step, grad_scale=1.0, flag=None, lr=LR):
    if dev_form:
        cnt = torch.tensor([step - 1, 0], dtype=torch.int32, device=DEV)
        h.adam_step_dev(p, g, m, v, lr, BETA1, BETA2, EPS, cnt, grad_scale, nonfinite=flag)
        assert cnt.tolist() == [step, 0]
    else:
        h.adam_step(p, g, m, v, lr, BETA1, BETA2, EPS, step, grad_scale, nonfinite=flag)


def report(tag, errs):
    print(f"\n{tag} [worst error in bars | worst error over the element's scale | the CPU fp32 step's]: "
          + "  ".join(f"{k} {a:.2f}|{b:.1e}|{c:.1e}" for k, (a, b, c) in errs.items()))


@pytest.mark.parametrize("dev_form", [False, True], ids=["host-counter", "device-counter"])
@pytest.mark.parametrize("size", SIZES, ids=[str(s) for s in SIZES])
def test_adam_one_step_every_element_against_fp64(size, dev_form):
    """Step 4 from a given state at today's regression sizes, the AT flat size, around the first grid-stride boundary (8192 blocks
    x 256 lanes x float4), a scalar tail behind a multi-trip body and the real SP flat size.  Update, m and v of EVERY element
    against fp64 within half an ulp + 2 x the CPU fp32 step's own distance (adam_errors: scaled with the element for m and v); an element skipped or updated twice is off by ~lr = 1e-3, 10^4 bars.  The
    elements with p unchanged are exactly the zero-gradient ones (a skipped trip cannot hide in a max), their m and v stay 0, the
    64 floats on either side of p, m, v (and g) are untouched, no non-finite flag; grad_scale = 0.125 equals the step on the
    pre-scaled gradient bit for bit."""
    h = H()
    n = size_of(size)
    # (below 4099 elements the state is the head of the 4099-element one and the yardsticks -- relative to each element's own
    # scale for m and v -- are the maxima over all 4099: the maximum over 1 - 5 samples says nothing about an operation's
    # rounding.  At n = 5 the CPU's m happened to sit 1.1e-8 from fp64 and the kernel's three correctly rounded operations,
    # 5.7e-8, missed a bar built on that by a factor 1.11)
    npop = max(n, 4099)
    p0, g, m0, v0, zero = adam_state(npop, seed=900 + npop % 1000)
    pop = None
    if npop > n:
        pop = adam_yardsticks(*[t.cpu() for t in (p0, g, m0, v0)], 4)
        p0, g, m0, v0, zero = (t[:n].clone() for t in (p0, g, m0, v0, zero))
    bufs = [guarded(n, t) for t in (p0, g, m0, v0)]
    (pb, p), (gb, gd), (mb, m), (vb, v) = bufs
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    adam_launch(h, dev_form, p, gd, m, v, 4, flag=flag)
    torch.cuda.synchronize()
    assert all(guards_intact(b, n) for b, _ in bufs), "a launch wrote outside [0, n)"
    assert torch.equal(gd, g) and int(flag.item()) == 0
    p1, m1, v1 = p.cpu(), m.cpu(), v.cpu()
    p0c, gc_, m0c, v0c, zc = p0.cpu(), g.cpu(), m0.cpu(), v0.cpu(), zero.cpu()
    ref = adam_ref64(p0c, gc_, m0c, v0c, 4)
    errs = adam_errors(p0c, p1, m1, v1, ref, adam_cpu32(p0c, gc_, m0c, v0c, 4), one_step_scales(gc_, m0c, ref), pop=pop)
    unchanged = p1 == p0c
    predicted = (p0c.double() + ref[0]).float() == p0c
    report(f"adam n={n} {'dev' if dev_form else 'host'}", errs)
    print(f"  unchanged elements {int(unchanged.sum())} (fp64 predicts {int(predicted.sum())}, zero-gradient {int(zc.sum())})")
    assert torch.equal(predicted, zc), "the test state must move every element with a gradient"
    assert torch.equal(unchanged, zc), f"{int((unchanged != zc).sum())} elements skipped or moved without a gradient"
    assert not m1[zc].any() and not v1[zc].any()
    for k, (worst, _, _) in errs.items():
        assert worst <= 1.0, (k, errs[k])
    del ref, errs

    # grad_scale: (8 g) x 0.125 is exact, so the scaled launch must reproduce the bits
    (pb2, p2), (gb2, g2), (mb2, m2), (vb2, v2) = [guarded(n, t) for t in (p0, g * 8.0, m0, v0)]
    adam_launch(h, dev_form, p2, g2, m2, v2, 4, grad_scale=0.125)
    torch.cuda.synchronize()
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)
    assert all(guards_intact(b, n) for b in (pb2, gb2, mb2, vb2))


def test_adam_slices_across_the_grid_stride_boundary():
    """hipops.adam_step on [lo, hi) slices (multiples of 4; the middle one crosses element 8,388,608 and the last one ends in a
    scalar tail): after the middle slice alone everything outside it is untouched and everything inside equals the full-buffer
    step bit for bit; after all three the buffers equal the full step."""
    h = H()
    n = ADAM_TRIP + 4099
    p0, g, m0, v0, _ = adam_state(n, seed=77)
    full = [t.clone() for t in (p0, m0, v0)]
    h.adam_step(full[0], g, full[1], full[2], LR, BETA1, BETA2, EPS, 3)
    (pb, p), (mb, m), (vb, v) = [guarded(n, t) for t in (p0, m0, v0)]
    cuts = [0, 4096, ADAM_TRIP + 1024, n]
    lo, hi = cuts[1], cuts[2]
    h.adam_step(p, g, m, v, LR, BETA1, BETA2, EPS, 3, lo=lo, hi=hi)
    for got, want, before in zip((p, m, v), full, (p0, m0, v0)):
        assert torch.equal(got[lo:hi], want[lo:hi])
        assert torch.equal(got[:lo], before[:lo]) and torch.equal(got[hi:], before[hi:])
    h.adam_step(p, g, m, v, LR, BETA1, BETA2, EPS, 3, lo=cuts[0], hi=cuts[1])
    h.adam_step(p, g, m, v, LR, BETA1, BETA2, EPS, 3, lo=cuts[2], hi=cuts[3])
    for got, want in zip((p, m, v), full):
        assert torch.equal(got, want)
    assert all(guards_intact(b, n) for b in (pb, mb, vb))


def test_adam_eight_steps_at_the_sp_size_both_counter_forms():
    """Eight steps with a fresh gradient each at the real SP flat size from zero moments: the host-counter and the device-counter
    form are bit-identical on p, m, v after EVERY step (what the graphed-step tests rely on), the device counter reads 8, and the
    end state is within 8 half-ulps + 2 x the distance of the 8-step CPU run (torch.optim.Adam, fp32; adam_errors) of an fp64 run,
    element by element."""
    h = H()
    n = sp_numel()
    gen = torch.Generator(device=DEV).manual_seed(5)
    p0 = (0.25 + 0.75 * torch.rand(n, generator=gen, device=DEV)) * torch.where(torch.rand(n, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    p0c = p0.cpu()
    del p0
    p64, m64, v64 = p0c.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    s_m = torch.zeros(n, dtype=torch.float64)           # the scale m is formed at: the same recursion over |g| (no cancellation)
    P = torch.nn.Parameter(p0c.clone())
    opt = torch.optim.Adam([P], lr=LR, betas=(BETA1, BETA2), eps=EPS, foreach=False)
    for step in range(1, 9):
        g = torch.randn(n, generator=gen, device=DEV) * 10.0 ** (-(step % 4))
        h.adam_step(pa, g, ma, va, LR, BETA1, BETA2, EPS, step)
        h.adam_step_dev(pb, g, mb, vb, LR, BETA1, BETA2, EPS, cnt)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), f"the two counter forms part at step {step}"
        gc_ = g.cpu()
        del g
        g64 = gc_.double()
        m64 = m64 + (1.0 - BETA1) * (g64 - m64)
        s_m = BETA1 * s_m + (1.0 - BETA1) * g64.abs()
        v64 = v64 * BETA2 + (1.0 - BETA2) * g64 * g64
        p64 = p64 - (LR / (1.0 - BETA1 ** step)) * (m64 / (v64.sqrt() / math.sqrt(1.0 - BETA2 ** step) + EPS))
        P.grad = gc_
        opt.step()
    assert cnt.tolist() == [8, 0]
    st = opt.state[P]
    errs = adam_errors(p0c, pa.cpu(), ma.cpu(), va.cpu(), (p64 - p0c.double(), m64, v64), (P.detach(), st["exp_avg"], st["exp_avg_sq"]),
                       (s_m, v64), nsteps=8)
    report(f"adam 8 steps n={n} host == dev bit for bit", errs)
    for k, (worst, _, _) in errs.items():
        assert worst <= 1.0, (k, errs[k])


@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
def test_adam_step_counts(step):
    """Bias corrections at step counts 1 ... 100000 (host: the count as an argument; device: preset in the counter), each against
    fp64 at the AT flat size.  The two forms must be bit-identical up to 64 steps (the graphed-step tests compare them with
    torch.equal); beyond that the device pow() against the host pow() is only recorded."""
    h = H()
    n = AT_FLAT
    p0, g, m0, v0, _ = adam_state(n, seed=300 + step % 97)
    host = [t.clone() for t in (p0, m0, v0)]
    dev = [t.clone() for t in (p0, m0, v0)]
    adam_launch(h, False, host[0], g, host[1], host[2], step)
    adam_launch(h, True, dev[0], g, dev[1], dev[2], step)
    same = all(torch.equal(a, b) for a, b in zip(host, dev))
    p0c, gc_, m0c, v0c = p0.cpu(), g.cpu(), m0.cpu(), v0.cpu()
    ref, cpu = adam_ref64(p0c, gc_, m0c, v0c, step), adam_cpu32(p0c, gc_, m0c, v0c, step)
    for tag, st in (("host", host), ("dev", dev)):
        errs = adam_errors(p0c, st[0].cpu(), st[1].cpu(), st[2].cpu(), ref, cpu, one_step_scales(gc_, m0c, ref))
        report(f"adam step count {step} {tag} (host == dev bit for bit: {same})", errs)
        for k, (worst, _, _) in errs.items():
            assert worst <= 1.0, (tag, k, errs[k])
    if step <= 64:
        assert same


@pytest.mark.parametrize("dev_form", [False, True], ids=["host-counter", "device-counter"])
def test_adam_skips_nonfinite_gradients_at_the_sp_size(dev_form):
    """NaN / inf planted in the first grid-stride trip, in a later trip, in the last vector element and in the scalar tail (the SP
    flat size is a multiple of 4, so this buffer is 3 elements longer): those elements keep p, m, v, the flag is raised, and every
    other element has exactly the bits of the clean step."""
    h = H()
    n = sp_numel() + 3
    p0, g, m0, v0, _ = adam_state(n, seed=41)
    spots = [5, 2 * ADAM_TRIP + 17, (n // 4) * 4 - 1, n - 1]
    bad = g.clone()
    bad[spots] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")], device=DEV)
    res = {}
    for tag, grad in (("clean", g), ("bad", bad)):
        bufs = [guarded(n, t) for t in (p0, m0, v0)]
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        for step in (1, 2):
            adam_launch(h, dev_form, bufs[0][1], grad, bufs[1][1], bufs[2][1], step, flag=flag)
        assert all(guards_intact(b, n) for b, _ in bufs)
        res[tag] = ([v_ for _, v_ in bufs], int(flag.item()))
    assert res["clean"][1] == 0 and res["bad"][1] == 1
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[spots] = False
    for a, b in zip(res["clean"][0], res["bad"][0]):
        assert torch.equal(a[keep], b[keep])
    for got, before in zip(res["bad"][0], (p0, m0, v0)):
        assert torch.equal(got[spots], before[spots])
    assert torch.isfinite(res["bad"][0][0]).all()


@pytest.mark.parametrize("size", [ADAM_TRIP - 4, ADAM_TRIP, ADAM_TRIP + 4, "sp"], ids=["trip-4", "trip", "trip+4", "sp"])
def test_fill_zero_and_copy_into_at_the_flat_sizes(size):
    """zero_grad()'s fill and copy_into at the SP flat size and around the grid-stride boundary of their float4 kernels: every
    element, the 64 guard floats on either side; and the unaligned routes (the runtime's memset / memcpy) one element off."""
    h = H()
    n = size_of(size)
    gen = torch.Generator(device=DEV).manual_seed(n % 1000)
    src = torch.rand(n + 1, generator=gen, device=DEV) + 1.0
    for off, cnt in ((0, n), (1, n), (0, n + 1)) if size != "sp" else ((0, n),):
        buf = torch.full((cnt + off + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        view = buf[GUARD + off:GUARD + off + cnt]
        h.copy_into(view, src[:cnt])
        torch.cuda.synchronize()
        assert torch.equal(view, src[:cnt]), (off, cnt)
        assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + cnt:] == SENTINEL).all()), (off, cnt)
        h.fill_zero(view)
        torch.cuda.synchronize()
        assert not view.any(), (off, cnt)
        assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + cnt:] == SENTINEL).all()), (off, cnt)


def test_fused_adam_on_model_sp_every_parameter_view():
    """FusedAdam on a real model_SP: zero_grad() clears the whole flat gradient (filled with ones first); after one step() from a
    synthetic flat gradient every parameter VIEW holds the fp64-predicted value within the per-element bar, and the padding slots
    between parameters stay 0 in p, m and v."""
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import make_layers, cfg
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20)).to(DEV)
    opt = FusedAdam(model.parameters(), lr=LR)
    n = opt.numel
    assert n == sp_numel() and n > 5 * ADAM_TRIP
    opt.flat_g.fill_(1.0)
    opt.zero_grad()
    assert not opt.flat_g.any()
    pad = torch.ones(n, dtype=torch.bool, device=DEV)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
        assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * o and p.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * o
    # parameters away from 0 so that the update is thousands of ulps everywhere
    gen = torch.Generator(device=DEV).manual_seed(8)
    opt.flat_p.copy_((0.25 + 0.75 * torch.rand(n, generator=gen, device=DEV)) * (~pad))
    g = torch.randn(n, generator=gen, device=DEV) * 0.01 * (~pad)
    opt.flat_g.copy_(g)
    p0c, gc_ = opt.flat_p.cpu(), g.cpu()
    opt.step()
    opt.check_finite()
    torch.cuda.synchronize()
    z = torch.zeros(n)
    ref, cpu = adam_ref64(p0c, gc_, z, z, 1), adam_cpu32(p0c, gc_, z, z, 1)
    views = torch.cat([p.detach().reshape(-1) for p in opt.params]).cpu()
    real = (~pad).cpu()
    assert torch.equal(views, opt.flat_p.cpu()[real])
    errs = adam_errors(p0c, opt.flat_p.cpu(), opt.flat_m.cpu(), opt.flat_v.cpu(), ref, cpu, one_step_scales(gc_, z, ref))
    report(f"FusedAdam(model_SP) n={n}, {int(pad.sum())} padding slots", errs)
    for k, (worst, _, _) in errs.items():
        assert worst <= 1.0, (k, errs[k])
    moved = opt.flat_p.cpu() != p0c
    assert int((moved != (real & (gc_ != 0))).sum()) == 0
    for t in (opt.flat_p, opt.flat_m, opt.flat_v, opt.flat_g):
        assert not t[pad].any()
