"""The T = 1, B = 1 lstmnet step (csrc/lstm_b1.hip: layer forward, Linear + ReLU, rank-1 outer product with strip partials, cell
backward) directly on hipops.lstm_b1_fwd / lstm_b1_bwd against torch-CPU float64.

test_hip_at.py runs this path at (L, C, H, N) = (2, 512, 512, 512) only, one seed, small h0 / c0, whole-tensor bars of 1e-5 /
2e-5: the row / column / strip tails, the 16-way unrolled strip sum and its single tail, the k += 256 and j += 512 loops past
their first pass, null gradient entries, the ReLU mask and the "every gradient is written in full" invariant that AT.py and
optim.py rely on never execute under a test.

Reference: fp64 autograd of tanh(x) -> L LSTM layers (gate order i, f, g, o, torch semantics) -> Linear -> ReLU with the loss
(out . a) + (hn . wh) + (cn . wc), with both state terms, with neither (dhn = dcn = None) and with the cn term alone, from
the fp32 operands the kernels read.  Errors are max |got - ref| / max |ref| per tensor.  No bar is taken from a kernel's
output: the same step is run in fp32 on the CPU (torch ops) from the same operands, its distance d_cpu32 from fp64 is measured
at run time, and the bar is 4 x d_cpu32 (the project's allowance for another, equally valid fp32 summation order, as
test_hip_at_step_ops.py).  Every bar of a tensor behind a reduction must also see the smallest defect of that reduction,
computed in fp64 from the same data (defect >= 10 x bar): one 256-wide pass of a dot product lost (layer forward: of W_ih . x
or of W_hh . h; head: of lin.weight . h), or one 8-row strip lost from a transposed product W^T d (what outer_b1_kernel writes
per block and cell_bwd_b1_kernel sums).  What is exact by construction is compared bit for bit.  Figures:
profiles/b1_glue_tests.txt."""
import gc
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STRIP = 8            # csrc/lstm_b1.hip: rows of a weight matrix per outer_b1_kernel block
PASS = 256           # floats one trip of a dot-product loop covers (64 lanes x 4)
FACTOR = 4
KEEP_EVERY = 2       # saturated cases: every second hidden unit above layer 0 is kept out of saturation (make_case)
MODES = ("full", "out", "cn")       # loss terms through (hn, cn): both, none (dhn = dcn = None), cn only (dhn = None)
KINDS = ("w_ih", "w_hh", "b_ih", "b_hh")

# (L, C, H, N): the smallest shapes that reach each branch
SHAPES = [
    (2, 512, 512, 512),     # the product's own
    (1, 512, 512, 512),     # layer 0 is the top layer: the head's partials feed a layer whose own outer launch has part == null
    (3, 20, 36, 10),        # H % 32 != 0 and H < 256, C < H, N % 4 != 0 and N % 8 != 0 (lin_relu row tail, STRIP tail of 2 rows)
    (2, 1028, 516, 132),    # C > H (wide = C); k += 256: four passes + a 4-float tail; j += 512: a second pass with a tail;
                            # 4H / 8 = 258 strips: strip groups 0 and 1 take the tail add, 2 - 7 do not
    (2, 32, 32, 8), (2, 32, 32, 64), (2, 32, 32, 72), (2, 32, 32, 136),   # 1, 8, 9, 17 head strips: edges of the unrolled sum
]


def H():
    import egaze_amd.hipops as h
    return h


@pytest.fixture(autouse=True)
def cpu_threads():
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        torch.set_num_threads(keep)
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


def rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------- operands and references
def names(L):
    return [f"{k}_l{l}" for l in range(L) for k in KINDS] + ["lin.weight", "lin.bias"]


def make_case(L, C, Hd, N, seed, wscale=1.0):
    """Weights U(+-wscale / sqrt(H)) (nn.LSTM's init at wscale 1); h0 ~ 0.5 N(0,1) inside (-1, 1); c0 ~ 2 N(0,1) (tanh(c)
    saturates for some units); inp ~ 3 N(0,1).  Head rows i % 8 == 3 are dead: their bias is below -sum |w| (|h| < 1), so
    out == 0 whatever the rounding; row 5 (when there is one) has an all-zero weight row and zero bias: its pre-activation is
    exactly 0 and the row is masked, as torch's ReLU does.  Rows i % 8 == 0 have the bias +wscale (five standard deviations of
    w . h): every strip of eight head rows, the short last one included, carries gradient (asserted on the fp64 run).
    wscale > 1 (saturated gates): a strip of eight gate rows that are ALL saturated carries no gradient even in fp64, and its
    loss could not be seen.  So in the layers above layer 0 every second hidden unit is kept out of saturation: its four
    weight rows stay scaled (its share of W_ih_l^T dgates_l is as large as any), b_hh goes back to scale 1 and b_ih cancels
    the unit's w . x + w . h (fp64 forward pass of the layers below) up to a rest of magnitude 0.5 .. 1.  Every 8-row strip then
    holds four such rows (with one per strip the smallest of the 256 strips is 1.4e-05 of the gradient, below 10 bars; with
    four it is 1.1e-03 .. 7.2e-03 against 10 bars of 3.0e-04 .. 3.8e-04, computed on the host); the other units of those layers
    and all of layer 0 stay scaled and pass the saturation limit the case asserts."""
    g = torch.Generator().manual_seed(seed)
    bound = wscale / Hd ** 0.5

    def u(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) * bound
    params = []
    for l in range(L):
        params += [u(4 * Hd, C if l == 0 else Hd), u(4 * Hd, Hd), u(4 * Hd), u(4 * Hd)]
    lw, lb = u(N, Hd), u(N)
    dead = torch.arange(N) % 8 == 3
    lb[dead] = -(Hd * bound + 1.0)
    lb[torch.arange(N) % 8 == 0] = wscale
    if N > 5:
        lw[5], lb[5] = 0.0, 0.0
    params += [lw, lb]
    case = {"L": L, "C": C, "H": Hd, "N": N, "params": params, "dead": dead,
            "h0": (0.5 * torch.randn(L, Hd, generator=g)).clamp(-0.999, 0.999), "c0": 2.0 * torch.randn(L, Hd, generator=g),
            "inp": 3.0 * torch.randn(C, generator=g), "a": torch.randn(N, generator=g),
            "wh": torch.randn(L, Hd, generator=g), "wc": torch.randn(L, Hd, generator=g)}
    if wscale != 1.0:
        keep = (torch.arange(4 * Hd) % Hd) % KEEP_EVERY == 0
        x = torch.tanh(case["inp"].double())
        for l in range(L):
            w_ih, w_hh, b_ih, b_hh = params[4 * l:4 * l + 4]
            if l:
                dot = w_ih.double() @ x + w_hh.double() @ case["h0"][l].double()
                b_hh[keep] /= wscale
                rest = b_ih.double() / bound
                rest = torch.where(rest < 0, -1.0, 1.0) * (0.5 + 0.5 * rest.abs())
                b_ih[keep] = (rest - dot)[keep].float()
            pre = w_ih.double() @ x + b_ih.double() + w_hh.double() @ case["h0"][l].double() + b_hh.double()
            x = cell_fwd(pre, case["c0"][l].double())[0]
    return case


def cell_fwd(pre, c_prev):
    i, f, g, o = pre.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat((i, f, g, o), -1)


def cell_bwd(act, c, c_prev, dh, dcn):
    """lstm_b1.hip's header formulas; dh may carry a leading dimension (one row per lost strip)."""
    i, f, g, o = act.chunk(4, -1)
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + dcn
    return torch.cat((dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), -1)


def torch_step(case, dtype, mode):
    """The whole step with torch ops on the CPU in ``dtype`` (autograd backward) -> forward tensors and the 4L + 2 gradients."""
    L = case["L"]
    P = [p.to(dtype).clone().requires_grad_(True) for p in case["params"]]
    h0, c0 = case["h0"].to(dtype), case["c0"].to(dtype)
    x = xt = torch.tanh(case["inp"].to(dtype))
    acts, pres, hs, cs = [], [], [], []
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = P[4 * l:4 * l + 4]
        pre = torch.nn.functional.linear(x, w_ih, b_ih) + torch.nn.functional.linear(h0[l], w_hh, b_hh)
        x, c, act = cell_fwd(pre, c0[l])
        acts.append(act), pres.append(pre), hs.append(x), cs.append(c)
    prelin = torch.nn.functional.linear(x, P[-2], P[-1])
    out = torch.relu(prelin)
    hn, cn = torch.stack(hs), torch.stack(cs)
    loss = (out * case["a"].to(dtype)).sum()
    if mode == "full":
        loss = loss + (hn * case["wh"].to(dtype)).sum()
    if mode in ("full", "cn"):
        loss = loss + (cn * case["wc"].to(dtype)).sum()
    loss.backward()
    res = {"xt": xt, "acts": torch.stack(acts), "pre": torch.stack(pres), "hn": hn, "cn": cn, "out": out, "prelin": prelin}
    res = {k: v.detach() for k, v in res.items()}
    res["grads"] = [p.grad.detach() for p in P]
    return res


def passes(w, v):
    """The share of w @ v each 256-wide trip of the dot-product loop contributes (the last one may be narrower)."""
    return [w[:, k:k + PASS] @ v[k:k + PASS] for k in range(0, v.numel(), PASS)]


def strip_shares(w, d):
    """(number of strips, columns): the share of w^T d each STRIP-row block contributes (the last strip may be shorter)."""
    prod = w * d[:, None]
    pad = (-w.shape[0]) % STRIP
    if pad:
        prod = torch.cat((prod, prod.new_zeros(pad, w.shape[1])))
    return prod.view(-1, STRIP, w.shape[1]).sum(1)


def forward_defects(case, r64):
    """fp64: for every layer the smallest change of (acts, hn, cn), over the tensor's max, when one pass of W_ih . x or of
    W_hh . h is lost; for the head the smallest change of out when one pass of lin.weight . h_top is lost."""
    L = case["L"]
    P = [p.double() for p in case["params"]]
    h0, c0 = case["h0"].double(), case["c0"].double()
    out = {}
    for l in range(L):
        vin = r64["xt"] if l == 0 else r64["hn"][l - 1]
        worst = {"acts": [], "hn": [], "cn": []}
        for lost in passes(P[4 * l], vin) + passes(P[4 * l + 1], h0[l]):
            h2, c2, a2 = cell_fwd(r64["pre"][l] - lost, c0[l])
            for k, v in (("acts", a2), ("hn", h2), ("cn", c2)):
                worst[k].append(((v - r64[k][l]).abs().max() / r64[k][l].abs().max()).item())
        for k, v in worst.items():
            out[f"{k}{l}"] = min(v)
    pl = r64["prelin"]
    out["out"] = min(((torch.relu(pl) - torch.relu(pl - lost)).abs().max() / r64["out"].abs().max()).item()
                     for lost in passes(P[-2], r64["hn"][L - 1]))
    return out


def backward_defects(case, r64, mode):
    """fp64: for every layer the smallest change of its gate gradients (= its bias gradients; the weight gradients are their
    outer products with a fixed vector, so the ratio is the same), over their max, when ONE strip is missing from the transposed
    product that feeds the layer: lin.weight^T dpre for the top layer, W_ih_{l+1}^T dgates_{l+1} below.  Also cross-checks the
    written-out cell backward against autograd."""
    L = case["L"]
    P = [p.double() for p in case["params"]]
    c0 = case["c0"].double()
    zero = torch.zeros_like(c0)
    dhn = case["wh"].double() if mode == "full" else zero
    dcn = case["wc"].double() if mode in ("full", "cn") else zero
    d = case["a"].double() * (r64["out"] > 0)
    w = P[-2]
    out = {}
    for l in reversed(range(L)):
        shares = strip_shares(w, d)
        dh = shares.sum(0) + dhn[l]
        dg = cell_bwd(r64["acts"][l], r64["cn"][l], c0[l], dh, dcn[l])
        assert rel(dg, r64["grads"][4 * l + 2]) < 1e-12, "the written-out cell backward disagrees with autograd"
        dg2 = cell_bwd(r64["acts"][l], r64["cn"][l], c0[l], dh - shares, dcn[l])
        out[l] = ((dg2 - dg).abs().amax(1) / dg.abs().max()).min().item()
        w, d = P[4 * l], dg
    return out


class Table:
    """Measured error, yardstick, bar and defect of every checked tensor of one case; asserted after it has been printed."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def check(self, name, got, ref, cpu32, defect=None):
        err, dc = rel(got, ref), rel(cpu32, ref)
        bar = FACTOR * dc
        self.rows.append(f"{name} {err:.2e}/{dc:.2e}" + ("" if defect is None else f"/{defect:.1e}"))
        if not err <= bar:
            self.bad.append(f"{name}: error {err:.3e} above the bar {bar:.3e} (d_cpu32 {dc:.3e})")
        if defect is not None and not defect >= 10 * bar:
            self.bad.append(f"{name}: the smallest defect {defect:.3e} is below 10 bars ({bar:.3e})")

    def exact(self, name, got, ref):
        ok = torch.equal(got, ref)
        self.rows.append(f"{name} {'exact' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append(f"{name}: not bit-identical ({(got != ref).sum().item()} entries differ)")

    def finish(self):
        print(f"\n{self.tag} [error/d_cpu32(/defect)]: " + "  ".join(self.rows))
        assert not self.bad, self.tag + ":\n" + "\n".join(self.bad)


def relu_kink_is_clear(tb, r64, r32, bar_out):
    """The comparison of the gradients needs ONE ReLU mask: the CPU fp32 step must have the fp64 one, and no fp64 pre-activation
    other than the exact zero of the zero row may lie within the forward bar of the kink (then a kernel inside the bar has it
    too).  A property of the operands, computed on the host."""
    assert torch.equal(r32["prelin"] > 0, r64["prelin"] > 0), f"{tb.tag}: the CPU fp32 step flips a ReLU sign: choose another seed"
    pl = r64["prelin"]
    near = (pl != 0) & (pl.abs() <= bar_out * r64["out"].abs().max())
    assert not bool(near.any()), f"{tb.tag}: {int(near.sum())} head pre-activations within the forward bar of 0: choose another seed"


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def raw_forward(h, P, inp, h0, c0, L, C, Hd, N):
    """egz_lstm_b1_fwd through the C-ABI into NaN-filled buffers (hipops allocates its outputs itself)."""
    xt, acts, hn, cn, out = nan_like((C,)), nan_like((L, 4 * Hd)), nan_like((L, Hd)), nan_like((L, Hd)), nan_like((N,))
    from egaze_amd._lib import check
    check(h.LIB.egz_lstm_b1_fwd(h._ptr_table(P), L, inp.data_ptr(), h0.data_ptr(), c0.data_ptr(), xt.data_ptr(), acts.data_ptr(),
                                hn.data_ptr(), cn.data_ptr(), out.data_ptr(), C, Hd, N, h._stream()), "egz_lstm_b1_fwd")
    return xt, acts, hn, cn, out


def backward(h, P, fw, a, dhn, dcn, h0, c0, skip=None):
    """lstm_b1_bwd into NaN-filled gradient buffers (entry ``skip`` withheld) -> the list of gradients."""
    grads = [None if i == skip else nan_like(tuple(p.shape)) for i, p in enumerate(P)]
    xt, acts, hn, cn, out = fw
    h.lstm_b1_bwd(P, grads, a, dhn, dcn, xt, acts, h0, c0, hn, cn, out)
    return grads


def run_case(L, C, Hd, N, seed, wscale=1.0, gate_limit=None, tag=""):
    h = H()
    case = make_case(L, C, Hd, N, seed, wscale)
    nm = names(L)
    P = [p.to(DEV) for p in case["params"]]
    inp, h0, c0, a = (case[k].to(DEV) for k in ("inp", "h0", "c0", "a"))
    wh, wc = case["wh"].to(DEV), case["wc"].to(DEV)
    tb = Table(f"lstm_b1 L={L} C={C} H={Hd} N={N}{tag}")

    # ------------------------------------------------------------------ forward
    fw = h.lstm_b1_fwd(P, inp, h0, c0)
    raw = raw_forward(h, P, inp, h0, c0, L, C, Hd, N)
    fw2 = h.lstm_b1_fwd(P, inp, h0, c0)
    lean = h.lstm_b1_fwd(P, inp, h0, c0, want_acts=False)
    torch.cuda.synchronize()
    xt, acts, hn, cn, out = fw
    for k, t, t_raw, t2 in zip(("xt", "acts", "hn", "cn", "out"), fw, raw, fw2):
        assert bool(torch.isfinite(t_raw).all()), f"{tb.tag}: {k} is not written in full (or not finite)"
        tb.exact(f"{k} [NaN-filled buffer]", t_raw, t)
        tb.exact(f"{k} [second call]", t2, t)
    assert lean[1] is None
    for k, i in (("hn", 2), ("cn", 3), ("out", 4)):
        tb.exact(f"{k} [want_acts=False]", lean[i], fw[i])

    r64 = {m: torch_step(case, torch.float64, m) for m in MODES}
    r32 = {m: torch_step(case, torch.float32, m) for m in MODES}
    f64, f32 = r64["full"], r32["full"]
    dfw = forward_defects(case, f64)
    tb.check("xt", xt, f64["xt"], f32["xt"])
    for l in range(L):
        for k, t in (("acts", acts), ("hn", hn), ("cn", cn)):
            tb.check(f"{k}{l}", t[l], f64[k][l], f32[k][l], defect=dfw[f"{k}{l}"])
    tb.check("out", out, f64["out"], f32["out"], defect=dfw["out"])
    relu_kink_is_clear(tb, f64, f32, FACTOR * rel(f32["out"], f64["out"]))
    alive = out.cpu() > 0
    assert not bool(alive[case["dead"]].any()) and bool(alive[~case["dead"]].any()), "dead head rows must be dead, others not all"
    if N > 5:
        assert out[5].item() == 0.0 and f64["prelin"][5].item() == 0.0
    assert bool((f64["out"][::STRIP] > 0).all()), "every strip of head rows must carry gradient"
    if gate_limit is not None:
        gates = f64["pre"].view(L, 4, Hd)[:, (0, 1, 3)]
        tb.rows.append(f"[sigmoid pre-activations {gates.min().item():.1f} .. {gates.max().item():.1f}]")
        assert gates.max().item() > gate_limit and gates.min().item() < -gate_limit, "the saturation case must reach its limit"

    # ------------------------------------------------------------------ backward, three ways
    got = {}
    for mode in MODES:
        dhn = wh if mode == "full" else None
        dcn = wc if mode in ("full", "cn") else None
        grads = got[mode] = backward(h, P, fw, a, dhn, dcn, h0, c0)
        torch.cuda.synchronize()
        for k, g in zip(nm, grads):
            assert bool(torch.isfinite(g).all()), f"{tb.tag} [{mode}]: d {k} is not written in full (or not finite)"
        dbw = backward_defects(case, r64[mode], mode)
        for i, (k, g) in enumerate(zip(nm, grads)):
            tb.check(f"[{mode}] d {k}", g, r64[mode]["grads"][i], r32[mode]["grads"][i], defect=dbw[i // 4] if i < 4 * L else None)
        # exact by construction
        cpu = [g.cpu() for g in grads]
        for l in range(L):
            db = cpu[4 * l + 2]
            tb.exact(f"[{mode}] d b_hh_l{l} == d b_ih_l{l}", cpu[4 * l + 3], db)
            vin = xt.cpu() if l == 0 else hn[l - 1].cpu()
            tb.exact(f"[{mode}] d w_ih_l{l} == outer", cpu[4 * l], torch.outer(db, vin))
            tb.exact(f"[{mode}] d w_hh_l{l} == outer", cpu[4 * l + 1], torch.outer(db, case["h0"][l]))
        tb.exact(f"[{mode}] d lin.weight == outer", cpu[-2], torch.outer(cpu[-1], hn[L - 1].cpu()))
        tb.exact(f"[{mode}] d lin.bias == masked dout", cpu[-1], torch.where(alive, case["a"], torch.zeros(N)))

    # ------------------------------------------------------------------ the same launch asked in other ways
    again = backward(h, P, fw, a, wh, wc, h0, c0)
    zeros = backward(h, P, fw, a, torch.zeros_like(wh), torch.zeros_like(wc), h0, c0)
    for i, k in enumerate(nm):
        tb.exact(f"d {k} [second call]", again[i], got["full"][i])
        tb.exact(f"d {k} [dhn = dcn = 0 vs None]", zeros[i], got["out"][i])
    # one gradient withheld, once per kind (the LSTM kinds in the top layer, where every launch of the chain still depends on them)
    for skip in [4 * (L - 1) + j for j in range(4)] + [4 * L, 4 * L + 1]:
        part = backward(h, P, fw, a, wh, wc, h0, c0, skip=skip)
        same = all(torch.equal(part[i], got["full"][i]) for i in range(len(nm)) if i != skip)
        tb.rows.append(f"[d {nm[skip]} = None] {'exact' if same else 'DIFFERS'}")
        if not same:
            tb.bad.append(f"withholding d {nm[skip]} changes another gradient")
    torch.cuda.synchronize()
    tb.finish()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_lstm_b1_step_against_fp64(shape):
    """Forward tensors (xt, per layer acts / hn / cn, out) and all 4L + 2 gradients in the three loss forms within 4 x d_cpu32 of
    fp64, every bar behind a reduction at least 10 x below one lost pass / strip; the bit-level identities (bias pairs, rank-1
    weight gradients, the ReLU mask with dead rows and an exact-zero row); outputs and gradients written in full into NaN-filled
    buffers; null gradient entries, zero vs null state gradients, repeated calls and want_acts=False bit-identical."""
    L, C, Hd, N = shape
    run_case(L, C, Hd, N, seed=1000 + C + Hd + N + L)


@pytest.mark.parametrize("wscale,seed,limit", [(40.0, 4048, 80.0), (64.0, 4040, 89.0)], ids=["x40", "x64"])
def test_lstm_b1_saturated_gates_stay_finite_and_match_fp64(wscale, seed, limit):
    """The product shape with every weight and bias x 40: sigmoid pre-activations beyond +-80 (asserted on the fp64 run; the seed
    is the first from 4040 whose operands get there on both sides), and x 64: beyond +-89, where expf(-x) is inf and
    1 / (1 + expf(-x)) has to come out as 0 (asserted likewise).  Half the units above layer 0 are kept out of saturation
    (make_case) so that every strip of the lower transposed product carries gradient.  Same assertions as the regular cases,
    the defect conditions included: everything written, everything finite, everything inside its bar."""
    run_case(2, 512, 512, 512, seed=seed, wscale=wscale, gate_limit=limit, tag=f" weights x {wscale:g}")


# ---------------------------------------------------------------------------------------------- refusals
def dev_case(L, C, Hd, N, seed=7):
    case = make_case(L, C, Hd, N, seed)
    return case, [p.to(DEV) for p in case["params"]], case["inp"].to(DEV), case["h0"].to(DEV), case["c0"].to(DEV)


@pytest.mark.parametrize("C,Hd", [(18, 16), (16, 18), (16, 6)])
def test_lstm_b1_refuses_sizes_that_are_no_multiple_of_four(C, Hd):
    """The kernels use 16-byte loads on rows of C and H floats: the C-ABI refuses other sizes before any launch, forward and
    backward."""
    from egaze_amd._lib import EgazeHipError
    h = H()
    L, N = 2, 8
    case, P, inp, h0, c0 = dev_case(L, C, Hd, N)
    with pytest.raises(EgazeHipError, match="multiples of 4"):
        h.lstm_b1_fwd(P, inp, h0, c0)
    fw = (torch.zeros(C, device=DEV), torch.zeros(L, 4 * Hd, device=DEV), torch.zeros(L, Hd, device=DEV),
          torch.zeros(L, Hd, device=DEV), torch.zeros(N, device=DEV))
    with pytest.raises(EgazeHipError, match="multiples of 4"):
        backward(h, P, fw, case["a"].to(DEV), None, None, h0, c0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", [0, 1, 5, 8])
def test_lstm_b1_refuses_a_parameter_view_off_by_one_float(which):
    """A contiguous view that starts one float into its buffer is not 16-byte aligned: refused by name (its index in the
    state-dict order) before any launch, forward and backward."""
    from egaze_amd._lib import EgazeHipError
    h = H()
    L, C, Hd, N = 2, 16, 16, 8
    case, P, inp, h0, c0 = dev_case(L, C, Hd, N)
    good = h.lstm_b1_fwd(P, inp, h0, c0)
    buf = torch.zeros(P[which].numel() + 1, device=DEV)
    buf[1:].copy_(P[which].flatten())
    Q = list(P)
    Q[which] = buf[1:].view(P[which].shape)
    assert Q[which].is_contiguous() and Q[which].data_ptr() % 16 == 4
    with pytest.raises(EgazeHipError, match=f"parameter {which} is not 16-byte aligned"):
        h.lstm_b1_fwd(Q, inp, h0, c0)
    with pytest.raises(EgazeHipError, match=f"parameter {which} is not 16-byte aligned"):
        backward(h, Q, good, case["a"].to(DEV), None, None, h0, c0)
    torch.cuda.synchronize()


def test_lstm_b1_wrappers_refuse_inconsistent_shapes():
    """hipops infers (C, H, N) from w_ih_l0, w_hh_l0 and lin.weight and the C-ABI strides every other buffer by them: any of the
    4L + 2 parameters, h0 or c0 with another shape is a ValueError before the C-ABI is entered, forward and backward."""
    h = H()
    L, C, Hd, N = 2, 16, 24, 8
    case, P, inp, h0, c0 = dev_case(L, C, Hd, N)
    good = h.lstm_b1_fwd(P, inp, h0, c0)
    a = case["a"].to(DEV)

    def z(*shape):
        return torch.zeros(*shape, device=DEV)
    wrong = {"lin.weight columns": (8, z(N, Hd + 4)), "lin.bias": (9, z(N + 1)), "w_ih_l1 columns": (4, z(4 * Hd, C)),
             "w_hh_l0 rows": (1, z(4 * Hd + 4, Hd)), "w_ih_l0 rows": (0, z(4 * Hd - 4, C)), "b_ih_l0": (2, z(4 * Hd + 4)),
             "b_hh_l1": (7, z(Hd)), "w_hh_l1 columns": (5, z(4 * Hd, Hd - 4)), "lin.weight 1-D": (8, z(N * Hd))}
    for what, (i, t) in wrong.items():
        Q = list(P)
        Q[i] = t
        with pytest.raises(ValueError):
            h.lstm_b1_fwd(Q, inp, h0, c0)
        with pytest.raises(ValueError):
            backward(h, Q, good, a, None, None, h0, c0)
    for bad_state in (z(L + 1, Hd), z(L, Hd + 4), z(L * Hd)):
        with pytest.raises(ValueError):
            h.lstm_b1_fwd(P, inp, bad_state, c0)
        with pytest.raises(ValueError):
            h.lstm_b1_fwd(P, inp, h0, bad_state)
        with pytest.raises(ValueError):
            backward(h, P, good, a, None, None, bad_state, c0)
        with pytest.raises(ValueError):
            backward(h, P, good, a, None, None, h0, bad_state)
    with pytest.raises(ValueError):
        h.lstm_b1_fwd(P[:-1], inp, h0, c0)
    with pytest.raises(ValueError):
        h.lstm_b1_fwd(P, z(C + 4), h0, c0)
    with pytest.raises(ValueError):
        backward(h, P, good, z(N + 1), None, None, h0, c0)
    with pytest.raises(ValueError):
        h.lstm_b1_bwd(P, [None] * (len(P) - 1), a, None, None, *good[:2], h0, c0, *good[2:])
    # and the consistent call still runs
    g = backward(h, P, good, a, None, None, h0, c0)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in g)
