"""Non-finite propagation: plants, the two comparison rules and the fp64 references of the op-level cases.

The project's promise (INTEGRATION.md "failure words"): a NaN or inf that enters a step is still non-finite where the step
ends -- in the loss that is read back and in every gradient, where FusedAdam skips it and raises its flag.  That only holds if every
kernel between the input and the optimizer propagates a NaN the way the torch op it replaces does.  This module holds what the
tests of that chain share and needs no GPU:

  plant(t, kind, where)   writes NaN / +inf / -inf at a NAMED position of an operand (PLANTS: the positions where tile kernels go wrong)
  masks_agree(dev, ref)   the mask rule
  clean_twin(...)         the clean-twin rule (NaN plants)
  CASES                   the op-level cases: seeded operands, which of them are poisoned where, and the same op in torch fp64

tests/test_nonfinite_ref_host.py runs every reference on the CPU and refuses vacuous cases; tests/test_hip_nonfinite_ops.py runs the
same cases through hipops.

Two choices that are reasoned, not measured:
  * Weight plants sit on the CENTRE tap.  What NaN x (zero padding) gives depends on whether an implementation multiplies the
    halo zeros or skips them -- torch's own backends differ -- and is not what these tests are about.
  * inf plants go into activations and gradients only, and on the split-half legs only in front of epilogues without a ReLU: the
    f16 hi / lo split turns an inf into a NaN (accepted by the mask rule), and relu(-inf) = 0 in the reference cannot be asked of
    a NaN.  The exact-f32 legs take inf plants in front of the ReLU epilogue too.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


# ----------------------------------------------------------------------------- plants
def _act(s):            # (B, C, H, W) activation / gradient, NCHW on the host
    B, C, H, W = s
    d = {"interior": (0, C // 2, H // 2, W // 2),
         "corner": (0, 0, 0, 0),                                     # its halo is zero padding on two sides
         "last_row": (B - 1, 1 % C, H - 1, W // 2),
         "last_col": (0, C // 3, H // 2, W - 1),
         "last_channel": (B - 1, C - 1, H // 2, W // 2),          # C = 20 / 17: the last real channel before the pad to 32
         "last_tile": (B - 1, C - 1, H - 1, W - 1)}               # the last element: in the last (partial) pixel tile
    return d


def _weight(s):         # (K, C, 3, 3) / (K, C, 1, 1): centre tap only (module docstring)
    K, C = s[0], s[1]
    c = (s[2] // 2, s[3] // 2)
    return {"interior": (K // 2, C // 2) + c, "corner": (0, 0) + c, "last_channel": (K - 1, C - 1) + c}


def _vec(s):            # (K,) bias / BatchNorm parameter
    return {"interior": (s[0] // 2,), "corner": (0,), "last_channel": (s[0] - 1,)}


def _mat(s):            # (M, N) GEMM operand / (T, B, C) sequence / (L, B, H) state / (B, H, W) map: first, middle, last
    return {"interior": tuple(n // 2 for n in s), "corner": tuple(0 for _ in s), "last_tile": tuple(n - 1 for n in s)}


PLANTS: Dict[str, Callable] = {"act": _act, "weight": _weight, "vec": _vec, "mat": _mat}


def plant(t: torch.Tensor, kind: str, where: Tuple[str, str]) -> torch.Tensor:
    """A copy of ``t`` with KINDS[kind] written at PLANTS[where[0]](t.shape)[where[1]]."""
    idx = PLANTS[where[0]](tuple(t.shape))[where[1]]
    out = t.clone()
    out[idx] = KINDS[kind]
    return out


# ----------------------------------------------------------------------------- rules
def masks_agree(dev: torch.Tensor, ref64: torch.Tensor) -> Tuple[bool, str]:
    """NaN in the fp64 reference -> NaN on the device; +-inf -> non-finite (the f16 split turns an inf into a NaN);
    finite -> finite."""
    dev, ref64 = dev.detach().cpu(), ref64.detach()
    if tuple(dev.shape) != tuple(ref64.shape):
        return False, f"shape {tuple(dev.shape)} vs reference {tuple(ref64.shape)}"
    rn, ri, rf = torch.isnan(ref64), torch.isinf(ref64), torch.isfinite(ref64)
    bad_nan = rn & ~torch.isnan(dev)
    bad_inf = ri & torch.isfinite(dev)
    bad_fin = rf & ~torch.isfinite(dev)
    if bad_nan.any() or bad_inf.any() or bad_fin.any():
        first = torch.nonzero(bad_nan | bad_inf | bad_fin)[0].tolist()
        return False, (f"{int(bad_nan.sum())} of {int(rn.sum())} reference NaNs are not NaN on the device, {int(bad_inf.sum())} of "
                       f"{int(ri.sum())} reference infs are finite, {int(bad_fin.sum())} of {int(rf.sum())} finite elements are "
                       f"not; first at {first}: device {dev[tuple(first)].item()}, reference {ref64[tuple(first)].item()}")
    return True, ""


def untouched(ref_poisoned: torch.Tensor, ref_clean: torch.Tensor) -> torch.Tensor:
    """Mask of the output elements whose fp64 reference is bit-identical with and without the plant."""
    return ref_poisoned.detach().contiguous().view(torch.int64) == ref_clean.detach().contiguous().view(torch.int64)


def clean_twin(dev_poisoned, dev_clean, ref_poisoned, ref_clean, tol: Optional[float] = None) -> Tuple[bool, str]:
    """Where the plant does not reach in the reference, the device's poisoned run must equal its clean run: bit for bit, or within
    ``tol`` x max |clean| for an op documented as order-nondeterministic."""
    keep = untouched(ref_poisoned, ref_clean)
    a, b = dev_poisoned.detach().cpu().contiguous(), dev_clean.detach().cpu().contiguous()
    if tol is None:
        bits = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
        same = a.view(bits) == b.view(bits)
        bad = keep & ~same
    else:
        bad = keep & ~((a.double() - b.double()).abs() <= tol * b.double().abs().max())
    if bad.any():
        first = torch.nonzero(bad)[0].tolist()
        return False, (f"{int(bad.sum())} of {int(keep.sum())} elements the plant does not reach differ from the clean run; first at "
                       f"{first}: {a[tuple(first)].item()} vs {b[tuple(first)].item()}")
    return True, ""


# ----------------------------------------------------------------------------- op-level cases
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Case:
    """make() -> {operand: fp32 CPU tensor}; ref({operand: fp64}) -> {output: fp64 tensor}; poisons: [(operand, (shape kind, plant
    name), kinds)]; spreads: the op spreads a poison over a whole BatchNorm channel or the whole output (no finite element needed);
    tol: the clean-twin rule's tolerance where the op is documented as not bit-reproducible under a plant (one case: the pre-split
    gradient chain, see there), None = bit for bit."""

    def __init__(self, name, make, ref, poisons, spreads=False, tol=None):
        self.name, self.make, self.ref, self.poisons, self.spreads, self.tol = name, make, ref, poisons, spreads, tol
        self._ops = self._clean = None

    def operands(self):
        if self._ops is None:
            self._ops = self.make()
        return self._ops

    def run_ref(self, ops):
        with torch.enable_grad():
            out = self.ref({k: (v.double() if v.is_floating_point() else v) for k, v in ops.items()})
        return {k: v.detach() for k, v in out.items()}

    def clean_ref(self):
        if self._clean is None:
            self._clean = self.run_ref(self.operands())
        return self._clean

    def variants(self):
        return [(op, where, kind) for op, where, kinds in self.poisons for kind in kinds]


N_ = ("nan",)
NI = ("nan", "+inf")
NII = ("nan", "+inf", "-inf")


def _conv_ops(B, Hh, Ww, C, K, seed):
    return lambda: {"x": rnd(B, C, Hh, Ww, seed=seed), "w": rnd(K, C, 3, 3, seed=seed + 1, scale=(2.0 / (9 * C)) ** 0.5),
                    "b": rnd(K, seed=seed + 2, scale=0.1)}


def _conv_ref(epi, ups=False):
    def ref(o):
        x = F.interpolate(o["x"], scale_factor=2, mode="nearest") if ups else o["x"]
        y = F.conv2d(x, o["w"], o["b"], padding=1)
        out = {"y": torch.relu(y) if epi == 1 else y}
        if epi == 2:
            out["stat"] = torch.stack((y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))))
        return out
    return ref


def _conv_poisons(x_kinds, act_plants=("interior", "corner", "last_tile")):
    return ([("x", ("act", p), x_kinds if p == "interior" else N_) for p in act_plants]
            + [("w", ("weight", "last_channel"), N_), ("b", ("vec", "last_channel"), N_)])


def _bn_ops(B, Hh, Ww, K):
    def y():
        t = rnd(B, K, Hh, Ww, seed=15) * 1.7 + 0.3
        t[0, 0, 0, 0] = 5.0                       # open ReLU (and the window's maximum) where the gradient plant "corner" lands
        return t
    return lambda: {"y": y(), "gamma": torch.rand(K, generator=torch.Generator().manual_seed(16)) + 0.5,
                    "beta": rnd(K, seed=17, scale=0.2), "rm": rnd(K, seed=18, scale=0.1),
                    "rv": torch.rand(K, generator=torch.Generator().manual_seed(19)) + 0.5,
                    "dout_pool": rnd(B, K, Hh // 2, Ww // 2, seed=20), "dout": rnd(B, K, Hh, Ww, seed=21)}


def _bn_ref(pool, train=True):
    def ref(o):
        y = o["y"].clone().requires_grad_(True)
        g, b = o["gamma"].clone().requires_grad_(True), o["beta"].clone().requires_grad_(True)
        rm, rv = o["rm"].clone(), o["rv"].clone()
        out = torch.relu(F.batch_norm(y, rm, rv, g, b, train, 0.1, 1e-5))
        if pool:
            out = F.max_pool2d(out, 2, 2)
        res = {"out": out}
        if train:
            out.backward(o["dout_pool"] if pool else o["dout"])
            res.update(dy=y.grad, dgamma=g.grad, dbeta=b.grad, running_mean=rm, running_var=rv)
        return res
    return ref


def _chain_tail(o, y):
    """[BatchNorm (train) -> ReLU] of y, then the consuming convolution: its output, its BN sums and its weight gradient."""
    a = torch.relu(F.batch_norm(y, None, None, o["gamma"], o["beta"], True, 0.1, 1e-5))
    y2 = F.conv2d(a, o["w2"], o["b2"], padding=1)
    dw2 = torch.nn.grad.conv2d_weight(a, tuple(o["w2"].shape), o["dy2"], padding=1)
    return {"y2": y2, "stat2": torch.stack((y2.sum(dim=(0, 2, 3)), (y2 * y2).sum(dim=(0, 2, 3)))), "dw2": dw2}


def _chain_ref(o):
    return _chain_tail(o, F.conv2d(o["x"], o["w"], o["b"], padding=1))


def _lstm_ref(L):
    def ref(o):
        lstm = torch.nn.LSTM(512, 512, L).double()
        with torch.no_grad():
            for l in range(L):
                getattr(lstm, f"weight_ih_l{l}").copy_(o[f"w_ih{l}"]); getattr(lstm, f"weight_hh_l{l}").copy_(o[f"w_hh{l}"])
                getattr(lstm, f"bias_ih_l{l}").copy_(o[f"b_ih{l}"]); getattr(lstm, f"bias_hh_l{l}").copy_(o[f"b_hh{l}"])
        x, h0, c0 = (o[k].clone().requires_grad_(True) for k in ("x", "h0", "c0"))
        out, (hn, cn) = lstm(torch.tanh(x), (h0, c0))
        pred = torch.relu(F.linear(out, o["lin_w"], o["lin_b"]))
        ((pred * o["wo"]).sum() + (hn * o["wh"]).sum() + (cn * o["wc"]).sum()).backward()
        res = {"pred": pred, "hn": hn, "cn": cn, "dx": x.grad, "dh0": h0.grad, "dc0": c0.grad}
        for name, p in lstm.named_parameters():
            res["d_" + name] = p.grad
        return res
    return ref


def _cell_ref(o):
    gi, gf, gg, go = o["gates"].chunk(4, dim=1)
    act = torch.cat((torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)), 1)
    c = torch.sigmoid(gf) * o["c_prev"] + torch.sigmoid(gi) * torch.tanh(gg)
    return {"h": torch.sigmoid(go) * torch.tanh(c), "c": c, "act": act}


def _lstm_ops(L, T, B, seed):
    def make():
        g = torch.Generator().manual_seed(seed)
        r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
        o = {"x": r(T, B, 512), "h0": r(L, B, 512, sc=0.3), "c0": r(L, B, 512, sc=0.3), "wo": r(T, B, 512), "wh": r(L, B, 512),
             "wc": r(L, B, 512), "lin_w": r(512, 512, sc=0.04), "lin_b": r(512, sc=0.1)}
        for l in range(L):
            o.update({f"w_ih{l}": r(2048, 512, sc=0.04), f"w_hh{l}": r(2048, 512, sc=0.04), f"b_ih{l}": r(2048, sc=0.1),
                      f"b_hh{l}": r(2048, sc=0.1)})
        return o
    return make


# (tanh(+-inf) = +-1: an inf in x is no poison; an inf in c0 is -- c_n = f c_0 stays inf.  wh: the gradient arriving through h_n)
_LSTM_POISONS = [("x", ("mat", "interior"), N_), ("x", ("mat", "last_tile"), N_), ("h0", ("mat", "last_tile"), N_),
                 ("c0", ("mat", "corner"), NI), ("wh", ("mat", "last_tile"), N_)]


def _head_ops(C):
    return lambda: {"x": rnd(2, C, 9, 11, seed=27), "w": rnd(1, C, 1, 1, seed=28, scale=0.2), "b": torch.tensor([0.1]),
                    "dout": rnd(2, 1, 9, 11, seed=29)}


def _head_ref(o):
    x, w, b = (o[k].clone().requires_grad_(True) for k in ("x", "w", "b"))
    out = torch.sigmoid(F.conv2d(x, w, b))
    out.backward(o["dout"])
    return {"out": out[:, 0], "dx": x.grad, "dw": w.grad, "db": b.grad, "dw_nodx": w.grad, "db_nodx": b.grad}     # (_nodx: need_dx=False)


def _head_masked_ref(o):
    """sigmoid(conv1x1(a)) with a = the post-ReLU output of the block below; the gradient w.r.t. that block's pre-activation is
    threshold_backward(dx, a): torch lets a NaN activation pass its gradient."""
    a, w, b = (o[k].clone().requires_grad_(True) for k in ("x", "w", "b"))
    out = torch.sigmoid(F.conv2d(a, w, b))
    out.backward(o["dout"])
    dx = torch.ops.aten.threshold_backward(a.grad, a.detach(), 0.0)
    return {"dx": dx, "dbias": dx.sum(dim=(0, 2, 3)), "dw": w.grad, "db": b.grad}      # dbias: the masked form's partial rows, summed


def _floss_ops():
    g = torch.Generator().manual_seed(5)
    inp = torch.rand(2, 1, 16, 16, generator=g) * 0.9 + 0.05
    tgt = torch.rand(2, 1, 16, 16, generator=g)
    return {"inp": inp, "tgt": tgt}


def _floss_ref(o):
    from oracle import egaze_oracle as O
    inp = o["inp"].clone().requires_grad_(True)
    loss = O.floss_forward(inp, o["tgt"])
    loss.backward()
    return {"loss": loss.reshape(1), "dinp": inp.grad}


def _floss_gout_ref(o):
    from oracle import egaze_oracle as O
    inp = o["inp"].clone().requires_grad_(True)
    O.floss_forward(inp, o["tgt"]).backward(o["gout"][0])
    return {"dinp": inp.grad}


def _mse_gout_ref(o):
    a = o["a"].clone().requires_grad_(True)
    ((a - torch.tanh(o["b"])) ** 2).mean().backward(o["gout"][0])
    return {"da": a.grad}


def _bn_block(y, o):
    """relu(BatchNorm2d(train)(y)) with gamma / beta as leaves -> (activation, gamma, beta)."""
    g, b = o["gamma"].clone().requires_grad_(True), o["beta"].clone().requires_grad_(True)
    return torch.relu(F.batch_norm(y, None, None, g, b, True, 0.1, 1e-5)), g, b


def _first_block_ref(o):
    """Backward of the first [conv (C <= 3) -> BN (train) -> ReLU] block in one pass: dw, dgamma, dbeta."""
    w = o["w"].clone().requires_grad_(True)
    out, g, b = _bn_block(F.conv2d(o["x"], w, None, padding=1), o)
    out.backward(o["dout"])
    return {"dw": w.grad, "dgamma": g.grad, "dbeta": b.grad}


def _deferred_ref(o):
    """First conv -> BatchNorm whose output is never materialised (finalize from max / min rows) -> the consumer conv."""
    y = F.conv2d(o["x"], o["w"], o["b"], padding=1)
    rm, rv = o["rm"].clone(), o["rv"].clone()
    a = torch.relu(F.batch_norm(y, rm, rv, o["gamma"], o["beta"], True, 0.1, 1e-5))
    y2 = F.conv2d(a, o["w2"], o["b2"], padding=1)
    return {"y2": y2, "stat2": torch.stack((y2.sum(dim=(0, 2, 3)), (y2 * y2).sum(dim=(0, 2, 3)))), "running_mean": rm, "running_var": rv}


def _bnsums_ref(o):
    """conv(relu(BN(bn_y))) backward: the data gradient w.r.t. the activation, and the BatchNorm backward of the block below
    driven by the two sums the data-gradient launch folds."""
    y0 = o["bn_y"].clone().requires_grad_(True)
    a, g, b = _bn_block(y0, o)
    a.retain_grad()
    F.conv2d(a, o["w"], None, padding=1).backward(o["dy"])
    return {"dx": a.grad, "dyb": y0.grad, "dgamma": g.grad, "dbeta": b.grad}


def _bnsums_ops(B, Hh, Ww, C, K):
    return lambda: {"dy": rnd(B, K, Hh, Ww, seed=701), "w": rnd(K, C, 3, 3, seed=702, scale=(2.0 / (9 * C)) ** 0.5),
                    "bn_y": rnd(B, C, Hh, Ww, seed=703) * 1.3 + 0.2, "gamma": 1.0 + 0.3 * rnd(C, seed=704), "beta": 0.2 * rnd(C, seed=705)}


def _presplit_grad_ref(o):
    """[conv -> BN (train) -> ReLU] backward: BatchNorm backward writing dy as pairs, then the conv's data and weight gradients."""
    x, w = o["x"].clone().requires_grad_(True), o["w"].clone().requires_grad_(True)
    out, g, b = _bn_block(F.conv2d(x, w, o["b"], padding=1), o)
    out.backward(o["dout"])
    return {"dx": x.grad, "dw": w.grad, "dgamma": g.grad, "dbeta": b.grad}


def _ups_masked_dgrad_ref(o):
    a = o["a"].clone().requires_grad_(True)
    F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), o["w"], None, padding=1).backward(o["dy"])
    dx = torch.ops.aten.threshold_backward(a.grad, a.detach(), 0.0)
    return {"dx": dx, "dbias": dx.sum(dim=(0, 2, 3))}


def _mse_ref(tanh_t):
    def ref(o):
        a = o["a"].clone().requires_grad_(True)
        loss = ((a - (torch.tanh(o["b"]) if tanh_t else o["b"])) ** 2).mean()
        loss.backward()
        return {"loss": loss.reshape(1), "da": a.grad}
    return ref


def _dgrad_ref(ups=False):
    def ref(o):
        x = torch.zeros(o["xshape"].tolist(), dtype=torch.float64, requires_grad=True)
        xin = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
        F.conv2d(xin, o["w"], None, padding=1).backward(o["dy"])
        return {"dx": x.grad}
    return ref


def _dgrad_ops(B, Hh, Ww, C, K, seed, ups=False):
    return lambda: {"dy": rnd(B, K, Hh, Ww, seed=seed), "w": rnd(K, C, 3, 3, seed=seed + 1, scale=(2.0 / (9 * C)) ** 0.5),
                    "xshape": torch.tensor([B, C, Hh // 2, Ww // 2] if ups else [B, C, Hh, Ww])}


def _masked_dgrad_ref(o):
    """Data gradient of conv(a) with the ReLU backward of the layer below (a = its post-ReLU output) and that layer's bias gradient."""
    a = o["a"].clone().requires_grad_(True)
    F.conv2d(a, o["w"], None, padding=1).backward(o["dy"])
    dx = torch.ops.aten.threshold_backward(a.grad, a.detach(), 0.0)
    return {"dx": dx, "dbias": dx.sum(dim=(0, 2, 3))}


def _wgrad_ref(o):
    return {"dw": torch.nn.grad.conv2d_weight(o["x"], (o["dy"].shape[1], o["x"].shape[1], 3, 3), o["dy"], padding=1)}


def _wgrad_ops(B, Hh, Ww, C, K, seed):
    return lambda: {"x": rnd(B, C, Hh, Ww, seed=seed), "dy": rnd(B, K, Hh, Ww, seed=seed + 1)}


# (both operands' plants away from the border: what NaN x (the zero padding of x, the rows of dy past the image) gives is the
# implementation's choice, see above)
_WG_POISONS = [("x", ("act", "interior"), NI), ("x", ("act", "last_channel"), N_), ("dy", ("act", "interior"), N_),
               ("dy", ("act", "last_channel"), N_)]
_DG_POISONS_NAN = [("dy", ("act", p), N_) for p in ("interior", "corner", "last_tile")] + [("w", ("weight", "last_channel"), N_)]      # (pre-summed taps)
_DG_POISONS = [("dy", ("act", "interior"), NI), ("dy", ("act", "corner"), N_), ("dy", ("act", "last_tile"), N_),
               ("w", ("weight", "last_channel"), N_)]


def _relu_ops():
    out = torch.relu(rnd(3, 32, 4, 4, seed=24))
    for idx in _act((3, 32, 4, 4)).values():     # (a gradient plant behind a closed ReLU reaches nothing)
        out[idx] = 1.0
    return {"out": out, "g": rnd(3, 32, 4, 4, seed=25)}


def _relu_ref(o):
    dy = torch.ops.aten.threshold_backward(o["g"], o["out"], 0.0)
    return {"dy": dy, "dy_bias_form": dy, "db": dy.sum(dim=(0, 2, 3))}


def _pairmax_ops():
    a, b = rnd(2, 64, 5, 5, seed=21), rnd(2, 64, 5, 5, seed=22)
    b[0, :8, 0, 0] = a[0, :8, 0, 0]                       # ties: the first stream wins
    return {"a": a, "b": b, "dz": rnd(2, 64, 5, 5, seed=23)}


def _pairmax_ref(o):
    """nn.MaxPool3d((2, 1, 1)) over the depth-2 stack of the two streams (the reference's fusion block); its values equal
    torch.maximum's."""
    a, b = o["a"].clone().requires_grad_(True), o["b"].clone().requires_grad_(True)
    z = F.max_pool3d(torch.stack((a, b), dim=2), (2, 1, 1))[:, :, 0]
    z.backward(o["dz"])
    zm = torch.maximum(o["a"], o["b"])
    assert torch.equal(torch.isnan(z), torch.isnan(zm)) and torch.equal(z.detach().nan_to_num(0.0), zm.nan_to_num(0.0))
    return {"z": z, "da": a.grad, "db": b.grad}


def _gemm_ops():
    g = torch.Generator().manual_seed(0)
    return {"x": torch.randn(70, 130, generator=g), "w": torch.randn(50, 130, generator=g), "b": torch.randn(50, generator=g)}


def _first_ops(C, K=64):
    return lambda: {"x": rnd(1, C, 13, 21, seed=11), "w": rnd(K, C, 3, 3, seed=12, scale=(2.0 / (9 * C)) ** 0.5),
                    "b": rnd(K, seed=13, scale=0.1), "dy": rnd(1, K, 13, 21, seed=14)}


def _first_ref(o):
    w = o["w"].clone().requires_grad_(True)
    y = F.conv2d(o["x"], w, o["b"], padding=1)
    y.backward(o["dy"])
    return {"y": y, "stat": torch.stack((y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3)))).detach(), "dw": w.grad}


_FIRST_POISONS = [("x", ("act", "interior"), NI), ("x", ("act", "corner"), N_), ("x", ("act", "last_channel"), N_),
                  ("x", ("act", "last_tile"), N_), ("w", ("weight", "last_channel"), N_), ("dy", ("act", "last_col"), N_)]

_BN_POISONS = [("y", ("act", "interior"), NII), ("y", ("act", "last_tile"), N_), ("gamma", ("vec", "last_channel"), N_),
               ("dout", ("act", "corner"), N_), ("dout_pool", ("act", "last_row"), N_)]


CASES: List[Case] = [
    # --- 3x3 convolution forward, every leg (shapes: the smallest of each form's list in test_hip_ops.py)
    *[Case(f"conv_f32_epi{e}", _conv_ops(3, 9, 7, 32, 192, 1), _conv_ref(e), _conv_poisons(NII)) for e in (0, 1, 2)],
    *[Case(f"conv_{t}_epi{e}", _conv_ops(3, 9, 7, 32, 128, 41), _conv_ref(e), _conv_poisons(N_ if e == 1 else NI))
      for t in ("f16", "bf16") for e in (0, 1, 2)],
    *[Case(f"conv_streamed_epi{e}", _conv_ops(5, 5, 3, 64, 64, 61), _conv_ref(e), _conv_poisons(N_ if e == 1 else NI)) for e in (0, 1, 2)],
    *[Case(f"conv_streamed_narrow_epi{e}", _conv_ops(2, 16, 16, 32, 32, 61), _conv_ref(e), _conv_poisons(N_ if e == 1 else NI))
      for e in (0, 1, 2)],
    *[Case(f"conv_splitk_epi{e}", _conv_ops(1, 7, 9, 160, 128, 91), _conv_ref(e), _conv_poisons(N_ if e == 1 else NI)) for e in (0, 1, 2)],
    # (the phase forms multiply by PRE-SUMMED taps: inf (w1 + w2) is an inf where inf w1 + inf w2 may be a NaN -- NaN plants only)
    *[Case(f"conv_ups_{m}_epi{e}", _conv_ops(2, 6, 6, 64, 64, 4), _conv_ref(e, ups=True), _conv_poisons(NII if m == "fold" else N_))
      for m in ("fold", "phase") for e in (1, 2)],
    *[Case(f"conv_ups_streamed_epi{e}", _conv_ops(1, 5, 3, 64, 64, 81), _conv_ref(e, ups=True), _conv_poisons(N_)) for e in (0, 1)],
    Case("conv_padded_first", _conv_ops(2, 9, 7, 17, 64, 91), _conv_ref(2),
         _conv_poisons(NI, ("interior", "corner", "last_channel", "last_tile"))),
    Case("conv_first_c3", _first_ops(3), _first_ref, _FIRST_POISONS),
    Case("conv_first_c20", _first_ops(20), _first_ref, _FIRST_POISONS),
    # --- BatchNorm (train: finalize + apply + backward; eval coefficients), ReLU, pool
    *[Case(f"bn_k{K}_pool{int(p)}", _bn_ops(B, Hh, Ww, K), _bn_ref(p),
           [q for q in _BN_POISONS if q[0] != ("dout" if p else "dout_pool")], spreads=True)
      for (B, Hh, Ww, K) in ((2, 8, 8, 64), (2, 4, 4, 8)) for p in (False, True)],
    Case("bn_eval", _bn_ops(2, 8, 8, 64), _bn_ref(False, train=False),
         [("y", ("act", "interior"), NI), ("y", ("act", "last_tile"), N_), ("rv", ("vec", "last_channel"), N_),
          ("beta", ("vec", "corner"), N_)]),
    Case("presplit_chain", lambda: {**_conv_ops(2, 32, 32, 64, 64, 301)(), "gamma": 1.0 + 0.3 * rnd(64, seed=304),
                                    "beta": 0.2 * rnd(64, seed=305), "w2": rnd(64, 64, 3, 3, seed=306, scale=(2.0 / (9 * 64)) ** 0.5),
                                    "b2": rnd(64, seed=307, scale=0.1), "dy2": rnd(2, 64, 32, 32, seed=308, scale=1e-3)},
         _chain_ref, [("x", ("act", "interior"), N_), ("x", ("act", "last_tile"), N_), ("b", ("vec", "last_channel"), N_),
                      ("w2", ("weight", "last_channel"), N_), ("dy2", ("act", "corner"), N_)], spreads=True),
    Case("conv_bn_prologue", lambda: {"y0": rnd(2, 32, 16, 16, seed=401) * 1.3 + 0.2, "gamma": 1.0 + 0.3 * rnd(32, seed=402),
                                      "beta": 0.2 * rnd(32, seed=403), "w2": rnd(32, 32, 3, 3, seed=404, scale=(2.0 / (9 * 32)) ** 0.5),
                                      "b2": rnd(32, seed=405, scale=0.1), "dy2": rnd(2, 32, 16, 16, seed=406, scale=1e-3)},
         lambda o: _chain_tail(o, o["y0"]),
         [("y0", ("act", "interior"), N_), ("y0", ("act", "last_tile"), N_), ("gamma", ("vec", "last_channel"), N_),
          ("w2", ("weight", "last_channel"), N_), ("dy2", ("act", "corner"), N_)], spreads=True),
    Case("conv_bn_prologue_k8", lambda: {"y0": rnd(2, 32, 16, 16, seed=401) * 1.3 + 0.2, "gamma": 1.0 + 0.3 * rnd(32, seed=402),
                                         "beta": 0.2 * rnd(32, seed=403), "w2": rnd(8, 32, 3, 3, seed=404, scale=(2.0 / (9 * 32)) ** 0.5),
                                         "b2": rnd(8, seed=405, scale=0.1), "dy2": rnd(2, 8, 16, 16, seed=406, scale=1e-3)},
         lambda o: _chain_tail(o, o["y0"]),      # K = 8: the tap-packed weight-gradient kernel's prologue
         [("y0", ("act", "interior"), N_), ("gamma", ("vec", "last_channel"), N_), ("w2", ("weight", "last_channel"), N_),
          ("dy2", ("act", "interior"), N_)], spreads=True),
    *[Case(f"first_block_bwd_c{C}", (lambda C=C: {"x": rnd(2, C, 9, 16, seed=611), "w": rnd(32, C, 3, 3, seed=612, scale=0.3),
                                                  "gamma": torch.rand(32, generator=torch.Generator().manual_seed(613)) + 0.5,
                                                  "beta": rnd(32, seed=614, scale=0.2), "dout": rnd(2, 32, 9, 16, seed=615)}),
           _first_block_ref, [("dout", ("act", "last_row"), NI), ("dout", ("act", "last_col"), N_), ("x", ("act", "interior"), N_),      # (open ReLUs)
                              ("gamma", ("vec", "last_channel"), N_), ("w", ("weight", "last_channel"), N_)], spreads=True)
      for C in (2, 3)],
    Case("deferred_chain", lambda: {"x": rnd(2, 2, 16, 16, seed=801), "w": rnd(32, 2, 3, 3, seed=802, scale=0.3), "b": rnd(32, seed=803, scale=0.1),
                                    "gamma": 1.0 + 0.3 * rnd(32, seed=804), "beta": 0.2 * rnd(32, seed=805), "rm": rnd(32, seed=806, scale=0.1),
                                    "rv": torch.rand(32, generator=torch.Generator().manual_seed(807)) + 0.5,
                                    "w2": rnd(32, 32, 3, 3, seed=808, scale=(2.0 / (9 * 32)) ** 0.5), "b2": rnd(32, seed=809, scale=0.1)},
         _deferred_ref, [("x", ("act", "interior"), N_), ("w", ("weight", "last_channel"), N_), ("gamma", ("vec", "last_channel"), N_),
                         ("w2", ("weight", "last_channel"), N_), ("rm", ("vec", "corner"), N_)], spreads=True),
    *[Case(name, _bnsums_ops(*geo), _bnsums_ref,
           [("dy", ("act", "interior"), N_), ("w", ("weight", "last_channel"), N_), ("bn_y", ("act", "interior"), N_),
            ("gamma", ("vec", "last_channel"), N_)], spreads=True)
      for name, geo in (("dgrad_bnsums_wide", (3, 9, 7, 64, 128)), ("dgrad_bnsums_narrow", (2, 16, 16, 32, 32)))],
    # The pre-split GRADIENT pairs are scaled by a bound that a poisoned channel's sums turn non-finite (the scale then falls
    # back to 1), and pairs under another power-of-two scale round their sub-window elements differently (hipops/conv.py,
    # PRESPLIT_GRAD: "not bit-identical"): the clean twin is held to the 2e-6 of test_presplit_gradient_chain instead of bits.
    Case("presplit_grad_chain", lambda: {"x": rnd(2, 64, 32, 32, seed=501).clamp_(min=0), "w": rnd(64, 64, 3, 3, seed=502, scale=(2.0 / (9 * 64)) ** 0.5),
                                         "b": rnd(64, seed=503, scale=0.1), "gamma": 1.0 + 0.3 * rnd(64, seed=504), "beta": 0.2 * rnd(64, seed=505),
                                         "dout": rnd(2, 64, 32, 32, seed=506)},
         _presplit_grad_ref, [("dout", ("act", "interior"), N_), ("x", ("act", "last_tile"), N_), ("gamma", ("vec", "last_channel"), N_),
                              ("w", ("weight", "last_channel"), N_)], spreads=True, tol=2e-6),
    Case("pairmax", _pairmax_ops, _pairmax_ref,
         [("a", ("act", "interior"), NI), ("b", ("act", "last_tile"), NI), ("a", ("act", "corner"), N_), ("dz", ("act", "last_row"), N_)]),
    Case("relu_bwd", _relu_ops, _relu_ref,
         [("out&g", ("act", "interior"), N_), ("out&g", ("act", "last_tile"), N_), ("g", ("act", "corner"), NII), ("g", ("act", "last_channel"), N_)]),
    Case("upsample2x_bwd", lambda: {"g": rnd(2, 64, 6, 10, seed=31)},
         lambda o: {"dx": F.avg_pool2d(o["g"], 2, 2) * 4.0}, [("g", ("act", "interior"), NII), ("g", ("act", "last_tile"), N_)]),
    # --- GEMM, head, losses, tanh
    Case("gemm_bias_relu", _gemm_ops, lambda o: {"out": torch.relu(o["x"] @ o["w"].t() + o["b"])},
         [("x", ("mat", "interior"), NII), ("x", ("mat", "last_tile"), N_), ("w", ("mat", "last_tile"), N_), ("b", ("vec", "last_channel"), N_)]),
    *[Case(f"head_c{C}", _head_ops(C), _head_ref,
           [("x", ("act", "interior"), NII), ("x", ("act", "last_tile"), N_), ("w", ("weight", "last_channel"), N_),
            ("dout", ("act", "last_tile"), N_)], spreads=True) for C in (8, 64)],
    Case("head_masked_c8", lambda: {**_head_ops(8)(), "x": torch.relu(rnd(2, 8, 9, 11, seed=31))}, _head_masked_ref,
         [("x&dout", ("act", "interior"), N_), ("x", ("act", "last_tile"), N_), ("dout", ("act", "corner"), N_)], spreads=True),
    Case("floss", _floss_ops, _floss_ref, [("inp", ("act", "interior"), N_), ("inp", ("act", "last_tile"), N_), ("inp", ("act", "corner"), N_)],
         spreads=True),
    Case("floss_gout", lambda: {**_floss_ops(), "gout": torch.tensor([0.7])}, _floss_gout_ref, [("gout", ("vec", "corner"), NII)], spreads=True),
    Case("mse_gout", lambda: {"a": rnd(1, 1, 512, seed=32), "b": rnd(1, 1, 512, seed=33), "gout": torch.tensor([0.7])}, _mse_gout_ref,
         [("gout", ("vec", "corner"), NII)], spreads=True),
    *[Case(f"mse_tanh{int(t)}", lambda: {"a": rnd(1, 1, 512, seed=32), "b": rnd(1, 1, 512, seed=33)}, _mse_ref(t),
           [("a", ("mat", "interior"), NII), ("a", ("mat", "last_tile"), N_)], spreads=True) for t in (False, True)],
    Case("tanh", lambda: {"x": rnd(3, 2, 512, seed=34)}, lambda o: {"y": torch.tanh(o["x"])},
         [("x", ("mat", "interior"), N_), ("x", ("mat", "last_tile"), N_)]),
    # --- 3x3 convolution backward
    Case("dgrad_f32", _dgrad_ops(2, 12, 12, 64, 64, 7), _dgrad_ref(), _DG_POISONS),
    Case("dgrad_f16", _dgrad_ops(2, 10, 12, 64, 64, 44), _dgrad_ref(), _DG_POISONS),
    Case("dgrad_streamed", _dgrad_ops(5, 5, 3, 64, 64, 64), _dgrad_ref(), _DG_POISONS),
    Case("ups_dgrad_f32", _dgrad_ops(2, 12, 12, 64, 128, 10, ups=True), _dgrad_ref(ups=True), _DG_POISONS_NAN),
    Case("ups_dgrad_streamed", _dgrad_ops(1, 10, 6, 128, 64, 73, ups=True), _dgrad_ref(ups=True), _DG_POISONS_NAN),
    Case("dgrad_masked", lambda: {"dy": rnd(5, 64, 5, 3, seed=51), "w": rnd(64, 64, 3, 3, seed=52, scale=0.06),
                                  "a": torch.relu(rnd(5, 64, 5, 3, seed=53))}, _masked_dgrad_ref,
         [("dy", ("act", "interior"), N_), ("dy", ("act", "last_tile"), N_), ("a&dy", ("act", "interior"), N_), ("a&dy", ("act", "corner"), N_)]),
    Case("ups_dgrad_masked", lambda: {"dy": rnd(1, 64, 10, 6, seed=73), "w": rnd(64, 128, 3, 3, seed=74, scale=0.04),
                                      "a": torch.relu(rnd(1, 128, 5, 3, seed=75))}, _ups_masked_dgrad_ref,
         [("dy", ("act", "interior"), N_), ("dy", ("act", "last_tile"), N_), ("a&dy", ("act", "interior"), N_)]),
    Case("wgrad_split", _wgrad_ops(2, 7, 8, 64, 64, 21), _wgrad_ref, _WG_POISONS),
    Case("wgrad_narrow", _wgrad_ops(2, 9, 16, 8, 4, 21), _wgrad_ref, _WG_POISONS),
    Case("wgrad_f32", _wgrad_ops(2, 10, 6, 192, 64, 7), _wgrad_ref, _WG_POISONS),
    # --- LSTM: wavefront, persistent and batch-1 forms of nn.LSTM -> Linear -> ReLU, forward and backward
    Case("lstm_cell", lambda: {"gates": rnd(3, 2048, seed=71), "c_prev": rnd(3, 512, seed=72, scale=0.5)}, _cell_ref,
         [("gates", ("mat", "interior"), N_), ("gates", ("mat", "last_tile"), N_), ("c_prev", ("mat", "last_tile"), NII)]),
    Case("lstm_wave_l1", _lstm_ops(1, 1, 2, 112), _lstm_ref(1), _LSTM_POISONS),
    Case("lstm_wave_l2", _lstm_ops(2, 2, 33, 233), _lstm_ref(2), _LSTM_POISONS),
    Case("lstm_persist_t1b1", _lstm_ops(2, 1, 1, 211), _lstm_ref(2), _LSTM_POISONS, spreads=True),
    Case("lstm_persist_t3b16", _lstm_ops(2, 3, 16, 316), _lstm_ref(2), _LSTM_POISONS),
    Case("lstm_b1", _lstm_ops(2, 1, 1, 11), _lstm_ref(2), _LSTM_POISONS, spreads=True),
]
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)


def case_ids():
    return [(c.name, op, where, kind) for c in CASES for op, where, kind in c.variants()]


def poisoned_operands(case: Case, op: str, where, kind: str):
    ops = dict(case.operands())
    for name in op.split("&"):                   # "a&dy": the same position of both (a poisoned step has NaN in the activation AND its gradient)
        ops[name] = plant(ops[name], kind, where)
    return ops


# ----------------------------------------------------------------------------- step-level plants and their oracle
SP_SIZE, SP_B, SP_LR = 64, 4, 1e-4            # TRAJ_SIZE / TRAJ_B / TRAJ_LR of test_hip_model_sp.py
SP_PLANTS = ("input_pixel", "encoder_weight", "decoder_bias")


def sp_plant_target(shapes, name):
    """(state-dict key or 'x_t', index, kind) of an SP step plant: (a) one NaN pixel of the flow input, (b) one +inf in the centre tap
    of the middle conv of the RGB encoder, (c) one NaN in the bias of a decoder conv."""
    if name == "input_pixel":
        return "x_t", (1, 7, 20, 33), "nan"
    if name == "encoder_weight":
        convs = [k for k in shapes if k.startswith("features_s.") and k.endswith(".weight") and len(shapes[k]) == 4]
        k = convs[len(convs) // 2]
        return k, (shapes[k][0] // 2, shapes[k][1] // 2, 1, 1), "+inf"
    biases = [k for k in shapes if k.startswith("decoder.") and k.endswith(".bias") and shapes[k][0] > 1]
    return biases[len(biases) // 2], (0,), "nan"


def sp_oracle_poisoned(name, grads=False):
    """The oracle's train-mode forward of the poisoned SP step (seed-41 batch) -> (loss, state dict with the updated BN buffers);
    ``grads``: the whole step -> (loss, state dict, gradients)."""
    from oracle import egaze_oracle as O
    from oracle import synth
    sd = synth.synth_state_dict(O.sp_shapes(), seed=1, head_gain=0.25)
    x_s, x_t, gt, _ = synth.synth_sp_batch(SP_B, SP_SIZE, seed=41)
    key, idx, kind = sp_plant_target(O.sp_shapes(), name)
    if key == "x_t":
        x_t[idx] = KINDS[kind]
    else:
        sd[key][idx] = KINDS[kind]
    if grads:
        loss, _, g = O.sp_train_step(sd, {}, 1, x_s, x_t, gt, SP_LR)
        return loss, sd, g
    with torch.no_grad():
        out, _ = O.sp_forward(sd, x_s, x_t, training=True)
        loss = O.floss_forward(out, gt.view(out.shape))
    return loss, sd


AT_PLANTS = {"h0": ("h0", "last_tile"), "input": ("x", "interior")}


def at_inputs(T, B, seed):
    from oracle import synth
    x, tgt = synth.synth_at_batch(T, B, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return x, tgt, torch.randn(2, B, 512, generator=g) * 0.1, torch.randn(2, B, 512, generator=g) * 0.1


def at_poisoned_inputs(T, B, seed, name):
    x, tgt, h0, c0 = at_inputs(T, B, seed)
    op, where = AT_PLANTS[name]
    if op == "h0":
        h0 = plant(h0, "nan", ("mat", where))
    else:
        x = plant(x, "nan", ("mat", where))
    return x, tgt, h0, c0


def at_oracle_loss(x, tgt, h0, c0):
    """AT.py:138: criterion(lstm(input, hidden), tanh(target)) on the oracle, synth weights of seed 2."""
    from oracle import egaze_oracle as O
    from oracle import synth
    sd = synth.synth_state_dict(O.lstm_shapes(), seed=2)
    with torch.no_grad():
        out, _ = O.lstmnet_forward(sd, x, (h0, c0))
        return O.mse(out, torch.tanh(tgt))


LF_SIZE, LF_B = 32, 2                         # the smallest late-fusion step geometry of test_hip_lf.py
LF_PLANTS = {"input_pixel": ("feat", (1, 0, 20, 13), "nan"), "mid_weight": ("fusion.3.weight", (16, 16, 1, 1), "+inf"),
             "head_bias": ("fusion.9.bias", (0,), "nan")}


def lf_oracle_poisoned(name):
    """The oracle's train-mode forward of the poisoned late-fusion step (LF.py:90 argument order) -> (loss, state dict)."""
    from oracle import egaze_oracle as O
    from oracle import synth
    sd = synth.synth_state_dict(O.lf_shapes(), seed=3, head_gain=0.5)
    im, feat, gt = synth.synth_lf_batch(LF_B, LF_SIZE, seed=8)
    key, idx, kind = LF_PLANTS[name]
    if key == "feat":
        feat[idx] = KINDS[kind]
    else:
        sd[key][idx] = KINDS[kind]
    with torch.no_grad():
        out = O.late_fusion_forward(sd, feat, im, training=True)
        return O.floss_forward(out, gt), sd
