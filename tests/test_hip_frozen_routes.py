"""Frozen-parameter backward routes and gradient sinks against float64.

Every fused autograd node of functions.py branches its backward pass on ``ctx.needs_input_grad`` (skip the data gradient, skip
the weight gradient, relu_bwd vs relu_bwd_bias, masked vs plain head backward, the one-pass first-block backward) and on whether
the parameter has a gradient sink (hipops/sinks.py: the kernel writes ``p.grad`` in place, autograd gets None).  The rest of the
suite measures the all-trainable corner without an optimizer.  This file runs

  A. every fused block, built as a FusedSequential of stock modules, under every needs-grad subset (tests/frozen_ref.py lists
     them) against the same stock modules in fp64 with the same ``requires_grad`` pattern;
  B. the reference's default SP step (SP.py:63-81: encoders frozen, FusedAdam over fusion + bn + decoder) next to the
     all-trainable step, against the fp64 oracle, and through the SP driver;
  C. the sink contract on the GPU: three routes (sinks / hipops.DIRECT_GRADS = False / no optimizer) with one result,
     accumulation over two backward passes, one weight used twice in one graph under injected stream delays, and
     ``zero_grad(all_overwritten=True)``.

Part A inputs are flip-free: frozen_ref.SEEDS were picked on the CPU from the fp64 forward alone, and every test asserts the
margin again before it compares anything.
"""
import collections
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn

import frozen_ref as R
from oracle import synth
from stream_perturb import STATS, perturb
from test_hip_lf_step_ops import Recorder, chunk_defect
from test_hip_model_sp import GRAD_SEEDS, _small_oracle_pair, build_model, cos_norm, mostly_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELAY_MS = 2                   # tests/test_hip_stream_order.py: twice the delay at which its self-check sees every missing edge

EXTRA = ("relu_bwd", "conv3x3_ups_dgrad", "conv3x3_dgrad_masked", "colsum_f64", "pairmax_bwd", "stack2")
WGRAD = ("conv3x3_wgrad", "conv_first_wgrad", "bn_bwd_first_wgrad")
DGRAD = ("conv3x3_dgrad", "conv3x3_dgrad_bnsums", "conv3x3_dgrad_masked", "conv3x3_ups_dgrad")


@pytest.fixture(autouse=True)
def cpu_threads():
    """The fp64 references are a few tiny ops: eight host threads, not one fork / join per op over every core of the box."""
    keep = torch.get_num_threads()
    torch.set_num_threads(min(8, keep))
    try:
        yield
    finally:
        torch.set_num_threads(keep)


class RouteRecorder(Recorder):
    """test_hip_lf_step_ops.Recorder plus the entry points only the decoder and the fusion block launch."""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        for name in EXTRA:
            fn = getattr(self.h, name)
            monkeypatch.setattr(self.h, name, self._wrap(name, fn, inspect.signature(fn)))

    def take(self):
        calls, self.calls = self.calls, []
        return calls


class NodeSpy:
    """Wraps the backward of the four fused nodes: a gradient returned for an input that needs none is recorded (autograd
    itself drops such a tensor silently, so ``.grad is None`` alone cannot see a node that computed it anyway)."""

    def __init__(self, monkeypatch):
        import egaze_amd.functions as F
        self.unwanted = []
        for cls in (F.ConvBNReLUPool, F.ConvReLU, F.FusionBlock, F.HeadSigmoid):
            monkeypatch.setattr(cls, "backward", staticmethod(self._wrap(cls.__name__, cls.backward)))

    def _wrap(self, name, fn):
        def backward(ctx, *grads):
            res = fn(ctx, *grads)
            for i, (need, g) in enumerate(zip(ctx.needs_input_grad, res if isinstance(res, tuple) else (res,))):
                if g is not None and not need:
                    self.unwanted.append((name, i))
            return res
        return backward


def rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _rearm():
    """A backward pass that raised never ran its end-of-backward callback: re-arm it, as FusedAdam.zero_grad does."""
    import egaze_amd.functions as F
    F._JOIN_QUEUED[0] = False
    torch.cuda.synchronize()


# ================================================================================================ A. blocks x subsets
def hip_run(case, seed, on, rec):
    """The case on the HIP path with exactly the things in ``on`` requiring a gradient -> dict(out, grads, stats, fwd, bwd):
    the recorded launches of the forward and of the backward pass."""
    import egaze_amd.functions as F
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.utils import FusedSequential
    ref_net, inputs = R.make(case, seed)
    names = [k for k, _ in ref_net.named_parameters()]
    if case.kind == "late":
        net = late_fusion()
        net.load_state_dict({"fusion." + k: v for k, v in ref_net.state_dict().items()})
        params = {k: dict(net.named_parameters())["fusion." + k] for k in names}
        buffers = lambda: {k[7:]: v for k, v in net.named_buffers()}
    elif case.kind == "seq":
        net = FusedSequential(*ref_net.children())
        params = dict(net.named_parameters())
        buffers = lambda: dict(net.named_buffers())
    else:
        net = ref_net
        params = dict(net.named_parameters())
        buffers = lambda: dict(net.named_buffers())
    net.to(DEV).train()
    for k in names:
        params[k].requires_grad_(k in on)
    leaves = {}
    rec.take()
    rec.active = True
    if case.kind in ("seq", "late"):
        x = leaves["x"] = inputs["x"].to(DEV).requires_grad_("x" in on)
        out = net(x, fuse_sigmoid=case.head) if case.kind == "seq" else net(x[:, 0:1], x[:, 1:2])
    else:
        fs, ft = inputs["fs"].to(DEV), inputs["ft"].to(DEV)
        if case.kind == "fusion_halves":           # the two encoders' outputs as the halves of one NHWC buffer (model_SP.forward)
            B = fs.shape[0]
            buf = torch.empty((2 * B,) + tuple(fs.permute(0, 2, 3, 1).shape[1:]), device=DEV)
            buf[:B].copy_(fs.permute(0, 2, 3, 1))
            buf[B:].copy_(ft.permute(0, 2, 3, 1))
            fs, ft = buf[:B].permute(0, 3, 1, 2), buf[B:].permute(0, 3, 1, 2)
        fs, ft = fs.requires_grad_("fs" in on), ft.requires_grad_("ft" in on)
        leaves.update(fs=fs, ft=ft)
        bn = net.bn
        out = F.FusionBlock.apply(fs, ft, net.fusion.weight, net.fusion.bias, bn.weight, bn.bias, bn.running_mean,
                                  bn.running_var, bn.training, float(bn.momentum), float(bn.eps), bn.num_batches_tracked)
    torch.cuda.synchronize()
    fwd = rec.take()
    stats = {k: v.detach().clone() for k, v in buffers().items()}
    assert out.requires_grad
    try:
        out.backward(R.upstream(case, seed, out.shape).to(DEV))
        torch.cuda.synchronize()
    finally:
        rec.active = False
        bwd = rec.take()
    grads = {k: (None if t.grad is None else t.grad.detach().clone()) for k, t in list(leaves.items()) + list(params.items())}
    return dict(out=out.detach().clone(), grads=grads, stats=stats, fwd=fwd, bwd=bwd)


def conv_plan(case, on):
    """What the backward pass of the case must launch for ``on``: (weight-gradient launches as a Counter of (C as the kernel
    sees it, K), data-gradient launches as a Counter of (K, C), head input needs a gradient or None without a head)."""
    net, inputs = R.make(case, 0)
    wg, dg = collections.Counter(), collections.Counter()
    if isinstance(net, R.FusionRef):
        if "fusion.weight" in on:
            wg[(512, 512)] += 1
        if on & {"fs", "ft"}:
            dg[(512, 512)] += 1
        return wg, dg, None
    below = "x" in on          # something at or below the current layer's input needs a gradient
    head = None
    for name, m in net.named_children():
        if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
            C, K = m.in_channels, m.out_channels
            if f"{name}.weight" in on:
                wg[(32 if case.first and name == "0" and 16 <= C <= 32 else C, K)] += 1      # (the flow stack is padded to 32)
            if below:
                dg[(K, C)] += 1
        elif isinstance(m, nn.Conv2d):
            head = below
        below = below or any(f"{name}.{p}" in on for p, _ in m.named_parameters())
    return wg, dg, head


def launched(calls):
    wg, dg = collections.Counter(), collections.Counter()
    for c in calls:
        a = c["args"]
        if c["name"] == "conv3x3_wgrad":
            wg[(a["x"].shape[-1], a["dy"].shape[-1])] += 1
        elif c["name"] == "conv_first_wgrad":
            wg[(a["x_nchw"].shape[1], a["dy"].shape[-1])] += 1
        elif c["name"] == "bn_bwd_first_wgrad":
            wg[(a["x_nchw"].shape[1], a["y"].shape[-1])] += 1
        elif c["name"] in DGRAD:
            dg[(a["dy"].shape[-1], a["C"])] += 1
    return wg, dg


# Legitimate route differences between a subset and the control: (case, things on in the subset) -> {gradient: (the launch that
# produces it in the control, the launch that produces it in the subset)}, launch names as the recorder shows them.  These
# gradients are compared against fp64 alone; every other gradient a subset computes must carry the control's bits.
def route_difference(case, on, thing):
    """(control launch, subset launch) when ``thing``'s gradient legitimately comes from another launch than in the control,
    else None.  The table:

      block                       subset                                  gradients            control launch               subset launch
      first_lf, first_rgb         conv weight frozen                      gamma, beta          bn_bwd_first_wgrad           bn_relu_pool_bwd
      late_fusion                 fusion.0.weight frozen                  1.weight, 1.bias     bn_bwd_first_wgrad           bn_relu_pool_bwd
      tail, tail_head8, _nobias   nothing below the head needs a grad     head weight, bias    conv1x1_sigmoid_bwd_masked   conv1x1_sigmoid_bwd
      cr                          0.bias frozen                           x, 0.weight          relu_bwd_bias                relu_bwd
    (late_fusion's head sits on a BatchNorm block: it never takes the masked backward.)
    """
    th = R.things(case)
    first_w, first_bn = "0.weight", ("1.weight", "1.bias")
    if case.name in ("first_lf", "first_rgb", "late_fusion") and thing in first_bn and first_w not in on:
        return "bn_bwd_first_wgrad", "bn_relu_pool_bwd"
    if case.name == "cr" and thing != "0.bias" and "0.bias" not in on:
        return "relu_bwd_bias", "relu_bwd"
    if case.head and case.kind == "seq":
        head = [t for t in th if t.split(".")[0] == th[-1].split(".")[0]]
        if thing in head and not (on - set(head)):
            return "conv1x1_sigmoid_bwd_masked", "conv1x1_sigmoid_bwd"
    return None


@pytest.mark.parametrize("name", list(R.CASES))
def test_block_subsets_vs_fp64(name, monkeypatch):
    """Every needs-grad subset of one fused block: forward and BatchNorm statistics bit-identical to the control's, every
    computed gradient bit-identical to the control's (route_difference lists the exceptions) and within
    max(20 x the CPU-fp32 error, 2e-4) of fp64 autograd, frozen things untouched and their launches skipped.

    Observed on MI355X, max |d| / max |ref| against fp64 (the CPU-fp32 run of the same modules in brackets); the bar was 2e-4
    everywhere (20 x the fp32 error is below the floor at these sizes) and the worst gradient of any subset used 3 % of it:
      cbr            x 4.5e-07 (3.2e-07), 0.weight 3.4e-07 (3.3e-07), 1.weight 3.1e-07 (2.1e-07), 1.bias 3.0e-08 (7.5e-08)
      cbr_pool       x 3.2e-07 (2.6e-07), 0.weight 5.3e-07 (2.6e-07), 1.weight 2.8e-07 (2.5e-07), 1.bias 3.6e-08 (1.0e-07)
      cbr_chain      x 4.5e-07 (3.6e-07), 0.weight 4.4e-07 (3.5e-07), 3.weight 5.4e-07 (4.8e-07), BN 4.8e-08 ... 5.1e-07
      first_rgb      0.weight 9.8e-08 (1.5e-07), 1.weight 1.3e-07 (1.6e-07), 1.bias 4.2e-08 (8.4e-08)
      first_flow     0.weight 3.7e-07 (3.2e-07), 1.weight 2.5e-07 (2.3e-07), 1.bias 3.0e-08 (5.3e-08)
      first_lf       0.weight 9.7e-08 (2.1e-07), 1.weight 1.1e-07 (2.0e-07), 1.bias 2.8e-08 (5.5e-08)
      late_fusion    0.weight 1.0e-06 (3.1e-06), 3.weight 1.1e-06 (6.6e-06), 6.weight 1.4e-06 (1.5e-06), 9.weight 2.2e-07
                     (3.6e-07), 9.bias 9.0e-08 (4.8e-07), BN 3.3e-07 ... 1.2e-06
      tail           x 6.5e-07 (2.9e-07), 1.weight 5.7e-07 (7.7e-07), 1.bias 7.7e-07 (6.1e-07), 3.weight 6.6e-07 (4.6e-07),
                     3.bias 1.1e-06 (4.3e-07), 5.weight 1.1e-06 (4.2e-07), 5.bias 6.4e-06 (1.3e-06)
      tail_head8     x 5.0e-07 (2.1e-07), 1.weight 5.3e-07 (6.6e-07), 3.weight 4.1e-07 (3.1e-07), 5.weight 1.7e-07 (2.5e-07),
                     biases 1.5e-07 ... 4.2e-07
      tail_nobias    x 6.1e-07 (2.6e-07), 1.weight 4.5e-07 (5.5e-07), 3.weight 4.7e-07 (3.8e-07), 5.weight 4.5e-07 (5.8e-07)
      cr             x 5.1e-07 (2.2e-07), 0.weight 2.9e-07 (2.8e-07), 0.bias 4.2e-08 (1.1e-07)
      cr_nobias      x 6.1e-07 (2.2e-07), 0.weight 3.7e-07 (2.7e-07)
      fusion_*       fs 3.3e-07 (2.2e-07), ft 4.0e-07 (3.3e-07), fusion.weight 2.9e-07 (2.3e-07), bn.weight 5.1e-07 (3.2e-07),
                     bn.bias 3.3e-08 (7.6e-08); the halves and the stack2 branch give the same bits
    One dropped chunk of 16 pixels moves a weight or bias gradient by 8.8e-3 (late_fusion 9.bias) ... 0.7 of max |ref|: at
    least 44 x the bar.  Apart from the launches route_difference lists, every gradient of every subset had the control's bits."""
    case, seed = R.CASES[name], R.SEEDS[name]
    rec, spy = RouteRecorder(monkeypatch), NodeSpy(monkeypatch)
    rec.active = False
    zero = R.zero_bias(case)
    ctrl_on = R.control(case)
    ctrl = hip_run(case, seed, ctrl_on, rec)
    assert not spy.unwanted, spy.unwanted
    ctrl_names = [c["name"] for c in ctrl["bwd"]]
    # the yardstick: the same modules in fp32 through torch on the CPU (a thing's fp32 gradient does not depend on which other
    # things need one: run once, with the control's pattern)
    ref32 = R.run(case, seed, torch.float32, ctrl_on)
    worst, lines, problems = (0.0, None), [], []
    for label, on, refused in [("control", ctrl_on, False)] + R.subsets(case):
        if refused:
            with pytest.raises(NotImplementedError):
                hip_run(case, seed, on, rec)
            _rearm()
            continue
        got = ctrl if label == "control" else hip_run(case, seed, on, rec)
        ref64 = R.run(case, seed, torch.float64, on, taps=label == "control")
        assert ref64["margin"] >= R.MARGIN, (name, seed, ref64["margin"])           # flip-free, before anything is compared
        # 1. forward and statistics: freezing changes neither
        assert torch.equal(got["out"], ctrl["out"]), (name, label)
        assert rel(got["out"], ref64["out"]) < 1e-4
        for k, v in ctrl["stats"].items():
            assert torch.equal(got["stats"][k], v), (name, label, k)
            if v.is_floating_point():
                assert rel(v, ref64["stats"][k]) < 1e-4, (name, label, k)
            else:
                assert int(v) == int(ref64["stats"][k]) == 1, (name, label, k)
        names = [c["name"] for c in got["bwd"]]
        for t in R.things(case):
            g = got["grads"][t]
            # 4. frozen things stay untouched
            if t not in on:
                assert g is None and ref64["grads"][t] is None, (name, label, t)
                continue
            assert g is not None, (name, label, t)
            r64, r32 = ref64["grads"][t], ref32["grads"][t]
            # 2. the control's bits, unless the gradient legitimately comes from another launch
            diff = route_difference(case, on, t) if t in ctrl_on else None
            if diff is not None:
                assert diff[0] in ctrl_names and diff[1] in names and diff[0] not in names, (name, label, t, diff, names)
            elif t in ctrl_on and not torch.equal(g, ctrl["grads"][t]):
                problems.append(f"{label}: {t} differs from the control by {rel(g, ctrl['grads'][t]):.2e}; "
                                f"launches {sorted(set(names) ^ set(ctrl_names))}")
            # 3. against fp64, with the CPU-fp32 run of the same modules as the yardstick
            if t in zero:
                assert torch.count_nonzero(g).item() == 0, (name, label, t)
                scale = max([v.abs().max().item() for k, v in ref64["grads"].items() if v is not None and k not in zero],
                            default=1.0)
                assert r64.abs().max().item() < 1e-10 * scale, (name, label, t)
                continue
            e, e32 = rel(g, r64), rel(r32, r64)
            bar = max(20 * e32, 2e-4)
            if label == "control":
                lines.append(f"{t} {e:.1e} (fp32 {e32:.1e})")
            if e / bar > worst[0]:
                worst = (e / bar, f"{label}: {t} {e:.2e}, CPU fp32 {e32:.2e}, bar {bar:.2e}")
            if not e < bar:
                problems.append(f"{label}: {t} is {e:.2e} from fp64, CPU fp32 {e32:.2e}, bar {bar:.2e}")
        # 4. the work is really skipped
        assert not spy.unwanted, (name, label, spy.unwanted)
        want_wg, want_dg, head_dx = conv_plan(case, on)
        got_wg, got_dg = launched(got["bwd"])
        assert got_wg == want_wg, (name, label, got_wg, want_wg)
        assert got_dg == want_dg, (name, label, got_dg, want_dg)
        if head_dx is False:
            assert "conv1x1_sigmoid_bwd_masked" not in names, (name, label)
            assert all(not c["args"]["need_dx"] for c in got["bwd"] if c["name"] == "conv1x1_sigmoid_bwd"), (name, label)
        # the bar sees a defect: one dropped chunk of 16 pixels of each weight / bias reduction is >= 10 x the bar
        if label == "control":
            for cname, m, x, dy in ref64["taps"]:
                rows, per_pixel = R.dropped_chunk_rows(m, x, dy)
                for t, d in ((f"{cname}.weight", chunk_defect(rows, 1, ref64["grads"][f"{cname}.weight"].reshape(-1))),
                             (f"{cname}.bias", None if m.bias is None or f"{cname}.bias" in zero else
                              chunk_defect(per_pixel, R.UNIT, ref64["grads"][f"{cname}.bias"]))):
                    if d is not None and t in on:
                        bar = max(20 * rel(ref32["grads"][t], ref64["grads"][t]), 2e-4)
                        assert d > 10 * bar, (name, t, d, bar)
    print(f"{name} (seed {seed}) control vs fp64: " + ", ".join(lines))
    print(f"{name}: worst gradient over all subsets, as a share of its bar: {worst[0]:.2f} ({worst[1]})")
    assert not problems, "\n".join([name] + problems)


# ================================================================================================ B. the default SP step
SP_LR = 1e-4


def _trained(model):
    return list(model.fusion.parameters()) + list(model.bn.parameters()) + list(model.decoder.parameters())


def _is_encoder(k):
    return k.startswith(("features_s.", "features_t."))


def _sp_step(seed, frozen, rec):
    """One SP.trainSP iteration on the seeded 3 x 32 x 32 batch, encoders frozen as SP.py:72-81 or everything trainable."""
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    model, sd0 = build_model()
    if frozen:
        for p in list(model.features_s.parameters()) + list(model.features_t.parameters()):
            p.requires_grad = False
    opt = FusedAdam(_trained(model) if frozen else model.parameters(), lr=SP_LR)
    model.train()
    crit = floss().to(DEV)
    x_s, x_t, gt, _ = synth.synth_sp_batch(3, 32, seed=seed)
    opt.zero_grad()
    rec.take()
    rec.active = True
    out = model(x_s.to(DEV), x_t.to(DEV))
    loss = crit(out, gt.to(DEV).view(out.size()))
    torch.cuda.synchronize()
    rec.take()
    loss.backward()
    torch.cuda.synchronize()
    rec.active = False
    bwd = [(c["name"], tuple(c["args"]["dy"].shape) if "dy" in c["args"] else None) for c in rec.take()]
    named = dict(model.named_parameters())
    res = dict(out=out.detach().clone(), loss=loss.detach().clone(), bwd=bwd,
               grads={k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items()},
               before={k: p.detach().clone() for k, p in named.items()})
    lo, hi = opt.flat_p.data_ptr(), opt.flat_p.data_ptr() + 4 * opt.flat_p.numel()
    res["slots"] = {k: (any(p is q for q in opt.params), lo <= p.data_ptr() < hi, hasattr(p, "_egz_sink")) for k, p in named.items()}
    opt.step()
    torch.cuda.synchronize()
    res["after"] = {k: p.detach().clone() for k, p in named.items()}
    res["buffers"] = {k: v.detach().clone() for k, v in model.named_buffers()}
    res["buffers0"] = {k: sd0[k] for k in res["buffers"]}
    return res


@pytest.fixture(scope="module")
def sp_default():
    import egaze_amd.hipops as H
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(H, "SPLITK", False)             # the summation order GRAD_SEEDS were characterised with
        rec = RouteRecorder(mp)
        rec.active = False
        runs = {seed: {"all": _sp_step(seed, False, rec), "frozen": _sp_step(seed, True, rec)} for seed in GRAD_SEEDS}
    finally:
        mp.undo()
    yield runs
    torch.cuda.empty_cache()


def test_sp_default_same_forward_and_gradients_as_all_trainable(sp_default):
    """B.1: output, loss and the gradient of every fusion / bn / decoder parameter carry the all-trainable run's bits (their
    backward launches do not depend on what lies below)."""
    for seed, r in sp_default.items():
        a, f = r["all"], r["frozen"]
        assert torch.equal(a["out"], f["out"]) and torch.equal(a["loss"], f["loss"]), seed
        checked = 0
        for k, g in f["grads"].items():
            if not _is_encoder(k):
                assert g is not None and torch.equal(g, a["grads"][k]), (seed, k)
                checked += 1
        assert checked == 2 + 2 + 26


def test_sp_default_gradients_vs_fp64(sp_default):
    """B.2: the criteria of test_hip_model_sp._grads_vs_fp64 on the trained tensors of the frozen-encoder step, against the
    cached fp64 oracle gradients (the gradient of a decoder weight does not depend on whether the encoder leaves require one):
    every seed cosine >= 0.995 and norm within 3 %; tight -- median error within max(20 x CPU fp32, 2e-4), every tensor with
    98 % of its entries within 2e-3 of max |ref| -- on at least two of the three seeds.

    Observed on MI355X (29 tensors per seed; tight on all three seeds):
      seed 4  HIP vs fp64: median 1.76e-06 max 1.47e-05 | CPU fp32 vs fp64: median 4.43e-05 max 1.64e-04
      seed 5  HIP vs fp64: median 4.87e-05 max 1.50e-04 | CPU fp32 vs fp64: median 7.35e-07 max 9.94e-06
      seed 6  HIP vs fp64: median 2.32e-06 max 2.08e-05 | CPU fp32 vs fp64: median 9.19e-07 max 9.70e-06"""
    results = []
    for seed, r in sp_default.items():
        out32, g32, out64, g64 = _small_oracle_pair(seed)
        e_hip, e_cpu = rel(r["frozen"]["out"], out64), rel(out32, out64)
        assert e_hip < max(5 * e_cpu, 2e-6), (seed, e_hip, e_cpu)
        errs, tight = {}, True
        for k, g in r["frozen"]["grads"].items():
            if _is_encoder(k) or g64[k].abs().max().item() < 1e-9:
                continue
            errs[k] = (rel(g, g64[k]), rel(g32[k], g64[k]))
            c, rn = cos_norm(g.cpu().numpy(), g64[k].numpy())
            assert c >= 0.995 and abs(rn - 1) <= 0.03, (seed, k, c, rn)
            tight = tight and mostly_close(g.cpu().numpy(), g64[k].numpy())[0]
        assert len(errs) == 29                    # fusion.weight, bn.*, decoder.* (fusion.bias is zero identically)
        eh, ec = np.array([v[0] for v in errs.values()]), np.array([v[1] for v in errs.values()])
        print("seed %d frozen encoders, HIP vs fp64: median %.2e max %.2e | CPU fp32 vs fp64: median %.2e max %.2e" %
              (seed, np.median(eh), eh.max(), np.median(ec), ec.max()))
        results.append((seed, bool(tight and np.median(eh) < max(20 * np.median(ec), 2e-4))))
    print("frozen encoders, tight on seeds", [s for s, ok in results if ok])
    assert sum(ok for _, ok in results) >= 2, results


def test_sp_default_encoder_untouched_statistics_moved(sp_default):
    """B.3 and B.5: frozen weights, train-mode BatchNorm -- the reference's semantics -- and the same parameters after step()."""
    for seed, r in sp_default.items():
        a, f = r["all"], r["frozen"]
        n_enc = 0
        for k, g in f["grads"].items():
            in_opt, in_flat, has_sink = f["slots"][k]
            if _is_encoder(k):
                n_enc += 1
                assert g is None, (seed, k)
                assert torch.equal(f["after"][k], f["before"][k]), (seed, k)
                assert not in_opt and not in_flat and not has_sink, (seed, k)
            else:
                assert in_opt and in_flat and has_sink, (seed, k)
                assert torch.equal(f["after"][k], a["after"][k]), (seed, k)                  # B.5
                assert not torch.equal(f["after"][k], f["before"][k]) or k == "fusion.bias", (seed, k)
        assert n_enc == 2 * 13 * 4
        moved = 0
        for k, v in f["buffers"].items():
            assert torch.equal(v, a["buffers"][k]), (seed, k)
            if _is_encoder(k):
                moved += 1
                assert not torch.equal(v.cpu(), f["buffers0"][k]), (seed, k)
                if k.endswith("num_batches_tracked"):
                    assert int(v) == int(f["buffers0"][k]) + 1, (seed, k)
        assert moved == 2 * 13 * 3


def test_sp_default_skipped_launches(sp_default):
    """B.4: the backward pass of the frozen-encoder step holds the decoder's twelve weight and data gradients, the fusion
    conv's weight gradient (on the depth-2 stack: batch 6) and ONE BatchNorm backward -- no encoder launch, no data gradient of
    the fusion conv.  The all-trainable step next to it shows what the recorder sees when they do run."""
    for seed, r in sp_default.items():
        f, a = r["frozen"]["bwd"], r["all"]["bwd"]
        count = lambda calls, names: sum(n in names for n, _ in calls)
        assert count(f, WGRAD) == 13 and count(f, ("conv3x3_wgrad",)) == 13, [c for c in f if c[0] in WGRAD]
        assert sum(n == "conv3x3_wgrad" and s[0] == 6 for n, s in f) == 1
        assert count(f, DGRAD) == 12 and not any(n in DGRAD and s[0] == 6 for n, s in f), [c for c in f if c[0] in DGRAD]
        assert count(f, ("bn_relu_pool_bwd",)) == 1
        assert count(a, WGRAD) == 13 + 26 and count(a, DGRAD) == 12 + 1 + 24
        assert sum(n in DGRAD and s[0] == 6 for n, s in a) == 1


class _Frames(torch.utils.data.Dataset):
    """test_hip_drivers._SPData, loaded in the test's own process, with the order the samples were asked for."""
    loader_workers = 0

    def __init__(self, n, size, seed):
        self.im, self.fl, self.gt, self.fs = synth.synth_sp_batch(n, size, seed=seed)
        self.asked = []

    def __len__(self):
        return self.im.shape[0]

    def __getitem__(self, i):
        self.asked.append(int(i))
        return {'image': self.im[i], 'flow': self.fl[i], 'gt': self.gt[i], 'fixsac': self.fs[i], 'imname': 'frame_%05d.jpg' % i}


def test_sp_driver_default_mode_equals_the_steps_by_hand(tmp_path):
    """B.6: SP(resume=1) -- the mode a user gets without flags -- for one epoch over two batches of 2 x 32 x 32 ends with the
    parameters of the same two steps issued by hand on a copy of its model with the freeze and the parameter list B assumes."""
    from egaze_amd.SP import SP
    from egaze_amd.floss import floss
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import cfg, make_layers, owned_state_dict
    torch.save({'state_dict': {}}, str(tmp_path / "s.pth"))
    data = _Frames(4, 32, 0)
    sp = SP(lr=SP_LR, save_path=str(tmp_path / "save"), save_name='frozen_SP.pth.tar', num_epoch=1, batch_size=2, device='0',
            resume=1, pretrained_spatial=str(tmp_path / "s.pth"), pretrained_temporal=str(tmp_path / "s.pth"),
            traindata=data, valdata=_Frames(2, 32, 1))
    sd0 = owned_state_dict(sp.model)
    sp.train()
    assert sorted(data.asked) == [0, 1, 2, 3]
    hand = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    hand.load_state_dict(sd0)
    hand.to(DEV)
    for p in list(hand.features_s.parameters()) + list(hand.features_t.parameters()):
        p.requires_grad = False
    opt = FusedAdam(_trained(hand), lr=SP_LR)
    crit = floss().to(DEV)
    hand.train()
    for idx in (data.asked[:2], data.asked[2:]):
        opt.zero_grad()
        out = hand(data.im[idx].float().to(DEV), data.fl[idx].float().to(DEV))
        crit(out, data.gt[idx].float().to(DEV).view(out.size())).backward()
        opt.step()
    torch.cuda.synchronize()
    got, want = sp.model.state_dict(), hand.state_dict()
    assert [p.requires_grad for p in sp.model.parameters()] == [p.requires_grad for p in hand.parameters()]
    assert len(sp.optimizer.params) == len(opt.params) and sp.optimizer.step_count == 2
    for k, v in want.items():
        assert torch.equal(got[k], v), k
        if not _is_encoder(k) and k != "fusion.bias" and v.is_floating_point():
            assert not torch.equal(v.cpu(), sd0[k].cpu()), k


# ================================================================================================ C. gradient sinks
class _SPNet:
    no_sink = {"features_t.0.weight"}      # the channel-padded flow conv returns its gradient to autograd (functions.py, `padded`)

    def build(self):
        return build_model()[0].train()

    def batches(self):
        return [tuple(t.to(DEV) for t in synth.synth_sp_batch(3, 32, seed=s)[:3]) for s in GRAD_SEEDS[:2]]

    def backward(self, model, batch):
        from egaze_amd.floss import floss
        out = model(batch[0], batch[1])
        floss().to(DEV)(out, batch[2].view(out.size())).backward()


class _LFNet:
    no_sink = set()

    def build(self):
        from test_hip_lf import build
        return build().train()

    def batches(self):
        g = torch.Generator().manual_seed(21)
        return [tuple(torch.rand(2, 1, 32, 32, generator=g).to(DEV) for _ in range(3)) for _ in range(2)]

    def backward(self, model, batch):
        from egaze_amd.floss import floss
        floss().to(DEV)(model(batch[0], batch[1]), batch[2]).backward()


class _LSTMNet:
    no_sink = set()
    T, B = 3, 2

    def build(self):
        from test_hip_at import build
        return build().train()

    def batches(self):
        g = torch.Generator().manual_seed(5 + self.T)
        return [tuple(t.to(DEV) for t in (torch.randn(self.T, self.B, 512, generator=g),
                                          torch.tanh(torch.randn(self.T, self.B, 512, generator=g)),
                                          0.1 * torch.randn(2, self.B, 512, generator=g),
                                          0.1 * torch.randn(2, self.B, 512, generator=g))) for _ in range(2)]

    def backward(self, model, batch):
        from egaze_amd.functions import MSELoss
        pred, _ = model(batch[0], (batch[2], batch[3]))
        MSELoss.apply(pred, batch[1]).backward()


class _LSTMSample(_LSTMNet):
    """The single-sample step (T = 1, B = 1: csrc/lstm_b1.hip) AT.py takes with ``zero_grad(all_overwritten=True)``."""
    T, B = 1, 1


NETS = {"sp": _SPNet, "late_fusion": _LFNet, "lstm_T3_B2": _LSTMNet, "lstm_sample": _LSTMSample}


def _watch(named):
    """A tensor hook per parameter -> {name: [what each fused node handed autograd for it: True = a gradient tensor, which
    AccumulateGrad adds to p.grad; False = None, the kernel wrote p.grad through the sink and no add is issued]}."""
    seen = {k: [] for k in named}
    for k, p in named.items():
        p.register_hook(lambda g, k=k: seen[k].append(g is not None))
    return seen


def _views_ok(opt):
    return all(p.grad is not None and p.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * o for p, o in zip(opt.params, opt.offsets))


@pytest.mark.parametrize("net", list(NETS))
def test_sink_routes_give_one_result(net, monkeypatch):
    """C.1: the same backward with sinks attached, with hipops.DIRECT_GRADS = False and with no optimizer leaves the same bits
    in every p.grad.  With sinks, every parameter's gradient was written in place in this zero_grad generation and no
    AccumulateGrad ran for it (the one deliberate exception: _SPNet.no_sink)."""
    import egaze_amd.hipops as H
    from egaze_amd.optim import FusedAdam
    n = NETS[net]()
    batch = n.batches()[0]
    res = {}
    for route in ("sinks", "autograd", "no optimizer"):
        with monkeypatch.context() as m:
            m.setattr(H, "DIRECT_GRADS", route == "sinks")
            model = n.build()
            opt = FusedAdam(model.parameters(), lr=1e-4) if route != "no optimizer" else None
            if opt is not None:
                opt.zero_grad()
            named = dict(model.named_parameters())
            seen = _watch(named)
            n.backward(model, batch)
            torch.cuda.synchronize()
            if route == "sinks":
                assert seen == {k: [k in n.no_sink] for k in named}, {k: v for k, v in seen.items() if v != [False]}
                for k, p in named.items():
                    assert (p._egz_sink.gen_written == opt.zero_gen) == (k not in n.no_sink), k
            else:
                assert seen == {k: [True] for k in named}, {k: v for k, v in seen.items() if v != [True]}
            if opt is not None:
                assert _views_ok(opt)
            res[route] = {k: p.grad.detach().clone() for k, p in named.items()}
    for k, g in res["sinks"].items():
        assert g.abs().max().item() > 0 or k.endswith(".bias"), k
        assert torch.equal(g, res["autograd"][k]), (net, k, "sinks vs DIRECT_GRADS = False")
        assert torch.equal(g, res["no optimizer"][k]), (net, k, "sinks vs no optimizer")


@pytest.mark.parametrize("net", list(NETS))
def test_sink_second_backward_accumulates(net):
    """C.2: zero_grad(), backward on batch a, backward on batch b: the flat gradient buffer holds g_a + g_b (one fp32 add on
    the device of the gradients of two separately zeroed passes) bit for bit -- the first pass writes in place, the second
    finds the sinks taken and goes through AccumulateGrad."""
    from egaze_amd.optim import FusedAdam
    n = NETS[net]()
    model = n.build()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    a, b = n.batches()
    single = []
    for batch in (a, b):
        opt.zero_grad()
        n.backward(model, batch)
        single.append(opt.flat_g.clone())
    assert not torch.equal(single[0], single[1])
    opt.zero_grad()
    n.backward(model, a)
    n.backward(model, b)
    got = opt.flat_g.clone()
    torch.cuda.synchronize()
    assert _views_ok(opt)
    assert torch.equal(got, single[0] + single[1]), (net, rel(got, single[0] + single[1]))


@pytest.mark.parametrize("mode", ["none", "late_helper", "late_waiter"])
def test_sink_one_weight_two_uses_in_one_graph(mode):
    """C.3: the decoder tail of part A applied to two inputs, the two losses summed, one backward().  The first node autograd
    reaches takes the sink and leaves its weight gradient running on the detached helper stream; the second use goes through
    AccumulateGrad, whose add must be ordered behind that stream -- under injected delays, read right where backward() returns.
    The result is the sum of the two single-use gradients (one fp32 add)."""
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import FusedSequential
    case, seed = R.CASES["tail"], R.SEEDS["tail"]
    ref_net, inputs = R.make(case, seed)
    net = FusedSequential(*ref_net.children()).to(DEV).train()
    opt = FusedAdam(net.parameters(), lr=1e-4)
    named = dict(net.named_parameters())
    seen = _watch(named)
    xs = [inputs["x"].to(DEV), R.make(case, seed + 1)[1]["x"].to(DEV)]
    ds = [R.upstream(case, seed + i, (2, 1, 16, 16)).to(DEV) for i in range(2)]

    def loss(i):
        return (net(xs[i].clone().requires_grad_(), fuse_sigmoid=True) * ds[i]).sum()

    before = STATS["delays"]
    with perturb(mode, DELAY_MS):
        single = []
        for i in range(2):
            opt.zero_grad()
            loss(i).backward()
            single.append(opt.flat_g.clone())              # (no host wait between backward() and the read)
        assert seen == {k: [False, False] for k in named}, seen
        opt.zero_grad()
        (loss(0) + loss(1)).backward()
        got = opt.flat_g.clone()
        torch.cuda.synchronize()
    assert (STATS["delays"] - before > 0) == (mode != "none")
    # every parameter: written in place by the use autograd reached first, ONE AccumulateGrad add for the other use
    # (autograd sums what the two uses return before the leaf sees it: None from the use it reached first, which wrote the sink,
    # plus the other use's tensor -- ONE AccumulateGrad add per parameter)
    assert seen == {k: [False, False, True] for k in named}, seen
    assert all(p._egz_sink.gen_written == opt.zero_gen for p in named.values())
    assert _views_ok(opt) and not torch.equal(single[0], single[1])
    assert torch.equal(got, single[0] + single[1]), (mode, rel(got, single[0] + single[1]))


def test_sink_all_overwritten_single_sample_step():
    """C.4: the single-sample AT step with ``zero_grad(all_overwritten=True)`` over a flat gradient buffer full of a sentinel:
    every element that belongs to a parameter was overwritten, with the bits of the ordinary zero-filled step."""
    from egaze_amd.optim import FusedAdam
    n = _LSTMSample()
    model = n.build()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    batch = n.batches()[0]
    opt.zero_grad()
    n.backward(model, batch)
    want = opt.flat_g.clone()
    sentinel = 7.25e7
    opt.flat_g.fill_(sentinel)
    opt.zero_grad(all_overwritten=True)
    n.backward(model, batch)
    got = opt.flat_g.clone()
    torch.cuda.synchronize()
    assert _views_ok(opt)
    owned = torch.zeros(opt.numel, dtype=torch.bool, device=DEV)
    for p, o in zip(opt.params, opt.offsets):
        owned[o:o + p.numel()] = True
        assert p._egz_sink.gen_written == opt.zero_gen
    assert int((got[owned] == sentinel).sum()) == 0
    assert bool((got[~owned] == sentinel).all())              # (alignment padding between slots: nobody's to write)
    assert torch.equal(got[owned], want[owned])
