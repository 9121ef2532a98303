"""Float64 / float32 CPU references of the fused blocks for tests/test_hip_frozen_routes.py: the same stock ``nn`` modules the
fused autograd nodes stand for (train-mode BatchNorm, nearest upsample, MaxPool2d, Conv3d + MaxPool3d over the stream pair),
run through torch's own autograd with a given ``requires_grad`` pattern.

A case is a list of stock modules plus its inputs.  ``things(case)`` names everything that can need a gradient: the inputs
first, then the parameters by their ``nn.Sequential`` names.  ``run(case, dtype, on)`` runs forward and backward with
exactly the things in ``on`` requiring a gradient and returns the output, the gradients, the BatchNorm statistics, the
flip margin of the forward pass and, per convolution, the operands of its weight and bias gradient (for the
dropped-chunk defects).

Flip margin.  A ReLU or max decision taken within rounding distance of a tie makes a correct fp32 kernel disagree with fp64 by
O(1) of one entry.  ``margin`` is the smallest distance from a tie over every decision of the forward pass, relative to
max |value| of the tensor the decision is taken on: |z| of every pre-ReLU value, the gap between the two largest entries of
every pooling window (windows that are entirely ReLU-dead aside: their gradient is zero whichever zero is taken) and of
every stream pair.  SEEDS holds, per case, the first generator seed whose fp64 forward keeps
that margin above MARGIN (``python tests/frozen_ref.py`` repeats the search on the CPU; the tests assert the condition).
"""
import collections

import torch
import torch.nn as nn

MARGIN = 2e-5          # 10 x the 2e-6 forward bar test_conv3x3_split_half holds the f16x3 route to
UNIT = 16              # pixels per dropped chunk (chunk_defect)
LATE_WINDOW = 12       # side of the textured window of a late-fusion input map


def _cbr(cin, cout, pool=False):
    return [nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU()] + ([nn.MaxPool2d(2, 2)] if pool else [])


def _cr(cin, cout, bias=True):
    return [nn.Conv2d(cin, cout, 3, padding=1, bias=bias), nn.ReLU()]


def _tail(mid, bias=True):
    return [nn.Upsample(scale_factor=2)] + _cr(128, 64, bias) + _cr(64, mid, bias) + [nn.Conv2d(mid, 1, 1, bias=bias)]


def _late():
    return _cbr(2, 32) + _cbr(32, 32) + _cbr(32, 8) + [nn.Conv2d(8, 1, 1)]


Case = collections.namedtuple("Case", "name kind layers inputs first head")
# kind "seq": a FusedSequential of the layers; "late": models.late_fusion (its two maps are the channels of the one input);
# "fusion_halves" / "fusion_stack2": functions.FusionBlock on the halves of one buffer / on two separate tensors.
# first: the block reads the network input (no gradient into it: NotImplementedError).  head: ends in Conv1x1 -> Sigmoid.
CASES = collections.OrderedDict((c.name, c) for c in [
    Case("cbr", "seq", lambda: _cbr(64, 64), {"x": (2, 64, 8, 8)}, False, False),
    Case("cbr_pool", "seq", lambda: _cbr(64, 64, pool=True), {"x": (2, 64, 8, 8)}, False, False),
    Case("cbr_chain", "seq", lambda: _cbr(64, 64) + _cbr(64, 64), {"x": (2, 64, 8, 8)}, False, False),
    Case("first_rgb", "seq", lambda: _cbr(3, 64), {"x": (2, 3, 8, 8)}, True, False),
    Case("first_flow", "seq", lambda: _cbr(20, 64), {"x": (2, 20, 8, 8)}, True, False),
    Case("first_lf", "seq", lambda: _cbr(2, 32), {"x": (2, 2, 8, 8)}, True, False),
    Case("late_fusion", "late", _late, {"x": (2, 2, 32, 32)}, True, True),
    Case("tail", "seq", lambda: _tail(64), {"x": (2, 128, 8, 8)}, False, True),
    Case("tail_head8", "seq", lambda: _tail(8), {"x": (2, 128, 8, 8)}, False, True),
    Case("tail_nobias", "seq", lambda: _tail(64, bias=False), {"x": (2, 128, 8, 8)}, False, True),
    Case("cr", "seq", lambda: _cr(64, 64), {"x": (2, 64, 8, 8)}, False, False),
    Case("cr_nobias", "seq", lambda: _cr(64, 64, bias=False), {"x": (2, 64, 8, 8)}, False, False),
    Case("fusion_halves", "fusion_halves", None, {"fs": (2, 512, 4, 4), "ft": (2, 512, 4, 4)}, False, False),
    Case("fusion_stack2", "fusion_stack2", None, {"fs": (2, 512, 4, 4), "ft": (2, 512, 4, 4)}, False, False),
])

# first seed (0, 1, 2, ...) whose fp64 forward is flip-free: find_seed() below, run on the CPU with this file alone
SEEDS = {"cbr": 0, "cbr_pool": 0, "cbr_chain": 10, "first_rgb": 4, "first_flow": 0, "first_lf": 0, "late_fusion": 108, "tail": 155,
         "tail_head8": 2, "tail_nobias": 96, "fusion_halves": 31, "fusion_stack2": 31, "cr": 0, "cr_nobias": 0}


class FusionRef(nn.Module):
    """models/model_SP.py:33-47 of the reference: Conv3d (1,3,3) over the depth-2 stack -> MaxPool3d((2,1,1)) -> BN -> ReLU."""

    def __init__(self):
        super().__init__()
        self.fusion = nn.Conv3d(512, 512, kernel_size=(1, 3, 3), padding=(0, 1, 1))
        self.pool3d = nn.MaxPool3d(kernel_size=(2, 1, 1), padding=0)
        self.bn = nn.BatchNorm2d(512)
        self.relu = nn.ReLU()

    def forward(self, fs, ft):
        x = torch.cat((fs.unsqueeze(2), ft.unsqueeze(2)), 2)
        return self.relu(self.bn(self.pool3d(self.fusion(x)).squeeze(2)))


def make(case, seed):
    """The case's module (fp32, CPU, train mode) and inputs from one seeded generator: convolutions He-scaled so that
    activations stay O(1), biases and betas O(0.1), every third gamma negative."""
    g = torch.Generator().manual_seed(1000 * seed + 17)
    net = FusionRef() if case.layers is None else nn.Sequential(*case.layers())
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                fan_in = m.in_channels * m.kernel_size[-1] * m.kernel_size[-2]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                K = m.num_features
                m.weight.copy_((0.5 + torch.rand(K, generator=g)) * torch.where(torch.arange(K) % 3 == 1, -1.0, 1.0))
                m.bias.copy_(torch.randn(K, generator=g) * 0.3)
    net.train()
    inputs = collections.OrderedDict((k, torch.randn(shape, generator=g)) for k, shape in case.inputs.items())
    if case.kind == "late":
        # the maps late fusion is fed (data/lateDataset.py: a prediction and an attention map): a flat level with one textured
        # window each.  Besides being what the net sees, flat regions repeat ONE pre-ReLU value per channel, which is what lets
        # a 2 x 32 x 32 input through three ReLU layers (147456 decisions) clear the flip margin at all
        x = inputs["x"]
        for b in range(x.shape[0]):
            for c in range(x.shape[1]):
                r0, c0 = (int(v) for v in torch.randint(0, x.shape[2] - LATE_WINDOW + 1, (2,), generator=g))
                x[b, c] = torch.rand((), generator=g)
                x[b, c, r0:r0 + LATE_WINDOW, c0:c0 + LATE_WINDOW] = torch.rand((LATE_WINDOW, LATE_WINDOW), generator=g)
    return net, inputs


def upstream(case, seed, shape):
    """The fixed random gradient fed in at the output."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 * seed + 29))


_THINGS = {}


def things(case):
    if case.name not in _THINGS:
        net, inputs = make(case, 0)
        _THINGS[case.name] = list(inputs) + [k for k, _ in net.named_parameters()]
    return list(_THINGS[case.name])


def zero_bias(case):
    """Conv biases in front of a train-mode BatchNorm: the loss does not depend on them (BN subtracts the batch mean), their
    gradient is zero identically.  The fused nodes return exact zeros (functions._zero_bias_grad); fp64 autograd returns the
    round-off of a sum that cancels."""
    net, _ = make(case, 0)
    if isinstance(net, FusionRef):
        return {"fusion.bias"}
    mods = list(net.named_children())
    return {f"{n}.bias" for (n, m), (_, nx) in zip(mods, mods[1:]) if isinstance(m, nn.Conv2d) and isinstance(nx, nn.BatchNorm2d)
            and m.bias is not None}


def forward(case, net, inputs):
    if isinstance(net, FusionRef):
        return net(inputs["fs"], inputs["ft"])
    out = net(inputs["x"])
    return torch.sigmoid(out) if case.head else out


def _gap2(v):
    """Smallest gap between the two largest entries along the last dim."""
    top = v.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]).min().item()


def run(case, seed, dtype, on, taps=False):
    """Forward + backward of the stock modules in ``dtype`` on the CPU; exactly the things in ``on`` require a gradient.
    -> dict(out, dout, grads {thing: tensor or None}, stats {buffer name: tensor}, margin, taps)."""
    net, inputs = make(case, seed)
    net = net.to(dtype)
    inputs = collections.OrderedDict((k, v.to(dtype).requires_grad_(k in on)) for k, v in inputs.items())
    for k, p in net.named_parameters():
        p.requires_grad_(k in on)
    margins, tapped, hooks = [], [], []

    def relu_pre(m, args):
        z = args[0].detach()
        margins.append(z.abs().min().item() / z.abs().max().item())

    def pool2_pre(m, args):
        z = args[0].detach()
        win = z.unfold(2, 2, 2).unfold(3, 2, 2).flatten(-2)
        # (the pool follows the ReLU: a window whose maximum is exactly 0 is ReLU-dead in every implementation, and whichever of
        # its zeros the pool takes, the ReLU backward behind it returns 0 -- no decision to flip)
        win = win[win.max(-1).values > 0]
        margins.append(_gap2(win) / z.abs().max().item())

    def pool3_pre(m, args):
        z = args[0].detach()                       # (B, K, 2, h, w): the stream pair
        margins.append((z[:, :, 0] - z[:, :, 1]).abs().min().item() / z.abs().max().item())

    def conv_tap(name):
        def hook(m, args, out):
            if out.requires_grad:
                out.retain_grad()
            tapped.append((name, m, args[0].detach(), out))
        return hook

    for name, m in net.named_modules():
        if isinstance(m, nn.ReLU):
            hooks.append(m.register_forward_pre_hook(relu_pre))
        elif isinstance(m, nn.MaxPool2d):
            hooks.append(m.register_forward_pre_hook(pool2_pre))
        elif isinstance(m, nn.MaxPool3d):
            hooks.append(m.register_forward_pre_hook(pool3_pre))
        elif taps and isinstance(m, (nn.Conv2d, nn.Conv3d)):
            hooks.append(m.register_forward_hook(conv_tap(name)))
    out = forward(case, net, inputs)
    for h in hooks:
        h.remove()
    dout = upstream(case, seed, out.shape)
    if out.requires_grad:
        out.backward(dout.to(dtype))
    grads = {k: v.grad for k, v in inputs.items()}
    grads.update({k: p.grad for k, p in net.named_parameters()})
    stats = {k: v.detach().clone() for k, v in net.named_buffers()}
    res = dict(out=out.detach(), dout=dout, grads=grads, stats=stats, margin=min(margins), taps=[])
    for name, m, x, y in tapped:
        if y.grad is None:
            continue
        dy = y.grad
        if isinstance(m, nn.Conv3d):               # the depth-2 stack folded into the batch dim, as the kernels see it
            x = x.permute(2, 0, 1, 3, 4).flatten(0, 1)
            dy = dy.permute(2, 0, 1, 3, 4).flatten(0, 1)
        res["taps"].append((name, m, x, dy))
    return res


def dropped_chunk_rows(m, x, dy):
    """What ONE chunk of UNIT consecutive output pixels (NHWC order) contributes to the weight gradient of conv ``m``: the
    first, a middle and the last chunk, as rows of a (3, K*C*kh*kw) matrix -- chunk_defect(rows, 1, ref) takes the smallest.
    -> (rows for the weight, per-pixel contributions (pixels, K) for the bias)."""
    B, K, Hh, Ww = dy.shape
    n = B * Hh * Ww
    kh = m.kernel_size[-1]
    shape = (K, x.shape[1], kh, kh)
    rows = []
    for s in sorted({0, (n // 2) // UNIT * UNIT, (n - UNIT) // UNIT * UNIT}):
        mask = torch.zeros(n, dtype=dy.dtype)
        mask[s:s + UNIT] = 1
        rows.append(torch.nn.grad.conv2d_weight(x, shape, dy * mask.view(B, 1, Hh, Ww), padding=kh // 2).reshape(-1))
    return torch.stack(rows), dy.permute(0, 2, 3, 1).reshape(n, K)


def subsets(case):
    """(label, set of things on, refused) for every subset the tests run.  ``refused``: the code raises NotImplementedError
    by design (a gradient into the network input of a first block)."""
    th = things(case)
    ins, params = [t for t in th if t in case.inputs], [t for t in th if t not in case.inputs]
    out = [("all", set(th)), ("input only", set(ins)), ("params only", set(params))]
    out += [(f"all but {t}", set(th) - {t}) for t in th]
    out += [(f"only {t}", {t}) for t in th]
    if case.first:          # the valid single-freeze patterns of a first block: the parameters without one, the input off
        out += [(f"params but {t}", set(params) - {t}) for t in params]
    seen, res = [], []
    for label, on in out:
        if on and on not in seen:
            seen.append(on)
            res.append((label, on, bool(case.first and on & set(ins))))
    return res


def control(case):
    th = things(case)
    return set(t for t in th if not (case.first and t in case.inputs))


def find_seed(case, limit=200000):
    for seed in range(limit):
        m = run(case, seed, torch.float64, set())["margin"]          # (nothing requires a gradient: the forward pass alone)
        if m >= MARGIN:
            return seed, m
    raise RuntimeError(f"{case.name}: no flip-free seed below {limit}")


if __name__ == "__main__":
    import sys
    torch.set_num_threads(4)
    for name in sys.argv[1:] or list(CASES):
        print(name, *find_seed(CASES[name]), flush=True)
