"""Every host-side cache of derived weights against every way a tensor can change.

No convolution reads an nn.Parameter: it reads a packed copy (hipops.packing._PACKED, eight kinds x three dtype codes), a
BatchNorm-folded weight (``weight._egz_fold``), eval-mode BatchNorm rows (``running_mean._egz_evalcoef``), an abs-max scalar an
activation carries (``_egz_absmax``), or packings baked into a captured hipGraph (graphs.GraphedModule / GraphedTrainStep).  A
stale copy raises nothing and returns plausible numbers.  Each case here runs one launch to fill the cache, changes the values by
one route, and runs the launch again.

One oracle throughout: torch.nn.functional on the CPU in fp64, from the parameter values as they are when the launch is issued.
A launch passes when max|got - ref| / max|ref| is within the bar tests/test_hip_ops.py sets for that arithmetic: f16 x3 2e-6,
bf16 x3 3e-5, exact f32 1e-5, an eval-mode [conv -> BatchNorm -> ReLU] block 1e-5 (test_bn_relu_pool's bar for the BatchNorm
pass, test_eval_batchnorm_folded_into_conv's for the fold).  Every mutation replaces the values by an independent draw of the
same scale (the optimizer routes: by a step of twice the weights' standard deviation with random signs -- the first Adam step
moves every element by lr), so a stale copy is off by O(1); each case asserts that the references before and after differ by
more than 0.1 of max|ref| -- the test's own power.

The routes (tests/test_cache_tags_host.py pins what each does to torch's version counter):
  adam-batch / adam-lazy   FusedAdam.step(): raw-pointer write through the flat buffer + touch_params + refresh_packings,
                           hipops.BATCH_REPACK on / off
  sgd                      torch.optim.SGD.step()
  copy_                    with torch.no_grad(): p.copy_(new)
  load_state_dict          module.load_state_dict(sd)
  assign                   module.load_state_dict(sd, assign=True): a new Parameter object
  state_dict-write         module.state_dict()[k].copy_(new)
  data-assign              p.data = new_tensor
  data+touch / data+bump   p.data.copy_(new), declared with hipops.touch_params([p]) / hipops.bump_weight_epoch() -- the
                           contract of INTEGRATION.md ("Writes behind torch's back"); the undeclared write is not tested
  init_like_reference      utils.init_like_reference(module) on a module that has already run
  second-adam              a second FusedAdam over the same parameter (re-homed into a new flat buffer), then its step

Left out: the undeclared ``.data`` write (by design there is no content fingerprint).  Elsewhere: the device-side writes of a
REPLAYED GraphedTrainStep as a route into the eval caches (replay, eval, replay, eval on one step object; the step object declares
them after every replay, hipops.note_replay) are walked by tests/test_hip_graph_replay.py.  The values of a further replay of a
re-captured GraphedModule are compared bit for bit with the eager forward in test_graphed_module_replay_follows below (every
route, both precisions) and with the first replay in test_hip_graph_replay.py (second and third replay after a re-capture that a
replayed training step caused).  (An earlier version of this paragraph recorded a second replay 2.7e-7 = 2^-22 of max|ref| off
the first, cause not found.  The same step of one f16 x3 scale showed in test_hip_graph_replay.py in replays that follow eager
launches, in about half the runs, and went away with the standalone abs-max pass zero-filling its buffer by a kernel instead of
a captured hipMemsetAsync: csrc/bn_pool.hip, egz_absmax.)
"""
import contextlib
import functools
import gc

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {0: 1e-5, 1: 2e-6, 2: 3e-5}            # dtype code -> the bar of test_hip_ops.py (exact f32, f16 x3, bf16 x3)
TOL_BLOCK = 1e-5                             # eval [conv -> BN -> ReLU] block, folded or not
POWER = 0.1
PACK_LAUNCHES = ("egz_pack_w3x3_fwd", "egz_pack_w3x3_dgrad", "egz_pack_w3x3_ups_fwd", "egz_pack_w3x3_ups_dgrad",
                 "egz_pack_w3x3_split", "egz_pack_w3x3_split_frag", "egz_pack_w3x3_frag_batch")


def H():
    import egaze_amd.hipops as h
    return h


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def _precision(monkeypatch, precision, grad_split="f16"):
    h = H()
    monkeypatch.setattr(h, "PRECISION", precision)
    monkeypatch.setattr(h, "GRAD_SPLIT", grad_split)
    return h


@contextlib.contextmanager
def count_pack_launches(h):
    """Calls of the weight-pack entry points issued from Python, per name (the proxy caches a launcher per name as an instance
    attribute; it is wrapped for the duration of the block)."""
    seen, keep = {}, {}

    def wrap(name, fn):
        def wrapped(*a):
            seen[name] = seen.get(name, 0) + 1
            return fn(*a)
        return wrapped
    for name in PACK_LAUNCHES:
        keep[name] = getattr(h.LIB, name)
        setattr(h.LIB, name, wrap(name, keep[name]))
    try:
        yield seen
    finally:
        for name, fn in keep.items():
            setattr(h.LIB, name, fn)


# ============================================================================ packed weights
# (kind, dtype code) -> PRECISION, GRAD_SPLIT, role, conv channels C -> K and the image of the conv's INPUT (B, H, W): the
# smallest geometry at which hipops.conv_weight returns that kind (egz_conv3x3_streamed_ok: every plain geometry of this size
# with C % 32 == 0 is streamed; the upsample data gradient needs C % 128 == 0, the upsample forward K % 64 == 0), odd sizes,
# two images.  Up to 16 x 16 pixels the plane-ordered 'fwd' / 'dgrad' / 'ups_fwd' kinds are reached in exact f32 only; the
# forward pass is f16 x3 under either GRAD_SPLIT.
CASES = {
    ("fwd", 0): ("f32", "f16", "fwd", 32, 64, (2, 6, 5)),
    ("dgrad", 0): ("f32", "f16", "dgrad", 64, 32, (2, 6, 5)),
    ("ups_fwd", 0): ("f32", "f16", "ups_fwd", 32, 64, (2, 4, 3)),
    ("ups_dgrad", 0): ("f32", "f16", "ups_dgrad", 64, 32, (2, 4, 3)),
    ("ups_dgrad", 1): ("split", "f16", "ups_dgrad", 64, 32, (2, 4, 3)),
    ("ups_dgrad", 2): ("split", "bf16", "ups_dgrad", 64, 32, (2, 4, 3)),
    ("fwd_frag", 1): ("split", "f16", "fwd", 32, 64, (2, 6, 5)),
    ("dgrad_frag", 1): ("split", "f16", "dgrad", 64, 64, (2, 6, 5)),
    ("dgrad_frag", 2): ("split", "bf16", "dgrad", 64, 64, (2, 6, 5)),
    ("ups_fwd_frag", 1): ("split", "f16", "ups_fwd", 32, 64, (2, 4, 3)),
    ("ups_dgrad_frag", 1): ("split", "f16", "ups_dgrad", 128, 32, (2, 4, 3)),
    ("ups_dgrad_frag", 2): ("split", "bf16", "ups_dgrad", 128, 32, (2, 4, 3)),
}
CASE_IDS = sorted(CASES)
ROUTES = ("adam-batch", "adam-lazy", "sgd", "copy_", "load_state_dict", "assign", "state_dict-write", "data-assign",
          "data+touch", "data+bump", "init_like_reference", "second-adam")


def _wscale(K):
    return (2.0 / (9 * K)) ** 0.5            # utils.init_like_reference's (fan-out): every draw of a weight has this scale


@functools.lru_cache(maxsize=None)
def _operand(case):
    """The gathered operand of the case's launch (CPU, logical NCHW): x for the forward roles, dy for the gradients."""
    _, _, role, C, K, (B, Hh, Ww) = CASES[case]
    if role == "fwd":
        return rnd(B, C, Hh, Ww, seed=11)
    if role == "ups_fwd":
        return rnd(B, C, Hh, Ww, seed=12)
    if role == "dgrad":
        return rnd(B, K, Hh, Ww, seed=13)
    return rnd(B, K, 2 * Hh, 2 * Ww, seed=14)


@functools.lru_cache(maxsize=None)
def _operand_dev(case):
    return nhwc(_operand(case))


def reference(case, w, b):
    """fp64 torch.nn.functional on the CPU for the case's launch with weight ``w`` / bias ``b`` (any device, any dtype)."""
    _, _, role, C, K, (B, Hh, Ww) = CASES[case]
    w64, b64 = w.detach().double().cpu(), b.detach().double().cpu()
    op = _operand(case).double()
    if role == "fwd":
        return F.conv2d(op, w64, b64, padding=1)
    if role == "ups_fwd":
        return F.conv2d(F.interpolate(op, scale_factor=2, mode="nearest"), w64, b64, padding=1)
    x = torch.zeros(B, C, Hh, Ww, dtype=torch.float64, requires_grad=True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if role == "ups_dgrad" else x
    (dx,) = torch.autograd.grad(F.conv2d(xin, w64, b64, padding=1), x, op)
    return dx


def launch(h, case, conv):
    """The case's public launch on ``conv``'s current parameters -> (result as CPU NCHW, uid of the weight).  Asserts the
    packing kind and dtype conv_weight handed out, so that a dispatch change cannot turn the case into a repeat of another."""
    kind, dtype = case
    _, _, role, C, K, _ = CASES[case]
    op = _operand_dev(case)
    w = conv.weight
    fwd = role in ("fwd", "ups_fwd")
    dt = h.conv_dtype("fwd", K, C, op) if fwd else h.conv_dtype("dgrad", C, K, op)
    wp, st = h.conv_weight(w, role, dt, op, K if fwd else C)
    keys = [k for k, v in h._PACKED.items() if v[1] is wp]
    assert keys == [(w._egz_uid, kind, dtype)] and dt == dtype and st == kind.endswith("_frag"), (keys, dt, st)
    if role == "fwd":
        y, _ = h.conv3x3_fwd(op, wp, conv.bias.detach(), K, epi=h.EPI_BIAS, dtype=dt, streamed=st)
    elif role == "ups_fwd":
        y, _ = h.conv3x3_fwd(op, wp, conv.bias.detach(), K, ups="phase", epi=h.EPI_BIAS, dtype=dt, streamed=st)
    elif role == "dgrad":
        y = h.conv3x3_dgrad(op, wp, C, dtype=dt, streamed=st)
    else:
        y = h.conv3x3_ups_dgrad(op, wp, C, dtype=dt, streamed=st)
    return nchw(y), w._egz_uid


def make_conv(C, K, seed=1):
    conv = nn.Conv2d(C, K, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(rnd(K, C, 3, 3, seed=seed, scale=_wscale(K)))
        conv.bias.copy_(rnd(K, seed=seed + 1, scale=0.1))
    return conv.to(DEV)


def _adam_write(opt, conv, seed):
    """One FusedAdam step that moves every weight element by 2 sigma with an independent random sign (first step of Adam:
    lr * g / (|g| + eps)); the bias gradient stays zero."""
    opt.zero_grad()
    conv.weight.grad.copy_(torch.sign(rnd(*conv.weight.shape, seed=seed)).to(DEV))
    opt.step()


def prepare(h, route, conv):
    """What a route needs in place BEFORE the first launch fills the cache."""
    from egaze_amd.optim import FusedAdam
    if route in ("adam-batch", "adam-lazy", "second-adam"):
        return FusedAdam(conv.parameters(), lr=2.0 * _wscale(conv.out_channels))
    return None


def mutate(h, route, conv, opt, seed=101):
    """Replace ``conv``'s weight (and bias, where the route carries one) by an independent draw.  Returns what must stay alive."""
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import init_like_reference
    K, C = conv.out_channels, conv.in_channels
    new_w = rnd(K, C, 3, 3, seed=seed, scale=_wscale(K)).to(DEV)
    new_b = rnd(K, seed=seed + 1, scale=0.1).to(DEV)
    if route in ("adam-batch", "adam-lazy"):
        _adam_write(opt, conv, seed)
    elif route == "second-adam":
        opt2 = FusedAdam(conv.parameters(), lr=2.0 * _wscale(K))
        _adam_write(opt2, conv, seed)
        return opt2
    elif route == "sgd":
        conv.weight.grad = conv.weight.detach() - new_w
        conv.bias.grad = conv.bias.detach() - new_b
        torch.optim.SGD(conv.parameters(), lr=1.0).step()
    elif route == "copy_":
        with torch.no_grad():
            conv.weight.copy_(new_w)
            conv.bias.copy_(new_b)
    elif route == "load_state_dict":
        conv.load_state_dict({"weight": new_w, "bias": new_b})
    elif route == "assign":
        conv.load_state_dict({"weight": new_w, "bias": new_b}, assign=True)
    elif route == "state_dict-write":
        sd = conv.state_dict()
        sd["weight"].copy_(new_w)
        sd["bias"].copy_(new_b)
    elif route == "data-assign":
        conv.weight.data = new_w
        conv.bias.data = new_b
    elif route in ("data+touch", "data+bump"):
        conv.weight.data.copy_(new_w)
        conv.bias.data.copy_(new_b)
        if route == "data+touch":
            h.touch_params([conv.weight, conv.bias])
        else:
            h.bump_weight_epoch()
    elif route == "init_like_reference":
        torch.manual_seed(seed)
        init_like_reference(conv)                 # N(0, sqrt(2 / (9 K))) weight, zero bias
    else:
        raise AssertionError(route)
    return None


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", CASE_IDS, ids=[f"{k}-dt{d}" for k, d in CASE_IDS])
def test_packed_weight_follows(case, route, monkeypatch):
    precision, grad_split, _, C, K, _ = CASES[case]
    h = _precision(monkeypatch, precision, grad_split)
    monkeypatch.setattr(h, "BATCH_REPACK", route != "adam-lazy")
    conv = make_conv(C, K)
    opt = prepare(h, route, conv)
    ref0 = reference(case, conv.weight, conv.bias)
    got0, uid0 = launch(h, case, conv)
    e0 = rel(got0, ref0)
    keep = mutate(h, route, conv, opt)
    ref1 = reference(case, conv.weight, conv.bias)          # from the values as they are now
    got1, uid1 = launch(h, case, conv)
    e1, power = rel(got1, ref1), rel(ref0, ref1)
    print(f"{case} {route}: err before {e0:.2e} after {e1:.2e} (bar {TOL[case[1]]:.0e}), references differ by {power:.2f}")
    assert power > POWER
    assert e0 < TOL[case[1]]
    assert e1 < TOL[case[1]]
    if route == "assign":
        # a new Parameter object: none of the old one's entries may serve it, and they die with the old tensor
        assert uid1 != uid0
        gc.collect()
        assert not any(k[0] == uid0 for k in h._PACKED)
    else:
        assert uid1 == uid0
    del keep


def test_changing_one_weight_repacks_only_that_weight(monkeypatch):
    """Two weights with warm packings: a change of ``a`` (every counted route and the two declared ones) launches one repack,
    for ``a``; ``b``'s launch finds its packing fresh."""
    h = _precision(monkeypatch, "split")
    case = ("fwd_frag", 1)
    _, _, _, C, K, _ = CASES[case]
    a, b = make_conv(C, K, seed=1), make_conv(C, K, seed=5)
    for m in (a, b):
        assert rel(launch(h, case, m)[0], reference(case, m.weight, m.bias)) < TOL[1]
    for n, route in enumerate(("copy_", "load_state_dict", "state_dict-write", "data-assign", "data+touch", "sgd")):
        mutate(h, route, a, None, seed=200 + n)
        with count_pack_launches(h) as seen:
            gb, _ = launch(h, case, b)
            assert not seen, (route, seen)
            ga, _ = launch(h, case, a)
            assert sum(seen.values()) == 1, (route, seen)
        assert rel(ga, reference(case, a.weight, a.bias)) < TOL[1] and rel(gb, reference(case, b.weight, b.bias)) < TOL[1]


def test_touch_params_of_one_optimizer_leaves_another_models_packings_fresh(monkeypatch):
    """hipops.touch_params promises it for the AT optimizer next to the SP model: a FusedAdam step over ``a`` (touch_params +
    the batched refresh) launches nothing for ``b``, whose own optimizer exists but did not step."""
    from egaze_amd.optim import FusedAdam
    h = _precision(monkeypatch, "split")
    monkeypatch.setattr(h, "BATCH_REPACK", True)
    case = ("fwd_frag", 1)
    _, _, _, C, K, _ = CASES[case]
    a, b = make_conv(C, K, seed=1), make_conv(C, K, seed=5)
    oa = FusedAdam(a.parameters(), lr=2.0 * _wscale(K))
    ob = FusedAdam(b.parameters(), lr=2.0 * _wscale(K))           # (both constructors bump the global epoch: before the launches)
    ra0 = reference(case, a.weight, a.bias)
    for m in (a, b):
        launch(h, case, m)
    with count_pack_launches(h) as seen:
        _adam_write(oa, a, 300)
        assert seen == {"egz_pack_w3x3_frag_batch": 1}, seen       # a's one used packing, rebuilt by the step
        gb, _ = launch(h, case, b)
        ga, _ = launch(h, case, a)
        assert seen == {"egz_pack_w3x3_frag_batch": 1}, seen       # ... and both launches found theirs fresh
    ra1 = reference(case, a.weight, a.bias)
    assert rel(ra0, ra1) > POWER
    assert rel(ga, ra1) < TOL[1] and rel(gb, reference(case, b.weight, b.bias)) < TOL[1]
    del ob


# ============================================================================ eval rows and the BatchNorm fold
BLOCK_KEYS = {"weight": "0.weight", "conv-bias": "0.bias", "gamma": "1.weight", "beta": "1.bias",
              "running_mean": "1.running_mean", "running_var": "1.running_var"}
BLOCK_ROUTES = ("copy_", "load_state_dict", "data+touch", "data+bump")


def draw(name, seed):
    """An independent draw of one of the block's six tensors, O(1) effect on the output each."""
    g = torch.Generator().manual_seed(seed)
    if name == "weight":
        return torch.randn(64, 64, 3, 3, generator=g) * _wscale(64)
    if name == "gamma":
        return 0.5 + torch.rand(64, generator=g)
    if name == "running_var":
        return 0.25 + 3.0 * torch.rand(64, generator=g)
    return torch.randn(64, generator=g)                           # conv bias, beta, running_mean


def make_block(seed=20):
    from egaze_amd.utils import make_layers
    block = make_layers([64], 64)
    block.load_state_dict({key: draw(name, seed + n) for n, (name, key) in enumerate(BLOCK_KEYS.items())}, strict=False)
    return block.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _block_input(B):
    return rnd(B, 64, 8, 8, seed=31)


def block_reference(block, B):
    sd = {k: v.detach().double().cpu() for k, v in block.state_dict().items()}
    y = F.conv2d(_block_input(B).double(), sd["0.weight"], sd["0.bias"], padding=1)
    return F.relu(F.batch_norm(y, sd["1.running_mean"], sd["1.running_var"], sd["1.weight"], sd["1.bias"], training=False,
                               eps=block[1].eps))


def block_forward(h, block, B, fold):
    """One eval forward under no_grad -> CPU NCHW; asserts that the folded form ran exactly when it was asked for."""
    before = h.EVAL_FOLD_STATS["folded"]
    with torch.no_grad():
        out = block(_block_input(B).to(DEV))
    torch.cuda.synchronize()
    assert h.EVAL_FOLD_STATS["folded"] - before == (1 if fold else 0)
    return out.cpu()


def block_mutate(h, block, name, route, seed):
    key = BLOCK_KEYS[name]
    t = dict(block.named_parameters())
    t.update(dict(block.named_buffers()))
    t, new = t[key], draw(name, seed).to(DEV)
    if route == "copy_":
        with torch.no_grad():
            t.copy_(new)
    elif route == "load_state_dict":
        res = block.load_state_dict({key: new}, strict=False)
        assert not res.unexpected_keys
    else:
        t.data.copy_(new)
        if route == "data+touch":
            h.touch_params([t])
        else:
            h.bump_weight_epoch()


@pytest.mark.parametrize("route", BLOCK_ROUTES)
@pytest.mark.parametrize("name", list(BLOCK_KEYS))
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "rows"])
def test_eval_block_follows(fold, B, name, route, monkeypatch):
    """[Conv 64 -> 64, BatchNorm, ReLU] of utils.make_layers in eval mode at 8 x 8: the folded weights and bias and their
    packings (EVAL_FOLD on) / the eval rows and the weight's packing (off) after a change of one of the six tensors."""
    h = _precision(monkeypatch, "split")
    monkeypatch.setattr(h, "EVAL_FOLD", fold)
    block = make_block()
    ref0 = block_reference(block, B)
    e0 = rel(block_forward(h, block, B, fold), ref0)
    block_mutate(h, block, name, route, seed=77)
    ref1 = block_reference(block, B)
    e1, power = rel(block_forward(h, block, B, fold), ref1), rel(ref0, ref1)
    print(f"fold={fold} B={B} {name} {route}: err before {e0:.2e} after {e1:.2e}, references differ by {power:.2f}")
    assert power > POWER
    assert e0 < TOL_BLOCK and e1 < TOL_BLOCK


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "rows"])
def test_eval_block_follows_a_train_mode_forward(fold, monkeypatch):
    """bn_finalize writes the running statistics behind torch's back: the eval forward after a train-mode forward through the
    same block uses the updated statistics (momentum 1: the batch statistics replace the drawn ones outright)."""
    h = _precision(monkeypatch, "split")
    monkeypatch.setattr(h, "EVAL_FOLD", fold)
    B = 2
    block = make_block()
    block[1].momentum = 1.0
    ref0 = block_reference(block, B)
    assert rel(block_forward(h, block, B, fold), ref0) < TOL_BLOCK
    block.train()
    with torch.no_grad():
        block(rnd(B, 64, 8, 8, seed=32, scale=2.0).to(DEV) + 1.0)
    block.eval()
    ref1 = block_reference(block, B)
    assert rel(ref0, ref1) > POWER
    assert rel(block_forward(h, block, B, fold), ref1) < TOL_BLOCK


# ============================================================================ the abs-max scalar an activation carries
@pytest.mark.parametrize("producer", ["bn-relu-pass", "conv-epilogue"])
@pytest.mark.parametrize("scale", [2.0 ** 12, 2.0 ** -12], ids=["x4096", "div4096"])
def test_absmax_scalar_does_not_outlive_an_in_place_write(scale, producer, monkeypatch):
    """The output of an encoder block carries max |a| from the pass that wrote it (the BatchNorm -> ReLU pass; the bias + ReLU
    epilogue of the folded eval conv); a forward hook scales the output in place.  The next block (functions.ConvReLU: conv ->
    ReLU, so the f16 x3 bar applies to its output as it stands) must split the scaled values by their own maximum: with the
    stale scalar the f16 hi half saturates at x 4096: with the version check of functions.to_nhwc taken out on a scratch copy
    both x 4096 cases fail with error 1.0.  Scaling DOWN shows no effect of a stale scalar in this kernel (measured with the
    check taken out: 3.6e-8 at / 4096 and at / 2^24, the same as with it), so the / 4096 case only guards the fresh path."""
    from egaze_amd.functions import ConvReLU
    h = _precision(monkeypatch, "split")
    monkeypatch.setattr(h, "EVAL_FOLD", True)
    block = make_block()
    if producer == "bn-relu-pass":
        block.train()
    nxt = make_conv(64, 64, seed=41)
    seen = []

    def hook(mod, inp, out):
        seen.append(getattr(out, "_egz_absmax", None) is not None)
        out.mul_(scale)
    handle = block.register_forward_hook(hook)
    try:
        with torch.no_grad():
            a = block(_block_input(2).to(DEV))
            y = ConvReLU.apply(a, nxt.weight, nxt.bias, False)
    finally:
        handle.remove()
    assert seen == [True]                                        # (the producer did attach a scalar: the case tests something)
    ref = F.relu(F.conv2d(a.detach().double().cpu(), nxt.weight.detach().double().cpu(), nxt.bias.detach().double().cpu(),
                          padding=1))
    err = rel(y.cpu(), ref)
    print(f"{producer} x {scale}: {err:.2e}")
    assert err < TOL[1]


# ============================================================================ captured steps
GRAPH_ROUTES = ("copy_", "load_state_dict", "data-assign", "data+touch", "data+bump")


def _graph_mutate(h, module, key, route, new):
    t = dict(module.named_parameters())
    t.update(dict(module.named_buffers()))
    t = t[key]
    new = new.to(DEV)
    if route == "copy_":
        with torch.no_grad():
            t.copy_(new)
    elif route == "load_state_dict":
        module.load_state_dict({key: new}, strict=False)
    elif route == "data-assign":
        t.data = new
    else:
        t.data.copy_(new)
        if route == "data+touch":
            h.touch_params([t])
        else:
            h.bump_weight_epoch()


@pytest.mark.parametrize("route", GRAPH_ROUTES)
@pytest.mark.parametrize("name", ["weight", "running_var"])
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_graphed_module_replay_follows(precision, name, route, monkeypatch):
    """graphs.GraphedModule over a two-block eval encoder at 32 x 32, batch 1: a change of the SECOND block's weight / running
    variance between two replays.  The replay equals the eager forward from the same state bit for bit, shows the new values,
    and a further replay of the unchanged model issues no pack launch, keeps its graph and returns the same values."""
    from egaze_amd.graphs import GraphedModule
    from egaze_amd.utils import make_layers
    h = _precision(monkeypatch, precision)
    enc = make_layers([64, 64], 64)
    sd = {}
    for n, blk in enumerate((0, 3)):
        for m, (nm, key) in enumerate(BLOCK_KEYS.items()):
            sd[f"{blk + int(key[0])}.{key[2:]}"] = draw(nm, 50 + 10 * n + m)
    enc.load_state_dict(sd, strict=False)
    enc = enc.to(DEV).eval()
    x = rnd(1, 64, 32, 32, seed=33).to(DEV)
    g = GraphedModule(enc, (x,))
    o1 = g(x).clone()
    with torch.no_grad():
        assert torch.equal(o1, enc(x))
    key = "3.weight" if name == "weight" else "4.running_var"
    _graph_mutate(h, enc, key, route, draw(name, 99))
    o2 = g(x).clone()
    with torch.no_grad():
        e2 = enc(x).clone()
    graph = g.graph
    with count_pack_launches(h) as seen:
        o3 = g(x).clone()
    print(f"{precision} {name} {route}: replay vs eager {rel(o2, e2):.2e}, third replay vs eager {rel(o3, e2):.2e}, "
          f"before vs after {rel(o1, o2):.2f}, pack launches of the unchanged replay {seen}")
    assert torch.equal(o2, e2)
    assert torch.equal(o3, e2)
    assert rel(o1, o2) > POWER
    assert not seen and g.graph is graph


def _lf_run(h, graphed, route, table_miss=False, steps=6, at=4):
    """``steps`` late-fusion training steps at 32 x 32, batch 2, on one batch; ``route`` rewrites fusion.3.weight in front of step
    ``at`` (with warm = 2 the graphed run captures at step 2 and replays from there on: the write falls between two replays).
    ``table_miss``: the capturing call finds no pointer table for the step's packing set (as after an eval pass in between), so
    the captured refresh cannot be the one-launch form.
    -> (losses, last output, flat parameters, pack launches issued from Python by the last step)."""
    from oracle import egaze_oracle as O
    from oracle import synth
    from egaze_amd.floss import floss
    from egaze_amd.graphs import GraphedTrainStep
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.optim import FusedAdam
    model = late_fusion()
    model.load_state_dict(synth.synth_state_dict(O.lf_shapes(), seed=3, head_gain=0.5))
    model.to(DEV).train()
    crit = floss().to(DEV)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    im, feat, gt = (t.to(DEV) for t in synth.synth_lf_batch(2, 32, seed=7))
    new = rnd(32, 32, 3, 3, seed=123, scale=(2.0 / (9 * 32)) ** 0.5)

    def fwd_loss(f, i, t):
        o = model(f, i)
        return crit(o, t), o
    step = GraphedTrainStep(fwd_loss, opt, (feat, im, gt), warm=2) if graphed else None
    losses, seen = [], {}
    for n in range(steps):
        if n == at and route is not None:
            _graph_mutate(h, model, "fusion.3.weight", route, new)
        if n == 2 and graphed and table_miss:
            h._BATCH_TABLES.clear()
            h._BATCH_PINNED.clear()
        with count_pack_launches(h) as seen:
            if graphed:
                l, o = step(feat, im, gt)
            else:
                l, o = fwd_loss(feat, im, gt)
                opt.zero_grad()
                l.backward()
                opt.step()
        losses.append(l.item())
    torch.cuda.synchronize()
    res = (losses, o.detach().clone(), opt.flat_p.clone(), dict(seen))
    if graphed:
        assert step.graph is not None
        step.close()
    return res


_LF_CONTROL = {}


@pytest.mark.parametrize("table_miss", [False, True], ids=["table", "table_miss"])
@pytest.mark.parametrize("route", ["copy_", "load_state_dict", "data+touch", "data+bump"])
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_graphed_train_step_replay_follows(precision, route, table_miss, monkeypatch):
    """graphs.GraphedTrainStep over the late-fusion step: an optimizer parameter rewritten between two replays.  The captured
    step trusts the packings its own Adam update left behind, so the write must be repacked in front of the replay: losses,
    output and parameters equal the eager run's bit for bit, the write shows (against an eager run without it), and the replay
    of the unchanged model after it issues no pack launch.  (Re-allocating a FusedAdam parameter, route data-assign, takes it out
    of the optimizer's flat buffer in an eager run as well; it is no cache question and is not run here.)  ``table_miss``: the
    captured refresh is the per-packing form (no pointer table at capture time); every replay must still repack."""
    h = _precision(monkeypatch, precision)
    if precision not in _LF_CONTROL:
        _LF_CONTROL[precision] = _lf_run(h, False, None)
    l0, o0, p0, _ = _lf_run(h, False, route)
    l1, o1, p1, seen = _lf_run(h, True, route, table_miss)
    lc = _LF_CONTROL[precision][0]
    print(f"{precision} {route}: eager {l0}, graphed {l1}, untouched {lc}")
    assert l0[:4] == lc[:4] and abs(l0[4] - lc[4]) > 1e-3 * abs(lc[4])      # the write is visible in the step after it
    assert l1 == l0
    assert torch.equal(o1, o0) and torch.equal(p1, p0)
    assert not seen                                             # the last replay: nothing changed since the one before


def _frozen_run(h, graphed, route, steps=6, at=4):
    """The stream pre-training pattern (streamtrain.GraphedStreamStep) at its smallest: a FROZEN [Conv 64 -> 64, ReLU] encoder run
    under no_grad, a trained [Conv 64 -> 64, ReLU, Conv 1x1 -> Sigmoid] decoder, floss, FusedAdam over the decoder; 32 x 32,
    batch 2.  The encoder's parameters are the step's ``extra_params``: the graph bakes their packings in and nothing inside
    it rebuilds them.  ``route`` rewrites the encoder's weight in front of step ``at``, between two replays.
    -> (losses, last output, flat parameters, pack launches issued from Python by the last step)."""
    from egaze_amd.floss import floss
    from egaze_amd.graphs import GraphedTrainStep
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import FusedSequential
    enc = FusedSequential(nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(inplace=True))
    dec = FusedSequential(nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(64, 1, 1))
    with torch.no_grad():
        for n, p in enumerate(list(enc.parameters()) + list(dec.parameters())):
            p.copy_(rnd(*p.shape, seed=140 + n, scale=_wscale(64) if p.dim() == 4 else 0.1))
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).train()
    for p in enc.parameters():
        p.requires_grad_(False)
    crit = floss().to(DEV)
    opt = FusedAdam(dec.parameters(), lr=1e-3)
    x = rnd(2, 64, 32, 32, seed=150).to(DEV)
    gt = torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(151)).to(DEV)
    new = rnd(64, 64, 3, 3, seed=152, scale=_wscale(64))

    def fwd_loss(a, t):
        with torch.no_grad():
            f = enc(a)
        o = dec(f, fuse_sigmoid=True)
        return crit(o, t), o
    step = GraphedTrainStep(fwd_loss, opt, (x, gt), warm=2, extra_params=list(enc.parameters())) if graphed else None
    losses, seen = [], {}
    for n in range(steps):
        if n == at and route is not None:
            _graph_mutate(h, enc, "0.weight", route, new)
        with count_pack_launches(h) as seen:
            if graphed:
                l, o = step(x, gt)
            else:
                l, o = fwd_loss(x, gt)
                opt.zero_grad()
                l.backward()
                opt.step()
        losses.append(l.item())
    torch.cuda.synchronize()
    res = (losses, o.detach().clone(), opt.flat_p.clone(), dict(seen))
    if graphed:
        assert step.graph is not None
        step.close()
    return res


_FROZEN_CONTROL = {}


@pytest.mark.parametrize("route", GRAPH_ROUTES)
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_graphed_train_step_extra_params_follow(precision, route, monkeypatch):
    """graphs.GraphedTrainStep(extra_params=...): a frozen encoder's weight rewritten between two replays, by a counted write, a
    declared ``.data`` write (per tensor, or with the global epoch alone: ``_extra_signature`` must see both) or a re-allocation
    (which re-captures).  Losses, output and parameters equal the eager run's bit for bit, the write shows, and the replay of
    the unchanged model after it issues no pack launch."""
    h = _precision(monkeypatch, precision)
    if precision not in _FROZEN_CONTROL:
        _FROZEN_CONTROL[precision] = _frozen_run(h, False, None)
    l0, o0, p0, _ = _frozen_run(h, False, route)
    l1, o1, p1, seen = _frozen_run(h, True, route)
    lc = _FROZEN_CONTROL[precision][0]
    print(f"{precision} {route}: eager {l0}, graphed {l1}, untouched {lc}")
    assert l0[:4] == lc[:4] and abs(l0[4] - lc[4]) > 1e-3 * abs(lc[4])      # the write is visible in the step after it
    assert l1 == l0
    assert torch.equal(o1, o0) and torch.equal(p1, p0)
    assert not seen
