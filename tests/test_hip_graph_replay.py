"""What a hipGraph replay leaves behind, and what it fails to pick up.

A replay of graphs.GraphedTrainStep rewrites parameters (Adam), BatchNorm running statistics and ``num_batches_tracked``
(bn_finalize*) on the device; the host side of those launches -- hipops.touch_params -- ran once, at capture.  The step object
therefore repeats the declarations after every replay (hipops.note_replay, fed by what hipops.capture logged).  This module
pins that, the input side of a replay (the static buffers), and the drivers over more than one epoch.

One yardstick throughout: a graphed run equals its eager twin BIT FOR BIT -- the same model, seed, inputs and order of calls,
issued launch by launch.  No new tolerance.  Where an fp64 check is made it is oracle.egaze_oracle on the state read back at
that moment, at the bar the existing test of the same forward uses: TOL_BLOCK = 1e-5 of test_hip_cache_coherence.py for an eval
[conv -> BatchNorm -> ReLU] block (folded or not), 2e-5 of test_hip_lf.py::test_late_fusion_golden for the eval-mode
late_fusion map.  Every case that waits for a cache to go stale asserts its own power: in the eager twin the two eval outputs
it compares differ by more than POWER = 0.1 of max|ref| (learning rate, BatchNorm momentum and the training inputs'
distribution are chosen for that, from an fp64 CPU run of the same sequence: 0.27 for the late-fusion map, 0.35 for the
encoder features of the stream pattern, whose sigmoid map moves by 0.05 only and is compared but carries no power claim).

1. test_replay_is_a_write_route_into_the_eval_caches: warm-up, capture, replay, eval A, two replays, eval B, replay, a
   trailing eager step on a batch of another size, eval C -- over the late-fusion step (BatchNorm in the trained stack) and the
   stream pre-training pattern (a frozen train-mode encoder under no_grad: replays move its running statistics only; a
   trained decoder), precision split / f32, EVAL_FOLD on / off, the eval forward eager or itself a graphs.GraphedModule that
   stays alive across the replays.  Without hipops.note_replay eval B (and C's BatchNorm caches) reuse eval A's rows, folds and
   packings: every case of this test fails on such a build.
2. The values of the second and third replay of a re-captured GraphedModule equal the first (the module form above, and
   test_hip_cache_coherence.py::test_graphed_module_replay_follows).
3. test_graphed_*_input_scale: a replay fed the example input, the input x 2^12, x 2^-12 and the example again through the
   static buffers -- what a replay scales its f16 split by must be computed inside the replay -- with and without an
   ``_egz_absmax`` / ``_egz_prepared`` attribute on the caller's tensor.
4. test_*_driver_three_epochs: LF._run, streamtrain.train_epoch + evaluate and AT._epoch, train then validate, three epochs,
   graph on against graph off (AT also: a filled ResidentLSTMDataset against the file loop): the same Python floats per epoch
   and a bit-identical checkpoint at the end.

AT._GraphedSampleStep repeats no declaration after a replay and needs none: the LSTM path reads no cache keyed by
hipops.packing._tag (no reader of ``_tag(`` / ``_egz_epoch`` outside hipops.packing, hipops.bn and graphs.py).

What this module found besides the missing declarations.  The stream pattern in f16 x3 with EVAL_FOLD off was red in about half
of its runs, on the build before this module as well (there with the documented touch_params in front of each eval): the first
replay after an eager eval forward computed with another -- sometimes a useless -- scale of its f16 split (eval maps off by 1.6e-7
up to 0.38 of max|ref|, the same few values run after run), with the helper streams on or off and with a device synchronisation in
front of every step, and never with hipops.FWD_SCALE off.  The step's first convolution reads a static input, whose max |x| comes
from the standalone pass egz_absmax; that pass zero-filled its buffer with hipMemsetAsync, which a capture turns into a memset
node.  With the zero fill issued as a kernel (csrc/bn_pool.hip) 12 of 12 runs were bit-identical, against 7 red of 14 before.
"""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn as nn

from oracle import egaze_oracle as O
from oracle import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_cache_coherence import (BLOCK_KEYS, DEV, POWER, TOL_BLOCK, H, _precision, _wscale,  # noqa: E402
                                      count_pack_launches, draw, make_block, rel, rnd)
from test_hip_lf import build as build_lf  # noqa: E402
from test_hip_lf_step_ops import TRACKED  # noqa: E402
from test_hip_model_sp import build_model as build_sp  # noqa: E402
from test_hip_streams import build as build_stream, key_of  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_LF_EVAL = 2e-5             # test_hip_lf.py::test_late_fusion_golden: the eval-mode late_fusion map
SCALES = (1.0, 2.0 ** 12, 2.0 ** -12, 1.0)


@contextlib.contextmanager
def count_tracked(h):
    """Calls of the hipops entry points of a training step (test_hip_lf_step_ops.TRACKED) issued from Python, per name."""
    seen, keep = {}, {}

    def wrap(name, fn):
        def wrapped(*a, **kw):
            seen[name] = seen.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapped
    for name in TRACKED:
        keep[name] = getattr(h, name)
        setattr(h, name, wrap(name, keep[name]))
    try:
        yield seen
    finally:
        for name, fn in keep.items():
            setattr(h, name, fn)


def two_block_encoder(momentum=0.1):
    """The two-block encoder of test_graphed_module_replay_follows: make_layers([64, 64], 64) with drawn tensors."""
    from egaze_amd.utils import make_layers
    enc = make_layers([64, 64], 64)
    sd = {}
    for n, blk in enumerate((0, 3)):
        for m, (nm, key) in enumerate(BLOCK_KEYS.items()):
            sd[f"{blk + int(key[0])}.{key[2:]}"] = draw(nm, 50 + 10 * n + m)
    enc.load_state_dict(sd, strict=False)
    for m in enc:
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = momentum
    return enc.to(DEV)


# ============================================================================ the two step patterns
class LFPattern:
    """The late-fusion step of test_hip_cache_coherence._lf_run (model, seed, loss, optimizer) at 32 x 32, batch 2; a trailing
    batch of 3.  BatchNorm sits in the trained stack: a step moves weights, running statistics and num_batches_tracked."""
    name = "lf"

    def __init__(self, lr=1e-2):
        from egaze_amd.floss import floss
        from egaze_amd.optim import FusedAdam
        self.model = build_lf().train()
        self.crit = floss().to(DEV)
        self.opt = FusedAdam(self.model.parameters(), lr=lr)
        self.extra = ()
        self.batches = [self._batch(2, 7 + k) for k in range(7)]
        self.tail = self._batch(3, 20)
        self.probe = self._batch(2, 30)[:2]

    @staticmethod
    def _batch(n, seed):
        im, feat, gt = (t.to(DEV) for t in synth.synth_lf_batch(n, 32, seed=seed))
        return feat, im, gt

    def fwd_loss(self, f, i, t):
        o = self.model(f, i)
        return self.crit(o, t), o

    def scaled(self, batch, s):
        return (batch[0] * s, batch[1] * s, batch[2])

    def oracle_errors(self, got):
        """[(error of the eval map against fp64 from the state as it is now, its bar)]; the model is in eval mode."""
        sd = {k: (v.detach().double().cpu() if v.is_floating_point() else v.cpu()) for k, v in self.model.state_dict().items()}
        ref = O.late_fusion_forward(sd, self.probe[0].double().cpu(), self.probe[1].double().cpu(), training=False)
        return [(rel(got[0], ref), TOL_LF_EVAL)]


class _EncDec(nn.Module):
    def __init__(self, enc, dec):
        super().__init__()
        self.enc, self.dec = enc, dec

    def forward(self, x):
        f = self.enc(x)
        return f, self.dec(f, fuse_sigmoid=True)


class StreamPattern:
    """The stream pre-training pattern (streamtrain.step_forward): make_layers([64, 64], 64) as a frozen encoder that runs in
    TRAIN mode under no_grad, the trained decoder of test_hip_cache_coherence._frozen_run, floss, FusedAdam over the decoder; the
    encoder's parameters are the step's ``extra_params``.  A step moves the encoder's running statistics (momentum 0.2, training
    inputs N(1, 2): far from the drawn statistics) and the decoder's weights.  An eval returns (encoder features, map)."""
    name = "stream"

    def __init__(self, lr=1e-2, carry=False):
        from egaze_amd.floss import floss
        from egaze_amd.optim import FusedAdam
        from egaze_amd.utils import FusedSequential
        dec = FusedSequential(nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(64, 1, 1))
        with torch.no_grad():
            for n, p in enumerate(dec.parameters()):
                p.copy_(rnd(*p.shape, seed=140 + n, scale=_wscale(64) if p.dim() == 4 else 0.1))
        self.model = _EncDec(two_block_encoder(momentum=0.2), dec).to(DEV).train()
        for p in self.model.enc.parameters():
            p.requires_grad_(False)
        self.crit = floss().to(DEV)
        self.opt = FusedAdam(dec.parameters(), lr=lr)
        self.extra = list(self.model.enc.parameters())
        self.batches = [self._batch(2, 150 + k) for k in range(7)]
        self.tail = self._batch(3, 160)
        self.probe = (rnd(2, 64, 32, 32, seed=190).to(DEV),)
        if carry:
            # the example input comes out of a producer block and carries its abs-max scalar (hipops.bn_relu_pool_fwd)
            with torch.no_grad():
                x = make_block().train()(self.batches[0][0])
            self.batches[0] = (x, self.batches[0][1])

    @staticmethod
    def _batch(n, seed):
        gt = torch.rand(n, 1, 32, 32, generator=torch.Generator().manual_seed(seed + 20))
        return (rnd(n, 64, 32, 32, seed=seed, scale=2.0) + 1.0).to(DEV), gt.to(DEV)

    def fwd_loss(self, a, t):
        with torch.no_grad():
            f = self.model.enc(a)
        o = self.model.dec(f, fuse_sigmoid=True)
        return self.crit(o, t), o

    def scaled(self, batch, s):
        return (batch[0] * s, batch[1])

    def oracle_errors(self, got):
        """Each encoder block on its own (the forward test_eval_block_follows bounds), launch by launch: block 2 is fed block 1's
        fp32 output in both the launch and the fp64 reference.  The model is in eval mode."""
        enc = self.model.enc
        sd = {k: (v.detach().double().cpu() if v.is_floating_point() else v.cpu()) for k, v in enc.state_dict().items()}
        x, errs = self.probe[0], []
        for blk in (0, 3):
            with torch.no_grad():
                y = enc[blk:blk + 3](x)
            one = {f"{int(k.split('.')[0]) - blk}.{k.split('.', 1)[1]}": v for k, v in sd.items()
                   if blk <= int(k.split('.')[0]) < blk + 3}
            ref = O.encoder_forward(one, "", x.detach().double().cpu(), False, cfg=[64])
            errs.append((rel(y, ref), TOL_BLOCK))
            x = y.detach().clone()
        return errs


PATTERNS = {"lf": LFPattern, "stream": StreamPattern}


def _tuple(out):
    return tuple(t.detach().clone() for t in (out if isinstance(out, (tuple, list)) else (out,)))


def _state(pat):
    torch.cuda.synchronize()
    return dict(p=pat.opt.flat_p.clone(), m=pat.opt.flat_m.clone(), v=pat.opt.flat_v.clone(), steps=pat.opt.step_count,
                sd={k: v.detach().clone() for k, v in pat.model.state_dict().items()})


def _assert_same_state(got, want):
    assert got["steps"] == want["steps"]
    for k in ("p", "m", "v"):
        assert torch.equal(got[k], want[k]), k
    assert list(got["sd"]) == list(want["sd"])
    for k in want["sd"]:                                    # parameters, running statistics, num_batches_tracked
        assert torch.equal(got["sd"][k], want["sd"][k]), k


def _train(pat, step, batch, res):
    if step is not None:
        l, o = step(*batch)
    else:
        l, o = pat.fwd_loss(*batch)
        pat.opt.zero_grad()
        l.backward()
        pat.opt.step()
    res["losses"].append(l.item())
    res["outs"].append(o.detach().clone())


# ============================================================================ 1. (and 2.) a replay as a write route
def _sequence(pat, graphed, module_form):
    """The sequence of the module docstring on one step object with warm = 2 -> what was seen on the way."""
    from egaze_amd.graphs import GraphedModule, GraphedTrainStep
    h = H()
    step = GraphedTrainStep(pat.fwd_loss, pat.opt, pat.batches[0], warm=2, extra_params=pat.extra) if graphed else None
    gm = GraphedModule(pat.model, pat.probe) if module_form else None
    res = dict(losses=[], outs=[], evals={}, oracle=[], again=[])

    def evaluate(tag):
        pat.model.eval()
        with torch.no_grad():
            res["evals"][tag] = _tuple(gm(*pat.probe) if gm is not None else pat.model(*pat.probe))
            if tag == "B":
                if gm is not None:                          # part 2: two more replays of the graph that was just re-captured
                    graph = gm.graph
                    res["again"] = [_tuple(gm(*pat.probe)), _tuple(gm(*pat.probe))]
                    assert gm.graph is graph
                res["oracle"] = pat.oracle_errors(res["evals"][tag])
        pat.model.train()

    for k in range(4):                                      # two eager steps, the capture (+ its replay), one replay
        _train(pat, step, pat.batches[k], res)
    evaluate("A")
    for k in (4, 5):
        _train(pat, step, pat.batches[k], res)
    evaluate("B")
    with count_pack_launches(h) as packs, count_tracked(h) as calls:
        _train(pat, step, pat.batches[6], res)
    res["packs"], res["calls"] = dict(packs), dict(calls)
    _train(pat, None, pat.tail, res)                        # as train_epoch / LF._run_loop issue a trailing partial batch
    evaluate("C")
    if step is not None:
        assert step.graph is not None and step.calls == 7
        step.close()
    res["state"] = _state(pat)
    return res


_TWINS = {}


def _twin(h, pattern, precision, fold):
    key = (pattern, precision, fold)
    if key not in _TWINS:
        _TWINS[key] = _sequence(PATTERNS[pattern](), False, False)
    return _TWINS[key]


@pytest.mark.parametrize("form", ["eager-eval", "graphed-eval"])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "rows"])
@pytest.mark.parametrize("precision", ["split", "f32"])
@pytest.mark.parametrize("pattern", ["lf", "stream"])
def test_replay_is_a_write_route_into_the_eval_caches(pattern, precision, fold, form, monkeypatch):
    h = _precision(monkeypatch, precision)
    monkeypatch.setattr(h, "EVAL_FOLD", fold)
    want = _twin(h, pattern, precision, fold)
    got = _sequence(PATTERNS[pattern](), True, form == "graphed-eval")
    power = [rel(a, b) for a, b in zip(want["evals"]["A"], want["evals"]["B"])]
    print(f"{pattern} {precision} fold={fold} {form}: eager A vs B {power}, fp64 at B {got['oracle']}, "
          f"launches of the last replay {got['packs']} {got['calls']}")
    assert power[0] > POWER                                 # (the late-fusion map; the stream pattern's encoder features)
    for tag in "ABC":
        for n, (a, b) in enumerate(zip(got["evals"][tag], want["evals"][tag])):
            assert torch.equal(a, b), (tag, n, rel(a, b))
    for again in got["again"]:                              # the second and third replay of the re-captured GraphedModule
        for n, (a, b) in enumerate(zip(again, got["evals"]["B"])):
            assert torch.equal(a, b), ("again", n, rel(a, b))
    for err, bar in got["oracle"]:
        assert err < bar, got["oracle"]
    assert got["losses"] == want["losses"]
    for n, (a, b) in enumerate(zip(got["outs"], want["outs"])):
        assert torch.equal(a, b), n
    _assert_same_state(got["state"], want["state"])
    assert not got["packs"] and not got["calls"]            # the replay and its declarations: host only


# ============================================================================ 3. input scale through the static buffers
@pytest.mark.parametrize("carry", [False, True], ids=["plain", "carried"])
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_graphed_module_input_scale_encoder(precision, carry, monkeypatch):
    """GraphedModule over the two-block eval encoder at 32 x 32, batch 1.  ``carried``: the example input is the output of a
    producer block and carries its abs-max scalar when it is handed to the constructor and to the calls."""
    from egaze_amd.graphs import GraphedModule
    h = _precision(monkeypatch, precision)
    enc = two_block_encoder().eval()
    x = rnd(1, 64, 32, 32, seed=33).to(DEV)
    if carry:
        with torch.no_grad():
            x = make_block()(x)
        assert precision != "split" or getattr(x, "_egz_absmax", None) is not None
    g = GraphedModule(enc, (x,))
    for n, s in enumerate(SCALES):
        xi = x if s == 1.0 else x * s
        got = g(xi).clone()
        with torch.no_grad():
            want = enc(xi)
        assert torch.equal(got, want), (n, s, rel(got, want))
        assert getattr(g.static_in[0], "_egz_absmax", None) is None and not hasattr(g.static_in[0], "_egz_prepared")


@pytest.mark.parametrize("carry", [False, True], ids=["plain", "prepared"])
@pytest.mark.parametrize("precision", ["split", "f32"])
def test_graphed_module_input_scale_sp(precision, carry, monkeypatch):
    """GraphedModule over the SP model at 64 x 64, batch 1 (both encoder streams, the padded 20-channel input path).
    ``prepared``: the flow stack carries ``_egz_prepared`` (hipops.prepare_network_input) when it is handed over: the eager
    twin consumes it, the graphed object must leave it alone and keep it out of its static buffers."""
    from egaze_amd.graphs import GraphedModule
    h = _precision(monkeypatch, precision)
    model, _ = build_sp()
    model.eval()
    x_s, x_t = (t.to(DEV) for t in synth.synth_sp_batch(1, 64, seed=70)[:2])
    prepared = carry and h.prepare_network_input(x_t) is not None
    assert prepared == (carry and precision == "split")
    g = GraphedModule(model, (x_s, x_t))
    for n, s in enumerate(SCALES):
        a, b = (x_s, x_t) if s == 1.0 else (x_s * s, x_t * s)
        if prepared:
            assert h.prepare_network_input(b) is not None
        got = g(a, b).clone()
        assert hasattr(b, "_egz_prepared") == prepared      # not consumed by the hand-over
        with torch.no_grad():
            want = model(a, b)
        assert torch.equal(got, want), (n, s, rel(got, want))
        assert not any(hasattr(t, "_egz_prepared") or hasattr(t, "_egz_absmax") for t in g.static_in)


def _scale_run(pat, graphed):
    """Two eager steps, the capture and one replay on the example batch, then the example x 2^12, x 2^-12 and the example."""
    from egaze_amd.graphs import GraphedTrainStep
    step = GraphedTrainStep(pat.fwd_loss, pat.opt, pat.batches[0], warm=2, extra_params=pat.extra) if graphed else None
    res = dict(losses=[], outs=[])
    for s in (1.0, 1.0, 1.0) + SCALES:
        _train(pat, step, pat.batches[0] if s == 1.0 else pat.scaled(pat.batches[0], s), res)
    if step is not None:
        assert step.graph is not None and step.calls == 7
        assert not any(hasattr(t, "_egz_prepared") or hasattr(t, "_egz_absmax") for t in step.static_in)
        step.close()
    res["state"] = _state(pat)
    return res


@pytest.mark.parametrize("precision", ["split", "f32"])
@pytest.mark.parametrize("pattern,carry", [("lf", False), ("stream", False), ("stream", True)],
                         ids=["lf", "stream", "stream-carried"])
def test_graphed_train_step_input_scale(pattern, carry, precision, monkeypatch):
    """GraphedTrainStep over both step patterns (the targets are not scaled).  ``carried``: the stream pattern's example input
    carries the abs-max scalar of the block that produced it, at construction and at every call with the example."""
    _precision(monkeypatch, precision)
    kw = dict(carry=True) if carry else {}
    want = _scale_run(PATTERNS[pattern](lr=1e-3, **kw), False)
    got = _scale_run(PATTERNS[pattern](lr=1e-3, **kw), True)
    print(f"{pattern} {precision} carry={carry}: eager {want['losses']}, graphed {got['losses']}")
    assert got["losses"] == want["losses"]
    for n, (a, b) in enumerate(zip(got["outs"], want["outs"])):
        assert torch.equal(a, b), (n, rel(a, b))
    _assert_same_state(got["state"], want["state"])


# ============================================================================ 4. the drivers, for more than one epoch
EPOCHS = 3


def _maps(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(n, 1, 224, 224, generator=g) for k in ("im", "gt", "feat")}


def test_lf_driver_three_epochs(monkeypatch):
    """LF._run(train) / LF._run(val) on the shell of test_lf_epoch_trailing_partial_batch_and_interrupted_epoch, LF_GRAPH on
    against off: 6 full batches of 4 and one of 2 to train on, 5 + one of 3 to validate on.  At 224 x 224, the only size the
    driver runs at: its captured iteration carries the batch metric (csrc/metrics.hip), which is defined for 224 x 224 maps
    and refuses any other."""
    import egaze_amd.LF as lf_mod
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import owned_state_dict
    train = [_maps(4, 300 + k) for k in range(6)] + [_maps(2, 310)]
    val = [_maps(4, 320 + k) for k in range(5)] + [_maps(3, 330)]
    runs = []
    for graphed in (False, True):
        monkeypatch.setattr(lf_mod, "LF_GRAPH", graphed)
        torch.manual_seed(7)
        s = object.__new__(lf_mod.LF)
        s.model = build_lf().train()
        s.device = torch.device(DEV)
        s.criterion = floss().to(DEV)
        s.optimizer = FusedAdam(s.model.parameters(), lr=1e-3)
        averages = []
        for epoch in range(EPOCHS):
            s.epochnow = epoch
            averages.append(s._run(train, True, 10 ** 9))
            with torch.no_grad():
                averages.append(s._run(val, False, 10 ** 9))
        torch.cuda.synchronize()
        assert not s.optimizer.capturable and s.optimizer.step_count == EPOCHS * len(train)
        runs.append((averages, s.optimizer, owned_state_dict(s.model), s.optimizer.state_dict()))
    _assert_same_run(*runs)


def _assert_same_run(eager, graphed):
    (avg0, opt0, sd0, osd0), (avg1, opt1, sd1, osd1) = eager, graphed
    print("per-epoch averages, eager:", avg0, "graphed:", avg1)
    assert avg1 == avg0                                     # the same Python floats
    assert opt1.step_count == opt0.step_count
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(opt1, name), getattr(opt0, name)), name
    assert list(sd1) == list(sd0)
    for k in sd0:                                           # the checkpoint: parameters, running statistics, num_batches_tracked
        assert torch.equal(sd1[k], sd0[k]), k
    assert list(osd1["state"]) == list(osd0["state"])
    for i, st in osd0["state"].items():
        for k in st:
            assert torch.equal(osd1["state"][i][k], st[k]), (i, k)


@pytest.mark.parametrize("stream", ["spatial", "temporal"])
def test_stream_driver_three_epochs(stream):
    """streamtrain.train_epoch(hipgraph=True / False) + evaluate (eval mode, as it is) on in-memory loaders at 32 x 32: 5 full
    batches of 2 and one of 1 to train on, 5 + one of 1 to validate on."""
    from egaze_amd import streamtrain
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from egaze_amd.utils import owned_state_dict

    def loader(seed):
        x_s, x_t, gt, _ = synth.synth_sp_batch(11, 32, seed=seed)
        x = x_s if stream == "spatial" else x_t
        cuts = [(2 * i, 2 * i + 2) for i in range(5)] + [(10, 11)]
        return [{key_of(stream): x[a:b], "gt": gt[a:b]} for a, b in cuts]
    train, val = loader(41), loader(42)
    runs = []
    for graphed in (False, True):
        model, _ = build_stream(stream)
        opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
        crit = floss().to(DEV)
        averages = []
        for epoch in range(EPOCHS):
            averages.append(streamtrain.train_epoch(train, model, crit, opt, epoch, DEV, stream, hipgraph=graphed))
            averages.append(streamtrain.evaluate(val, model, crit, epoch, DEV, stream))
        torch.cuda.synchronize()
        assert not opt.capturable and opt.step_count == EPOCHS * len(train)
        runs.append((averages, opt, owned_state_dict(model), opt.state_dict()))
    _assert_same_run(*runs)


def _bare_at(seed=5):
    from egaze_amd.AT import AT
    from egaze_amd.functions import MSELoss
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.optim import FusedAdam
    torch.manual_seed(seed)
    at = AT.__new__(AT)
    at.lstm, at.criterion_lstm, at.device = lstmnet().to(DEV), MSELoss.apply, torch.device(DEV)
    at.optimizer_lstm = FusedAdam(at.lstm.parameters(), lr=1e-4)
    return at


def _at_epochs(at, train, val):
    averages = []
    for epoch in range(EPOCHS):
        at.epochnow = epoch
        at.lstm.train()
        averages.append(at._epoch(train, True))
        at.lstm.eval()
        with torch.no_grad():
            averages.append(at._epoch(val, False))
    torch.cuda.synchronize()
    opt = at.optimizer_lstm
    assert not opt.capturable
    return averages, opt, {k: v.detach().clone() for k, v in at.lstm.state_dict().items()}, opt.state_dict()


def _write_vectors(folder, videos, seed):
    g = torch.Generator().manual_seed(seed)
    for name, frames in videos:
        for i in range(frames):
            torch.save(torch.randn(512, generator=g).abs(), str(folder / f"fix_{name}_{i + 1:010d}.pth.tar"))
    return str(folder)


def test_at_driver_three_epochs(tmp_path, monkeypatch):
    """AT._epoch(train) / AT._epoch(val) over the file loader, AT_GRAPH on against off, and over filled ResidentLSTMDatasets
    against the file loop: two videos of 9 + 17 vectors to train on, 5 + 6 to validate on."""
    import egaze_amd.AT as at_mod
    from torch.utils.data import DataLoader
    from egaze_amd.data.LSTMdatas import lstmDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    (tmp_path / "train").mkdir()
    (tmp_path / "test").mkdir()
    tr = _write_vectors(tmp_path / "train", (("Ahmad_Pizza1", 9), ("Carlos_Tea2", 17)), 11)
    va = _write_vectors(tmp_path / "test", (("Alireza_Pizza1", 5), ("Alireza_Tea2", 6)), 12)

    def loader(ds):
        return DataLoader(dataset=ds, batch_size=1, shuffle=False, num_workers=0)
    runs = {}
    for name, graph, cls in (("eager", False, lstmDataset), ("graphed", True, lstmDataset), ("resident", True, None)):
        monkeypatch.setattr(at_mod, "AT_GRAPH", graph)
        if cls is None:
            sets = [ResidentLSTMDataset(tr).fill(DEV), ResidentLSTMDataset(va).fill(DEV)]
            assert all(ds.filled for ds in sets)
        else:
            sets = [cls(tr), cls(va)]
        runs[name] = _at_epochs(_bare_at(), loader(sets[0]), loader(sets[1]))
        assert runs[name][1].step_count == EPOCHS * (9 + 17 - 2)
        if cls is None:
            for ds in sets:
                ds.release()
    _assert_same_run(runs["eager"], runs["graphed"])
    _assert_same_run(runs["graphed"], runs["resident"])
