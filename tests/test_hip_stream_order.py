"""Stream ordering under injected delays against the serial step.

The package's launches run on several HIP streams that are ordered "with stream waits only" (streams.py, DESIGN.md "Stream
concurrency"): fork / join / detach, the shared weight-gradient stream, the end-of-backward join, the abs-max arena's event, packed
weights rebuilt in place on whichever stream asks first, prepared network inputs, the h2d stream of staged_batches, the resident
gather's events, the gradient reducer's comm stream.  None of the kernels uses a floating-point atomic, so the same step with
``streams.ENABLED = False`` (everything on one stream) is an EXACT oracle: a correctly ordered multi-stream step equals it bit for
bit however its streams are delayed.  tests/stream_perturb.py supplies the delays (bounded spin kernels), the oracle switch and
the poisoning of freed memory; every compared run poisons before each step and uses fresh inputs each step, so a read that comes
too early returns NaN / garbage and never last step's identical values.

Self-check (test_selfcheck_*): three small scenarios on long-lived, pre-allocated buffers with ONE edge removed on purpose (a fork
that is not joined; an abs-max buffer taken on a second stream without the arena's event wait; a conv launch on a forked stream
whose initial wait is gone, right after the packed weight was rebuilt in place on the parent).  Under the matching mode each must
DIFFER from serial in 10 of 10 runs at DETECT_MS, and be bit-identical in 10 of 10 with the edge restored at DELAY_MS.  A fourth
check re-creates the ADVICE r2 defect on a full step (the end-of-backward join removed) and must see it in every step.

Calibration (MI355X, GPU_MAX_HW_QUEUES=4; detection counts out of 10 per candidate delay, from ``calibrate()`` below):
  torch.cuda._sleep: 2382745 cycles per ms
  fork_copy (late_helper):        1 ms 10/10, 2 ms 10/10, 5 ms 10/10, 10 ms 10/10, 20 ms 10/10; edge restored at 2 ms: 0/10 differ
  arena_chunk (late_owner):       1 ms 10/10, 2 ms 10/10, 5 ms 10/10, 10 ms 10/10, 20 ms 10/10; edge restored at 2 ms: 0/10 differ
  repacked_weight (late_owner):   1 ms 10/10, 2 ms 10/10, 5 ms 10/10, 10 ms 10/10, 20 ms 10/10; edge restored at 2 ms: 0/10 differ
DELAY_MS is the smallest candidate of {1, 2, 5, 10, 20} ms at which every scenario is detected 10 of 10 (DETECT_MS = 1), doubled:
2 ms.

Hardware queues decide whether a delay shows anything.  The 32 streams of torch's pool and the default stream share 4 hardware
queues (measured: 8 pool streams sit on the default stream's queue, 8 on each of the other three), and two streams on one queue
run FIFO: a spin kernel on one holds the other back.  That can hide a race, never invent one -- but it hid the abs-max scenario
completely (0 of 10) when its second stream happened to share the parent's queue, which behind the rest of the suite it did.
stream_perturb.perturb therefore hands the package helper streams MEASURED to sit on queues of their own (helper_streams /
shares_queue; with them 10 of 10 again), and test_helper_streams_sit_on_hardware_queues_of_their_own pins that.

Findings.  No comparison failed: every path below is bit-identical to its serial run under all four modes, and the product code
is unchanged.  Two things the harness showed on the way: (1) the queue sharing above; (2) the SP step cannot show the ADVICE r2
defect at all -- its last backward node is the flow encoder's first block, whose channel-padded weight gradient has no gradient
sink and is joined, so the caller's stream ends up behind the weight-gradient stream with or without the end-of-backward join;
the pre-training step (last node: decoder.0, a detached fork) shows it in every step.  The AT steps fork nothing: only
'late_waiter' places delays there (the optimizer step's joins).  The whole file takes about 25 s plus the 8 s of its one RCCL worker
process on an MI355X.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import synth
from stream_perturb import HELPER_KINDS, MODES, STATS, cycles_per_ms, helper_streams, perturb, poison, serial, shares_queue

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES_MS = (1, 2, 5, 10, 20)
DETECT_MS = 1
DELAY_MS = 2 * DETECT_MS
RUNS = 10


def H():
    import egaze_amd.hipops as h
    return h


def same(a, b):
    """Bit-identical (NaN payloads included): tensors by their bytes, everything else by ==."""
    if isinstance(a, torch.Tensor):
        return (isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
    return a == b


def first_difference(got, ref):
    """Label of the first entry of two [(label, value), ...] records that differs, or None."""
    if [k for k, _ in got] != [k for k, _ in ref]:
        return "the records list different entries"
    for (k, a), (_, b) in zip(got, ref):
        if not same(a, b):
            return k
    return None


def run_under(mode, fn, delay_ms=None):
    """``fn()`` in the serial oracle configuration ('serial') or multi-stream under ``perturb(mode)``; the device is drained."""
    ctx = serial() if mode == "serial" else perturb(mode, DELAY_MS if delay_ms is None else delay_ms)
    with ctx:
        res = fn()
        torch.cuda.synchronize()
    return res


_ORACLE = {}


def oracle(key, fn):
    """The serial record of a scenario, computed once per session and shared by the four modes."""
    if key not in _ORACLE:
        _ORACLE[key] = run_under("serial", fn)
    return _ORACLE[key]


def check_modes_equal_serial(key, mode, fn, multi_stream=True):
    """The record of ``fn()`` under ``mode`` equals the serial one entry by entry, bit for bit.  ``multi_stream``: the scenario
    is known to fork / wait / pack, so every mode but 'none' must have placed delays (a hook that no longer reaches its site
    would otherwise pass for ever)."""
    from egaze_amd import streams
    assert streams.ENABLED, "the multi-stream runs need HIP-stream concurrency on (EGAZE_STREAMS is not 0)"
    ref = oracle(key, fn)
    before = STATS["delays"]
    got = run_under(mode, fn)
    placed = STATS["delays"] - before
    print(f"{key} [{mode}]: {placed} delays of {DELAY_MS} ms, {len(ref)} entries compared")
    assert placed == 0 if mode == "none" else (placed > 0 or not multi_stream), (key, mode, placed)
    assert len(ref) > 0
    diff = first_difference(got, ref)
    assert diff is None, f"{key} under mode {mode!r}: first tensor that differs from the serial step: {diff}"


# ------------------------------------------------------------------------------------------------ 2a. self-check
class ForkCopy:
    """A forked region writes ``dst``; the parent reads it.  Broken: fork.join is a no-op."""
    mode = "late_helper"

    def __init__(self):
        n = 1 << 18
        self.src = [torch.full((n,), float(k + 1), device=DEV) for k in range(RUNS)]
        self.dst = torch.empty(n, device=DEV)
        self.out = [torch.empty(n, device=DEV) for _ in range(RUNS)]

    def broken(self, mp):
        from egaze_amd import streams
        mp.setattr(streams.fork, "join", lambda self, *tensors: None)

    def run(self, k):
        from egaze_amd import streams
        h = H()
        self.dst.view(torch.int32).fill_(-1)
        self.out[k].view(torch.int32).fill_(-1)
        poison(h)
        with streams.fork("wgrad") as f:
            h.copy_into(self.dst, self.src[k])
        f.join()
        h.copy_into(self.out[k], self.dst)
        torch.cuda.synchronize()
        return self.out[k].clone()


class ArenaChunk:
    """The parent stream creates a fresh abs-max chunk (one zero fill); a second stream takes a buffer from it and folds a maximum
    in with atomic max.  Broken: the second stream is marked as having waited for the fill already."""
    mode = "late_owner"

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        self.x = [(torch.randn(1 << 16, generator=g) * (k + 1)).to(DEV) for k in range(RUNS)]
        self.s2 = helper_streams()[0]     # (measured to sit on another hardware queue than the parent stream)
        self.keep = []                    # arenas (and with them their chunks) live until the scenario is dropped
        self.skip_wait = False

    def broken(self, mp):
        mp.setattr(self, "skip_wait", True)

    def run(self, k):
        h = H()
        poison(h)
        arena = h._AbsmaxArena()
        self.keep.append(arena)
        keep, h.ABSMAX_ARENA = h.ABSMAX_ARENA, arena
        try:
            arena.take(torch.device(DEV))                       # the parent creates the chunk and records the fill's event
            if self.skip_wait:
                arena.waited.add(self.s2.cuda_stream)
            x = self.x[k].view(-1)                              # (a new tensor object: no abs-max rides on it yet)
            with torch.cuda.stream(self.s2):
                am = h.absmax_of(x)
            torch.cuda.synchronize()
            return am.clone()
        finally:
            h.ABSMAX_ARENA = keep


class RepackedWeight:
    """A weight is overwritten, its packing rebuilt in place on the parent stream, and a conv launch on a forked stream consumes
    the packing.  Broken: the fork's initial ``side.wait_stream(cur)`` is gone."""
    mode = "late_owner"
    C = K = 64

    def __init__(self):
        h = H()
        g = torch.Generator().manual_seed(4)
        self.base = torch.randn(self.K, self.C, 3, 3, generator=g).to(DEV)
        self.w = self.base.clone()
        self.x = torch.randn(2, 16, 16, self.C, generator=g).to(DEV)
        self.bias = torch.zeros(self.K, device=DEV)
        self.keep = []
        h.packed_weight(self.w, "fwd")                          # the packing exists: every later rebuild is in place
        torch.cuda.synchronize()

    def broken(self, mp):
        from egaze_amd import streams

        def enter_without_wait(f):
            if f.enabled:
                f.cur = streams.current()
                f.side = streams.side_stream(f.kind)
                streams._set_current(f.side)
            return f
        mp.setattr(streams.fork, "__enter__", enter_without_wait)

    def run(self, k):
        from egaze_amd import streams
        h = H()
        poison(h)
        torch.mul(self.base, float(k + 2), out=self.w)          # fresh weights: the packing goes stale (version counter)
        torch.cuda.synchronize()
        buf = h.packed_weight(self.w, "fwd")                    # rebuilt on the parent stream, into the existing buffer
        with streams.fork("wgrad") as f:
            wp = h.packed_weight(self.w, "fwd")                 # fresh by its tag: no launch here
            y, _ = h.conv3x3_fwd(self.x, wp, self.bias, self.K, epi=h.EPI_BIAS)
        f.join(y)
        torch.cuda.synchronize()
        assert wp.data_ptr() == buf.data_ptr()
        self.keep.append(y)
        return y.clone()


SCENARIOS = {"fork_copy": ForkCopy, "arena_chunk": ArenaChunk, "repacked_weight": RepackedWeight}


def detection(name, delay_ms, broken=True):
    """(runs that differ from serial, runs) of scenario ``name`` under its matching mode, with the edge removed or restored."""
    sc = SCENARIOS[name]()
    with serial():
        refs = [sc.run(k) for k in range(RUNS)]
    mp = pytest.MonkeyPatch()
    try:
        if broken:
            sc.broken(mp)
        differ = 0
        with perturb(sc.mode, delay_ms):
            for k in range(RUNS):
                got = sc.run(k)
                differ += 0 if same(got, refs[k]) else 1
    finally:
        mp.undo()
        torch.cuda.synchronize()
    assert all(not same(refs[k], refs[k + 1]) for k in range(RUNS - 1)), "the runs of a scenario use fresh data"
    return differ, RUNS


def calibrate():
    """Detection counts of every scenario at every candidate delay (what the module docstring quotes)."""
    lines = [f"torch.cuda._sleep: {cycles_per_ms():.0f} cycles per ms"]
    for name in SCENARIOS:
        row = [f"{ms} ms: {detection(name, ms)[0]}/{RUNS}" for ms in CANDIDATES_MS]
        lines.append(f"{name} ({SCENARIOS[name].mode}): " + ", ".join(row) + f"; restored at {DELAY_MS} ms: "
                     f"{detection(name, DELAY_MS, broken=False)[0]}/{RUNS} differ")
    return lines


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_selfcheck_missing_edge_is_seen(name):
    differ, runs = detection(name, DETECT_MS)
    print(f"{name}: {differ}/{runs} runs differ from serial with the edge removed at {DETECT_MS} ms "
          f"({cycles_per_ms():.0f} cycles per ms)")
    assert differ == runs


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_selfcheck_restored_edge_is_bit_identical(name):
    differ, runs = detection(name, DELAY_MS, broken=False)
    assert differ == 0


def test_selfcheck_end_of_backward_join_is_seen(pretrain, monkeypatch):
    """The full-step comparison sees the ADVICE r2 defect: with functions._join_at_end_of_backward gone, backward() returns while
    the detached weight-gradient stream is still writing, and the gradients read right behind it differ from serial in every step
    under 'late_helper'.  What is read early is the optimizer's flat gradient buffer, which lives as long as the optimizer;
    step() joins every helper stream itself, so everything after the read is ordered as usual and equals serial.
    (On the pre-training step, whose last backward node -- decoder.0 -- ends in a detached fork.  The SP step hides the defect:
    its last backward node is the flow encoder's first block, whose channel-padded weight gradient has no sink and is JOINED,
    and the autograd engine orders the caller's stream behind that encoder's stream.)"""
    import egaze_amd.functions as F
    key = f"pretrain_{pretrain.stream}"
    ref = oracle(key, lambda: pretrain_steps(pretrain))
    monkeypatch.setattr(F, "_join_at_end_of_backward", lambda: None)
    got = run_under("late_helper", lambda: pretrain_steps(pretrain), delay_ms=DETECT_MS)
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (k, a), (_, b) in zip(got, ref):
        assert same(a, b) == (not k.endswith("grads after backward")), k


def test_helper_streams_sit_on_hardware_queues_of_their_own():
    """With GPU_MAX_HW_QUEUES = 4 the current stream and three helper streams fit on four queues; perturb() hands exactly these to
    the package as wgrad / encoder_t / h2d, so that a delay on one of them cannot hold the others back."""
    from egaze_amd import streams
    found = helper_streams()
    assert len(found) == len(HELPER_KINDS) == 3
    cur = torch.cuda.current_stream()
    group = [cur] + found
    assert len({st.cuda_stream for st in group}) == 4
    for i, a in enumerate(group):
        for b in group[i + 1:]:
            assert not shares_queue(a, b) and not shares_queue(b, a)
    assert shares_queue(cur, cur)                                    # (the probe does see a shared queue)
    before = dict(streams._SIDE)
    with perturb("none", DELAY_MS):
        assert [streams.side_stream(k) for k in HELPER_KINDS] == found
    assert dict(streams._SIDE) == before


def test_perturb_removes_its_hooks_and_bounds_the_delay():
    from egaze_amd import streams
    h = H()
    before = (streams.fork.__enter__, torch.cuda.stream, torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event,
              h._AbsmaxArena.take, h.prepare_network_input, h.resident_gather, h.LIB.egz_pack_w3x3_split_frag, streams.ENABLED)
    for mode in MODES:
        with perturb(mode, DELAY_MS):
            pass
    with serial():
        assert not streams.ENABLED
    after = (streams.fork.__enter__, torch.cuda.stream, torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event,
             h._AbsmaxArena.take, h.prepare_network_input, h.resident_gather, h.LIB.egz_pack_w3x3_split_frag, streams.ENABLED)
    assert all(a is b for a, b in zip(before, after))
    with pytest.raises(ValueError):
        with perturb("late_helper", 20.5):
            pass


# ------------------------------------------------------------------------------------------------ 2b. SP training
def bn_stats(model):
    return [(k, v.detach().clone()) for k, v in model.state_dict().items() if "running" in k or "tracked" in k]


class Trainer:
    """A model with its FusedAdam and criterion, reset to the same initial state before every compared run."""

    def __init__(self, model, params=None, lr=1e-4):
        from egaze_amd.floss import floss
        from egaze_amd.optim import FusedAdam
        self.model = model
        model.train()
        self.opt = FusedAdam(list(model.parameters()) if params is None else list(params), lr=lr)
        self.crit = floss().to(DEV)
        self.sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        torch.cuda.synchronize()

    def reset(self):
        self.model.load_state_dict(self.sd0)            # (in place: every packing goes stale and is rebuilt in its buffer)
        self.model.train()
        self.opt.flat_m.zero_()
        self.opt.flat_v.zero_()
        self.opt.step_count = 0
        torch.cuda.synchronize()

    def grads(self):
        """Every p.grad, read on the current stream right where the caller stands (they are views of one flat buffer)."""
        o = self.opt
        for p, off in zip(o.params, o.offsets):
            assert p.grad is not None and p.grad.data_ptr() == o.flat_g.data_ptr() + 4 * off
        return o.flat_g.clone()

    def step(self, tag, forward, gt, rec, second_backward=False):
        """One training step; appends (label, value) pairs to ``rec``: the gradients IMMEDIATELY after backward() returns
        (no host wait in between), output, loss, parameters and BatchNorm statistics after step()."""
        self.opt.zero_grad()
        out = forward()
        loss = self.crit(out, gt.view(out.size()))
        loss.backward()
        rec.append((f"{tag}/grads after backward", self.grads()))
        if second_backward:                          # zero_grad() and a second backward() with no step() in between
            self.opt.zero_grad()
            out = forward()
            loss = self.crit(out, gt.view(out.size()))
            loss.backward()
            rec.append((f"{tag}/grads after the second backward", self.grads()))
        self.opt.step()
        rec.append((f"{tag}/output", out.detach().clone()))
        rec.append((f"{tag}/loss", loss.detach().clone()))
        rec.append((f"{tag}/parameters", self.opt.flat_p.clone()))
        rec += [(f"{tag}/{k}", v) for k, v in bn_stats(self.model)]


@pytest.fixture(scope="module")
def sp():
    from test_hip_model_sp import build_model
    model, _ = build_model()
    t = Trainer(model)
    t.batches = [synth.synth_sp_batch(2, 64, seed=40 + i)[:3] for i in range(3)]
    t.eval_batches = {b: synth.synth_sp_batch(b, 64, seed=50 + b)[:2] for b in (1, 2)}
    yield t
    del t
    torch.cuda.empty_cache()


def sp_steps(t, second_backward=False):
    t.reset()
    rec = []
    for i, (x_s, x_t, gt) in enumerate(t.batches):
        poison(H())
        xs, xt, g = x_s.to(DEV), x_t.to(DEV), gt.to(DEV)           # fresh inputs each step
        t.step(f"step {i}", lambda: t.model(xs, xt), g, rec, second_backward=second_backward)
        del xs, xt, g
    return rec


@pytest.mark.parametrize("mode", MODES)
def test_sp_training_steps(sp, mode):
    """model_SP + floss + FusedAdam, B = 2 at 64 x 64, three consecutive steps."""
    check_modes_equal_serial("sp", mode, lambda: sp_steps(sp))


@pytest.mark.parametrize("mode", MODES)
def test_sp_second_backward_without_step(sp, mode):
    check_modes_equal_serial("sp2", mode, lambda: sp_steps(sp, second_backward=True))


@pytest.mark.parametrize("mode", MODES)
def test_sp_sequential_encoder_issue(sp, mode, monkeypatch):
    import egaze_amd.models.model_SP as M
    monkeypatch.setattr(M, "_INTERLEAVE", False)
    check_modes_equal_serial("sp", mode, lambda: sp_steps(sp))       # (serial takes no encoder fork at all: the same oracle)


@pytest.mark.parametrize("mode", MODES)
def test_sp_joined_weight_gradient_forks(sp, mode, monkeypatch):
    import egaze_amd.functions as F
    monkeypatch.setattr(F, "DETACH_WGRAD", False)
    check_modes_equal_serial("sp", mode, lambda: sp_steps(sp))


def sp_eval_after_training(t, batch):
    """A training step, an eval forward right behind it (eval-only packings and the BatchNorm fold are rebuilt lazily), then
    another training step."""
    t.reset()
    rec = []
    (a_s, a_t, a_g), (b_s, b_t, b_g) = t.batches[0], t.batches[1]
    e_s, e_t = t.eval_batches[batch]
    poison(H())
    xs, xt, g = a_s.to(DEV), a_t.to(DEV), a_g.to(DEV)
    t.step("train 0", lambda: t.model(xs, xt), g, rec)
    t.model.eval()
    es, et = e_s.to(DEV), e_t.to(DEV)
    with torch.no_grad():
        rec.append(("eval/output", t.model(es, et).clone()))
    t.model.train()
    poison(H())
    xs, xt, g = b_s.to(DEV), b_t.to(DEV), b_g.to(DEV)
    t.step("train 1", lambda: t.model(xs, xt), g, rec)
    return rec


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [1, 2])
def test_sp_eval_forward_right_after_a_training_step(sp, batch, mode):
    check_modes_equal_serial(f"sp_eval{batch}", mode, lambda: sp_eval_after_training(sp, batch))


# ------------------------------------------------------------------------------------------------ stream pre-training
@pytest.fixture(scope="module", params=["spatial", "temporal"])
def pretrain(request):
    from test_hip_streams import build
    model, _ = build(request.param)
    t = Trainer(model, params=model.decoder.parameters())
    t.stream = request.param
    batches = [synth.synth_sp_batch(2, 64, seed=60 + i) for i in range(3)]
    t.batches = [(b[0] if request.param == "spatial" else b[1], b[2]) for b in batches]
    yield t
    del t
    torch.cuda.empty_cache()


def pretrain_steps(t, second_backward=False):
    from egaze_amd import streamtrain
    t.reset()
    rec = []
    for i, (x, gt) in enumerate(t.batches):
        poison(H())
        xd, g = x.to(DEV), gt.to(DEV)
        t.step(f"step {i}", lambda: streamtrain.step_forward(t.model, xd), g, rec, second_backward=second_backward)
        del xd, g
    return rec


@pytest.mark.parametrize("mode", MODES)
def test_stream_pretraining_steps(pretrain, mode):
    check_modes_equal_serial(f"pretrain_{pretrain.stream}", mode, lambda: pretrain_steps(pretrain))


@pytest.mark.parametrize("mode", MODES)
def test_stream_pretraining_second_backward_without_step(pretrain, mode):
    check_modes_equal_serial(f"pretrain2_{pretrain.stream}", mode, lambda: pretrain_steps(pretrain, second_backward=True))


# ------------------------------------------------------------------------------------------------ late fusion, eager
class _PoisonedLoader:
    """A list of batches as a loader that poisons before it hands out each batch (staged_batches asks for batch k + 1 before the
    consumer's step k is issued: the poison lands between two steps, the prefetch still overlaps the step)."""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            poison(H())
            yield b


@pytest.fixture(scope="module")
def lf():
    import egaze_amd.LF as lf_mod
    from test_hip_lf import build
    t = Trainer(build(), lr=1e-3)
    s = object.__new__(lf_mod.LF)
    s.model, s.device, s.criterion, s.optimizer, s.epochnow = t.model, torch.device(DEV), t.crit, t.opt, 0
    t.shell = s
    g = torch.Generator().manual_seed(21)
    t.batches = [{k: torch.rand(4, 1, 32, 32, generator=g) for k in ("im", "gt", "feat")} for _ in range(3)]
    yield t
    del t
    torch.cuda.empty_cache()


def lf_epoch(t):
    t.reset()
    loss, auc, aae = t.shell._run(_PoisonedLoader(t.batches), True, 10 ** 9)
    o = t.opt
    return [("epoch loss / AUC / AAE", (loss, auc, aae)), ("gradients of the last step", o.flat_g.clone()),
            ("parameters", o.flat_p.clone()), ("Adam m", o.flat_m.clone()), ("Adam v", o.flat_v.clone())] + bn_stats(t.model)


@pytest.mark.parametrize("mode", MODES)
def test_late_fusion_eager_steps(lf, mode, monkeypatch):
    """LF._run launch by launch (LF_GRAPH off), B = 4 at 32 x 32, three batches through staged_batches."""
    import egaze_amd.LF as lf_mod
    monkeypatch.setattr(lf_mod, "LF_GRAPH", False)
    check_modes_equal_serial("lf", mode, lambda: lf_epoch(lf))


# ------------------------------------------------------------------------------------------------ AT
@pytest.fixture(scope="module")
def at():
    from test_hip_at import build
    from egaze_amd.optim import FusedAdam
    net = build()
    net.train()
    opt = FusedAdam(net.parameters(), lr=1e-3)
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(3, 4, 512, generator=g), torch.tanh(torch.randn(3, 4, 512, generator=g))) for _ in range(3)]
    samples = [{"input": torch.randn(1, 512, generator=g), "gt": torch.rand(1, 512, generator=g),
                "same": torch.tensor([0 if i == 4 else 1])} for i in range(8)]
    yield net, opt, sd0, batches, samples
    torch.cuda.empty_cache()


def _at_reset(net, opt, sd0):
    net.load_state_dict(sd0)
    net.train()
    opt.flat_m.zero_()
    opt.flat_v.zero_()
    opt.step_count = 0
    torch.cuda.synchronize()


def at_batched_steps(at):
    from egaze_amd.functions import MSELoss
    net, opt, sd0, batches, _ = at
    _at_reset(net, opt, sd0)
    rec = []
    for i, (x, tgt) in enumerate(batches):
        poison(H())
        xd, td = x.to(DEV), tgt.to(DEV)
        h0, c0 = torch.zeros(2, 4, 512, device=DEV), torch.zeros(2, 4, 512, device=DEV)
        opt.zero_grad()
        pred, _ = net(xd, (h0, c0))
        loss = MSELoss.apply(pred, td)
        loss.backward()
        rec.append((f"step {i}/grads after backward", opt.flat_g.clone()))
        opt.step()
        rec += [(f"step {i}/prediction", pred.detach().clone()), (f"step {i}/loss", loss.detach().clone()),
                (f"step {i}/parameters", opt.flat_p.clone())]
    assert H().lstm_persist_status() == 0
    return rec


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("persistent", [True, False])
def test_at_batched_steps(at, persistent, mode, monkeypatch):
    """lstmnet + MSE + FusedAdam at T = 3, B = 4, with the persistent recurrence launches and with the wavefront launches."""
    monkeypatch.setattr(H(), "LSTM_PERSIST", persistent)
    check_modes_equal_serial(f"at_batched_{persistent}", mode, lambda: at_batched_steps(at), multi_stream=False)


def at_sample_epoch(at):
    from test_hip_at import _at_shell
    net, opt, sd0, _, samples = at
    _at_reset(net, opt, sd0)
    poison(H())
    loss = _at_shell(net, opt)._epoch(samples, True)
    return [("mean loss", loss), ("gradients of the last step", opt.flat_g.clone()), ("parameters", opt.flat_p.clone()),
            ("Adam m", opt.flat_m.clone()), ("Adam v", opt.flat_v.clone())]


@pytest.mark.parametrize("mode", MODES)
def test_at_eager_per_sample_steps(at, mode, monkeypatch):
    import egaze_amd.AT as at_mod
    monkeypatch.setattr(at_mod, "AT_GRAPH", False)
    check_modes_equal_serial("at_sample", mode, lambda: at_sample_epoch(at), multi_stream=False)


# ------------------------------------------------------------------------------------------------ staged_batches -> SP step
@pytest.fixture(scope="module")
def sp224():
    from test_hip_model_sp import build_model
    model, _ = build_model()
    t = Trainer(model)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    from test_jpeg_host import make_tree
    from egaze_amd.data.resident import ResidentSTDataset
    from egaze_amd.data.STdatas import STDataset
    args = make_tree(str(tmp_path_factory.mktemp("stream_order")))
    return {"host": STDataset(*args, raw_u8=True), "gpu": STDataset(*args, raw_u8=True, decode="gpu"),
            "resident": ResidentSTDataset(*args, raw_u8=True, decode="gpu").fill(DEV)}


def staged_sp_steps(t, ds):
    """Three batches of one 224 x 224 frame through staged_batches (the copy stream runs a batch ahead) into SP training steps."""
    from torch.utils.data import DataLoader
    from egaze_amd.data.STdatas import staged_batches
    t.reset()
    rec = []
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, pin_memory=True, collate_fn=ds.collate_fn)
    poison(H())
    for i, (sample, staged) in enumerate(staged_batches(loader, torch.device(DEV))):
        xs, xt, g = staged
        rec += [(f"batch {i}/staged {n}", v.clone()) for n, v in zip(("image", "flow", "gt"), staged)]
        t.step(f"batch {i}", lambda: t.model(xs, xt), g, rec)
        del xs, xt, g, staged
        poison(H())              # behind step i and the prefetch of batch i + 1 that ran beside it, in front of the next prefetch
    assert i == 2
    return rec


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("source", ["host", "gpu", "resident"])
def test_staged_batches_into_sp_steps(sp224, datasets, source, mode):
    check_modes_equal_serial(f"staged_{source}", mode, lambda: staged_sp_steps(sp224, datasets[source]))


# ------------------------------------------------------------------------------------------------ 2c. allocator hand-over
def detached_wgrad(k, note):
    """What functions.ConvReLU.backward does around its weight gradient, by hand: the launch on the forked helper stream, the fork
    detached with its inputs, the inputs dropped -- and same-sized tensors allocated and filled on the parent stream right behind
    the fork, which is where the caching allocator would hand the inputs' blocks (the abs-max scalars included) out again if
    fork.detach had not recorded them on the helper stream.  ``note['reused']``: how many of the two inputs' blocks the
    allocator did hand to the tensors allocated next (serial: both, they are free at once)."""
    import egaze_amd.functions as F
    from egaze_amd import streams
    h = H()
    poison(h)
    g = torch.Generator().manual_seed(70 + k)
    # 12 MiB each: above the allocator's 10 MiB bound a block is a segment of its own, so a freed one keeps its address and size
    x = torch.randn(3, 64, 64, 256, generator=g).to(DEV)
    dy = (torch.randn(3, 64, 64, 256, generator=g) * 1e-3).to(DEV)
    for t in (x, dy):
        t._egz_absmax = h.absmax_of(t).clone()                        # a block of its own (not a slice of the arena's chunk)
    sink = torch.zeros(256 * 256 * 9, device=DEV)
    torch.cuda.synchronize()
    ptrs = {x.data_ptr(), dy.data_ptr()}
    with streams.fork("wgrad") as f:
        dw = h.conv3x3_wgrad(x, dy, out=sink)
    F._close_fork(f, sink, dw, x, dy)
    h.PENDING_PRODUCER[0] = None                                      # (no gradient-sink hook follows here)
    shape, am_elems = tuple(x.shape), x._egz_absmax.numel()
    del x, dy, dw, t
    junk = [torch.full(shape, float("nan"), device=DEV) for _ in range(4)]
    junk += [torch.full((am_elems,), -1, dtype=torch.int32, device=DEV) for _ in range(64)]
    note["reused"] = len(ptrs & {j.data_ptr() for j in junk})
    streams.join_all_into_current()
    res = sink.clone()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("mode", MODES)
def test_detached_fork_inputs_survive_until_the_helper_has_run(mode):
    """fork.detach's inputs and their abs-max scalars are dropped by the parent while the (delayed) helper stream has not read
    them yet, and same-sized tensors are allocated and filled with NaN / 0xFF on the parent stream right away: the weight gradient
    equals the serial one.  (The allocator's choice is printed, not asserted: in the serial run it hands both input blocks to
    the tensors allocated next, multi-stream it holds them back until the helper stream has passed the detach.)"""
    notes = [dict() for _ in range(3)]
    ref = oracle("detached_wgrad", lambda: [detached_wgrad(k, n) for k, n in enumerate(notes)])
    serial_notes = [n.get("reused") for n in notes]
    notes = [dict() for _ in range(3)]
    got = run_under(mode, lambda: [detached_wgrad(k, n) for k, n in enumerate(notes)])
    print(f"input blocks handed out again right behind the fork: serial {serial_notes}, mode {mode}: {[n['reused'] for n in notes]}")
    for k, (a, b) in enumerate(zip(got, ref)):
        assert same(a, b), f"weight gradient {k} under mode {mode!r} differs from the serial one"
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ dp.GradReducer, world 1
@pytest.fixture(scope="module")
def rccl_digests(tmp_path_factory):
    """ONE run of tests/rccl_gpu_worker.py with its opt-in perturbation argument: after its own checks it repeats two training
    steps with the reducer attached in the serial configuration and under every mode, and writes a digest of each."""
    from test_hip_rccl import _env, _free_port
    out = str(tmp_path_factory.mktemp("rccl") / "obs.json")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "rccl_gpu_worker.py"), out, "64", "2", str(_free_port()),
           ",".join(("serial",) + MODES), str(DELAY_MS)]
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    obs = json.load(open(out))
    assert obs["grad_bit_exact"] and obs["params_bit_exact"] and obs["backend"] == "nccl" and obs["world"] == 1
    return obs["digests"]


@pytest.mark.parametrize("mode", MODES)
def test_grad_reducer_world1(rccl_digests, mode):
    ref, got = rccl_digests["serial"], rccl_digests[mode]
    assert len(ref) >= 6 and [k for k, _ in got] == [k for k, _ in ref]
    for (k, a), (_, b) in zip(got, ref):
        assert a == b, f"reducer step under mode {mode!r}: {k} differs from the serial run"
