"""The launch status word of the six ops that end in one (resident_gather, resident_gather_aug, late_gather, late_input,
late_store, lstm_store) on the GPU: the same call with and without ``status_to`` gives the same bits and
the same judgement, what is left under the documented key is still ``(pinned host word, event)``, a number out of range is
left for the caller with ``status_to`` and judged with today's text, and one drain judges the words of several chunks after
one wait.  A number out of range is never dereferenced by these kernels (their own tests assert that); this file looks at
the word only.  Inputs are the smallest the ops' own tests use."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def H():
    from egaze_amd import hipops
    return hipops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Op:
    """One op: ``run(status_to, bad)`` launches it on fixed inputs (``bad``: with one number out of range) -> (outputs,
    destination or None); ``key``; ``wait(pending)`` -> the word; ``judge(pending)`` the op's deferred rule."""
    bad_kind, destination = RuntimeError, False


class _Gather(_Op):
    key, bad_word, bad_text = '_resident_status', 1, "resident_gather: a sample number .idx. outside the table: the sample was skipped"
    cols, Hh, Ww, P, N = 22, 6, 8, 11, 5

    def __init__(self):
        g = _gen(3)
        self.pool = torch.randint(0, 256, (self.P, self.Hh, self.Ww), dtype=torch.uint8, generator=g).to(DEV)
        table = torch.randint(0, self.P, (self.N, self.cols), dtype=torch.int64, generator=g)
        if self.cols == 22:
            table[:, 0] = torch.randint(0, self.P - 2, (self.N,), generator=g)      # the image takes three planes
        self.table = table.to(DEV)

    def idx(self, bad):
        return torch.tensor([4, self.N if bad else 1, 0], dtype=torch.int64, device=DEV)

    def good(self, outs):                                  # the samples a bad call still defines
        return [o[[0, 2]] for o in outs]

    def launch(self, idx, status_to):
        return H().resident_gather(self.pool, self.table, idx, status_to=status_to)

    def run(self, status_to, bad=False):
        return [o for o in self.launch(self.idx(bad), status_to) if o is not None], None

    def wait(self, pending):
        return H().LaunchStatus(*pending).wait()

    def judge(self, pending):
        H().check_resident_status(pending)


class _GatherAug(_Gather):
    def launch(self, idx, status_to):
        return H().resident_gather_aug(self.pool, self.table, idx, H().AugSpec(flip=0.5, shift=1, contrast=0.1, seed=7), 2,
                                       status_to=status_to)


class _LateGather(_Gather):
    cols = 3

    def launch(self, idx, status_to):
        return H().late_gather(self.pool, self.table, idx, status_to=status_to)


class _LateInput(_Op):
    """No number goes into late_input: what its word reports is a value outside [0, 1], and its rule warns."""
    key, bad_word, bad_text, bad_kind = '_late_input_status', 2, r"late_input: a value outside \[0, 1\] was clamped", RuntimeWarning

    def __init__(self):
        self.sp, self.at = torch.rand((2, 8, 8), generator=_gen(1)).to(DEV), torch.rand((2, 8, 8), generator=_gen(2)).to(DEV)
        self.at_bad = self.at.clone()
        self.at_bad[1, 3, 3] = 1.5

    def run(self, status_to, bad=False):
        return list(H().late_input(self.sp, self.at_bad if bad else self.at, want_u8=True, status_to=status_to)), None

    def good(self, outs):
        return [o[:1] for o in outs]

    def wait(self, pending):
        return H().late_input_status(pending)

    def judge(self, pending):                              # predict.py reads the word and lets it be; the immediate call warns
        H().check_late_store_status(H().late_input_status(pending), who="late_input")


class _LateStore(_Op):
    key, bad_word, bad_text, destination = '_late_store_status', 4, r"late_store: a plane number outside its pool \(that sample wrote nothing\)", True
    n, HW, P = 2, (8, 8), 8

    def __init__(self):
        self.sp, self.at = torch.rand((2, 8, 8), generator=_gen(1)).to(DEV), torch.rand((2, 8, 8), generator=_gen(2)).to(DEV)
        self.gt_pool = torch.randint(0, 256, (3, 8, 8), dtype=torch.uint8, generator=_gen(3)).to(DEV)
        self.gt_src = torch.tensor([2, 0], dtype=torch.int64, device=DEV)

    def run(self, status_to, bad=False, dst=None):
        pool = torch.full((self.P,) + self.HW, FILL, dtype=torch.uint8, device=DEV)
        if dst is None:
            dst = torch.tensor([[5, 0, 3], [self.P if bad else 1, 7, 2]], dtype=torch.int64)
        out = H().late_store(self.sp, self.at, pool, dst, gt_pool=self.gt_pool, gt_src=self.gt_src, status_to=status_to)
        assert out is pool
        return [pool], pool

    def good(self, outs):
        return [outs[0][[5, 0, 3]]]                        # the first sample's planes

    def untouched(self, pool):
        return bool((pool[[1, 2, 4, 6, 7]] == FILL).all())  # the bad sample wrote none of its three planes

    def wait(self, pending):
        return H().late_store_status(pending)

    def judge(self, pending):
        H().check_late_store_status(H().late_store_status(pending))


class _LstmStore(_Op):
    key, bad_word, bad_text, destination = '_lstm_store_status', 1, r"lstm_store: a ground-truth plane number or a pool row outside its pool", True

    def __init__(self):
        self.feat = torch.randn((2, 14, 14, 8), generator=_gen(4)).to(DEV)
        self.gt_pool = torch.randint(0, 256, (2, 224, 224), dtype=torch.uint8, generator=_gen(5)).to(DEV)
        self.gt_src = torch.tensor([1, 0], dtype=torch.int64, device=DEV)

    def run(self, status_to, bad=False):
        pool = torch.full((4, 8), float("nan"), device=DEV)
        out = H().lstm_store(self.feat, self.gt_pool, self.gt_src, pool, torch.tensor([2, 4 if bad else 0]), 3, status_to=status_to)
        assert out is pool
        return [pool], pool

    def good(self, outs):
        return [outs[0][2:3]]

    def untouched(self, pool):
        return bool(torch.isnan(pool[[0, 1, 3]]).all())

    def wait(self, pending):
        return H().lstm_store_status(pending)

    def judge(self, pending):
        H().check_lstm_store_status(H().lstm_store_status(pending))


OPS = {"resident_gather": _Gather, "resident_gather_aug": _GatherAug, "late_gather": _LateGather, "late_input": _LateInput,
       "late_store": _LateStore, "lstm_store": _LstmStore}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module", params=sorted(OPS))
def op(request):
    return OPS[request.param]()


def test_the_same_call_with_and_without_status_to(op):
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # the immediate call judges its word here: clean inputs, no warning
        now, _ = op.run(None)
    status = {}
    later, _ = op.run(status)
    assert list(status) == [op.key]
    assert _same(now, later)
    assert op.wait(status[op.key]) == 0                    # ... and the deferred word is the one it judged
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        op.judge(status[op.key])


def test_what_is_left_under_the_key_is_a_pinned_word_and_an_event(op):
    status = {}
    op.run(status)
    pending = status[op.key]
    host, event = pending                                  # the old contract: a pair
    assert isinstance(pending, tuple) and len(pending) == 2 and pending[0] is host and pending[1] is event
    assert isinstance(host, torch.Tensor) and host.dtype == torch.int32 and tuple(host.shape) == (1,)
    assert host.is_pinned() and not host.is_cuda
    assert isinstance(event, torch.cuda.Event)
    event.synchronize()
    assert int(pending[0][0]) == 0 and event.query()


def test_a_number_out_of_range_is_left_for_the_caller_and_judged_with_todays_text(op):
    clean, _ = op.run({})
    status = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        outs, destination = op.run(status, bad=True)       # the call itself neither raises nor warns
    assert op.wait(status[op.key]) == op.bad_word
    assert _same(op.good(outs), op.good(clean))            # what the word does not cover is what the clean call gave
    if op.destination:
        assert op.untouched(destination)
    if op.bad_kind is RuntimeWarning:
        with pytest.warns(RuntimeWarning, match=op.bad_text):
            op.judge(status[op.key])
        with pytest.warns(RuntimeWarning, match=op.bad_text) as seen:
            op.run(None, bad=True)                         # the immediate call judges the same word the same way
        assert seen[0].filename == __file__                # ... and the warning points at the op's caller
    else:
        with pytest.raises(RuntimeError, match=op.bad_text):
            op.judge(status[op.key])
        with pytest.raises(RuntimeError, match=op.bad_text):
            op.run(None, bad=True)


# ----------------------------------------------------------------------------- the drain
def _chunks(bad_chunk=None):
    """Three chunks as an ``into=`` extraction queues them: a gather and a late_store per chunk, every word left in the chunk's
    dict.  -> ([(who, status)], the pools)."""
    gather, store = _Gather(), _LateStore()
    chunks, pools = [], []
    for k in range(3):
        status = {}
        gather.run(status)
        dst = torch.tensor([[5, 0, 3], [store.P + 1 if k == bad_chunk else 1, 7, 2]], dtype=torch.int64)
        pools.append(store.run(status, dst=dst)[1])
        assert sorted(status) == ['_late_store_status', '_resident_status']
        chunks.append((f"chunk {k}", status))
    return chunks, pools


def _drain(chunks):
    h, waits = H(), []
    h.drain_status(chunks, '_late_store_status', lambda pending: waits.append(pending) or h.late_store_status(pending),
                   h.check_late_store_status, h.judge_resident_status)
    return waits


def test_drain_waits_once_and_passes_clean_chunks():
    chunks, pools = _chunks()
    waits = _drain(chunks)
    assert len(waits) == 1 and waits[0] is chunks[-1][1]['_late_store_status']
    assert all(not bool((p[[5, 0, 3, 1, 7, 2]] == FILL).flatten(1).all(1).any()) for p in pools)      # every named plane was written
    assert _drain([]) == []                                # nothing queued: nothing to wait for


def test_drain_names_the_chunk_whose_word_is_up():
    chunks, pools = _chunks(bad_chunk=1)
    with pytest.raises(RuntimeError, match=r"^chunk 1: a plane number outside its pool"):
        _drain(chunks)
    assert bool((pools[1][[1, 7, 2]] == FILL).all())       # the middle chunk's second sample wrote nothing
    assert [int(s['_late_store_status'][0][0]) for _, s in chunks] == [0, 4, 0]
    assert len(_drain([chunks[0], chunks[2]])) == 1        # the clean chunks around it raise nothing


def test_drain_judges_the_gather_before_the_store():
    gather, store = _Gather(), _LateStore()
    status = {}
    gather.launch(gather.idx(True), status)
    store.run(status, bad=True)
    with pytest.raises(RuntimeError, match="resident_gather: a sample number"):
        _drain([("chunk 0", status)])
