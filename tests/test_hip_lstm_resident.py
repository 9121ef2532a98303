"""The resident LSTM vectors on the GPU (csrc/lstm_pool.hip, hipops.lstm_pool_fetch, data/lstm_resident.py, AT._epoch_resident):
the fetch kernel through the raw C-ABI against a byte-exact host mirror of every buffer it may touch, the fetch under capture,
and the training / validation epochs, the driver and the fallback against the file loader -- equal, not close."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
GUARD = 8                                     # floats between (and around) the carved ranges


# ----------------------------------------------------------------------------- the kernel, raw entry point
class _Carved:
    """inp, tgt and state carved out of ONE sentinel-filled device buffer, with a host mirror that the test updates to what a
    launch is allowed to change: comparing the two as int32 words checks every copied value, every zero and every byte
    outside the three ranges at once.  ``shift`` = 0 puts the three ranges on 16-byte boundaries (the float4 body with its
    scalar tail), 1 puts them one float off (the scalar form)."""

    def __init__(self, width, state_n, shift):
        at, spans = GUARD, []
        for n in (width, width, state_n):
            at = (at + 3) // 4 * 4 + shift
            spans.append((at, n))
            at += n + GUARD
        self.spans = spans
        self.dev = torch.full((at * 4,), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.float32)
        self.host = torch.full((at * 4,), SENTINEL, dtype=torch.uint8).view(torch.float32)
        assert (self.dev.data_ptr() + 4 * spans[0][0]) % 16 == 4 * shift

    def part(self, i, buf=None):
        o, n = self.spans[i]
        return (self.dev if buf is None else buf)[o:o + n]

    def set_state(self, value):
        self.part(2).fill_(value)
        self.part(2, self.host).fill_(value)

    def same(self):
        return torch.equal(self.dev.view(torch.int32).cpu(), self.host.view(torch.int32))


def _plan(rows, extra=()):
    """in_row == tgt_row on the first and on the last row, first -> last, last -> first, a middle row; alternating resets."""
    steps = [(0, 0, 1), (rows - 1, rows - 1, 0), (0, rows - 1, 1), (rows - 1, 0, 0), (rows // 2, 0, 1)] + list(extra)
    return tuple(torch.tensor([s[c] for s in steps], dtype=dt) for c, dt in enumerate((torch.int32, torch.int32, torch.uint8)))


def _pool(rows, width, seed):
    return torch.randn((rows, width), generator=torch.Generator().manual_seed(seed))


class _Call:
    """The raw entry point with every argument replaceable (``None`` = a null pointer) -> return code."""

    def __init__(self, pool, plan, carved, with_state=True):
        self.pool, self.plan = pool.to(DEV), tuple(t.to(DEV) for t in plan)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        c = carved
        self.args = dict(pool=self.pool.data_ptr(), rows=pool.shape[0], width=pool.shape[1], in_row=self.plan[0].data_ptr(),
                         tgt_row=self.plan[1].data_ptr(), reset=self.plan[2].data_ptr(), n_steps=self.plan[0].numel(),
                         cursor=self.cursor.data_ptr(), inp=c.part(0).data_ptr(), tgt=c.part(1).data_ptr(),
                         state=c.part(2).data_ptr() if with_state else None, state_n=c.spans[2][1] if with_state else 0,
                         status=self.status.data_ptr())

    def __call__(self, **replace):
        from egaze_amd import hipops as Hp
        a = dict(self.args, **replace)
        rc = Hp._RAW_LIB.egz_lstm_pool_fetch(a["pool"], a["rows"], a["width"], a["in_row"], a["tgt_row"], a["reset"],
                                             a["n_steps"], a["cursor"], a["inp"], a["tgt"], a["state"], a["state_n"],
                                             a["status"], Hp._stream())
        torch.cuda.synchronize()
        return rc

    def words(self):
        return self.cursor.tolist(), int(self.status.item())


@pytest.mark.parametrize("rows", [1, 2, 7])
@pytest.mark.parametrize("width", [1, 3, 4, 511, 512, 513])
def test_fetch_copies_exactly_and_touches_nothing_else(width, rows):
    pool_h, plan_h = _pool(rows, width, seed=width * 10 + rows), _plan(rows)
    n = plan_h[0].numel()
    for state_n in (None, 1, 2048, 2049):                 # None: a null state pointer with state_n = 0
        for shift in (0, 1):
            c = _Carved(width, state_n or 0, shift)
            call = _Call(pool_h, plan_h, c, with_state=state_n is not None)
            for k in range(n):
                c.set_state(3.0)
                assert call() == 0
                c.part(0, c.host).copy_(pool_h[int(plan_h[0][k])])
                c.part(1, c.host).copy_(pool_h[int(plan_h[1][k])])
                if state_n is not None and int(plan_h[2][k]):
                    c.part(2, c.host).zero_()
                assert c.same(), (state_n, shift, k)
                assert call.words() == ([k + 1, k], 0)
            # launch n_steps + 1: the cursor has left the plan
            c.set_state(3.0)
            assert call() == 0
            assert c.same() and call.words() == ([n, n - 1], 1)


@pytest.mark.parametrize("width,rows,state_n", [(513, 7, 2049), (4, 2, 1)])
@pytest.mark.parametrize("which", ["in_row", "tgt_row"])
def test_refused_steps_write_the_status_word_only(width, rows, state_n, which):
    """A plan entry equal to ``rows`` (and a negative one) is refused with word 2; the cursor does not advance, so the step
    stays refused.  A cursor moved out of the plan on top of that: word 3, the two bits being a sticky OR across launches (one
    launch cannot show both: a cursor outside the plan names no plan entry to look at).  A good launch clears nothing."""
    pool_h = _pool(rows, width, seed=3)
    plan_h = _plan(rows)
    col = 0 if which == "in_row" else 1
    plan_h[col][1] = rows
    plan_h[col][3] = -1
    n = plan_h[0].numel()
    c = _Carved(width, state_n, 0)
    call = _Call(pool_h, plan_h, c)
    c.set_state(3.0)
    assert call() == 0                                     # step 0 is good
    c.part(0, c.host).copy_(pool_h[0]); c.part(1, c.host).copy_(pool_h[0]); c.part(2, c.host).zero_()
    assert c.same() and call.words() == ([1, 0], 0)
    c.set_state(3.0)
    for _ in range(2):                                     # step 1 holds the entry == rows
        assert call() == 0
        assert c.same() and call.words() == ([1, 0], 2)
    call.cursor.copy_(torch.tensor([3, 2], dtype=torch.int32))
    assert call() == 0                                     # step 3 holds the negative entry
    assert c.same() and call.words() == ([3, 2], 2)
    for bad in (n, -1, n + 1000):
        call.cursor.copy_(torch.tensor([bad, 2], dtype=torch.int32))
        assert call() == 0
        assert c.same() and call.words() == ([bad, 2], 3)
    call.cursor.copy_(torch.tensor([2, 7], dtype=torch.int32))
    assert call() == 0                                     # a good step: fetched, and the word stays
    c.part(0, c.host).copy_(pool_h[0]); c.part(1, c.host).copy_(pool_h[rows - 1]); c.part(2, c.host).zero_()
    assert c.same() and call.words() == ([3, 2], 3)


def test_host_refusals_launch_nothing():
    width, rows, state_n = 12, 3, 5
    pool_h, plan_h = _pool(rows, width, seed=4), _plan(rows)
    c = _Carved(width, state_n, 0)
    call = _Call(pool_h, plan_h, c)
    c.set_state(3.0)
    bad = [dict(pool=None), dict(in_row=None), dict(tgt_row=None), dict(reset=None), dict(cursor=None), dict(inp=None),
           dict(tgt=None), dict(status=None), dict(width=0), dict(width=-4), dict(width=4097), dict(rows=0), dict(rows=-1),
           dict(n_steps=0), dict(n_steps=-2), dict(state_n=-1)]
    for replace in bad:
        assert call(**replace) != 0, replace
        assert c.same() and call.words() == ([0, 0], 0), replace
    from egaze_amd import hipops as Hp
    assert b"egz_lstm_pool_fetch" in Hp._RAW_LIB.egz_last_error()
    assert call(state=None, state_n=0) == 0 and call.words() == ([1, 0], 0)          # a null state is no refusal


def test_wrapper_checks_its_arguments_and_fetches():
    from egaze_amd import hipops as Hp
    rows, width = 5, 16
    pool = _pool(rows, width, seed=6).to(DEV)
    plan = tuple(t.to(DEV) for t in _plan(rows))
    ctl = torch.zeros(3, dtype=torch.int32, device=DEV)
    both, state = torch.zeros((2, 1, 1, width), device=DEV), torch.ones((2, 2, 1, 4), device=DEV)
    ok = lambda **kw: dict(dict(pool=pool, plan=plan, cursor=ctl[:2], inp=both[0], tgt=both[1], state=state, status=ctl[2:]), **kw)
    wrong = [dict(pool=pool.double()), dict(pool=pool.t()), dict(pool=pool.cpu()), dict(pool=pool[0]),
             dict(plan=plan[:2]), dict(plan=(plan[0].long(), plan[1], plan[2])), dict(plan=(plan[0], plan[1], plan[2][:-1])),
             dict(plan=(plan[0], plan[1], plan[2].cpu())), dict(cursor=ctl), dict(cursor=ctl[:2].long()),
             dict(inp=both[0, 0, 0, :-1]), dict(tgt=both[1].double()), dict(state=state.cpu()), dict(state=state[:, :, :, ::2]),
             dict(status=ctl[1:]), dict(status=ctl[2:].float()),
             dict(pool=torch.zeros((2, 4097), device=DEV), inp=torch.zeros(4097, device=DEV), tgt=torch.zeros(4097, device=DEV))]
    for kw in wrong:
        with pytest.raises(ValueError, match="lstm_pool_fetch"):
            Hp.lstm_pool_fetch(**ok(**kw))
    assert ctl.tolist() == [0, 0, 0] and float(both.abs().sum()) == 0 and float(state.min()) == 1
    Hp.lstm_pool_fetch(**ok())
    assert torch.equal(both.view(2, width), pool[[0, 0]]) and float(state.abs().sum()) == 0 and ctl.tolist() == [1, 0, 0]
    Hp.lstm_pool_fetch(**ok(state=None))
    assert torch.equal(both.view(2, width), pool[[rows - 1, rows - 1]]) and ctl.tolist() == [2, 1, 0]


def test_fetch_captured_once_walks_the_plan_on_replay():
    from egaze_amd import hipops as Hp
    rows, width = 7, 512
    pool = _pool(rows, width, seed=8).to(DEV)
    plan = tuple(t.to(DEV) for t in _plan(rows))
    ctl = torch.zeros(3, dtype=torch.int32, device=DEV)
    both, state = torch.zeros((2, 1, 1, width), device=DEV), torch.zeros((2, 2, 1, 512), device=DEV)
    fetch = lambda: Hp.lstm_pool_fetch(pool, plan, ctl[:2], both[0], both[1], state, ctl[2:])
    fetch()                                                # an eager launch first, as the training loop's warm-up steps
    assert ctl.tolist() == [1, 0, 0]
    ctl.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with Hp.capture(g, eager_arena=False):
        fetch()
    assert ctl.tolist() == [0, 0, 0]                       # the capture ran nothing
    ins, tgts, resets = (t.tolist() for t in plan)
    for k in range(5):
        state.fill_(2.0)
        g.replay()
        assert ctl.tolist() == [k + 1, k, 0]
        assert torch.equal(both[0].view(-1), pool[ins[k]]) and torch.equal(both[1].view(-1), pool[tgts[k]])
        assert float(state.abs().max()) == (0.0 if resets[k] else 2.0)
    g.replay()                                             # a sixth replay has no step left
    assert ctl.tolist() == [5, 4, 1]


# ----------------------------------------------------------------------------- the epochs
VIDEOS = (("Ahmad_Pizza1", 9), ("Carlos_Tea2", 17))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Two videos of 9 + 17 files of 512 values, written with torch.save as extractLSTMw writes them."""
    d = tmp_path_factory.mktemp("w512")
    g = torch.Generator().manual_seed(11)
    for name, frames in VIDEOS:
        for i in range(frames):
            torch.save(torch.randn(512, generator=g).abs(), str(d / f"fix_{name}_{i + 1:010d}.pth.tar"))
    return str(d)


def _bare_at(seed=5):
    """AT without its constructor (which wants an SP checkpoint): the LSTM, its loss and its optimizer, seeded."""
    from egaze_amd.AT import AT
    from egaze_amd.functions import MSELoss
    from egaze_amd.models.LSTMnet import lstmnet
    from egaze_amd.optim import FusedAdam
    torch.manual_seed(seed)
    at = AT.__new__(AT)
    at.lstm, at.criterion_lstm, at.device = lstmnet().to(DEV), MSELoss.apply, torch.device(DEV)
    at.optimizer_lstm = FusedAdam(at.lstm.parameters(), lr=1e-4)
    return at


def _loader(ds):
    return DataLoader(dataset=ds, batch_size=1, shuffle=False, num_workers=0)


def _count_fetches(monkeypatch):
    from egaze_amd import hipops as Hp
    calls, inner = [], Hp.lstm_pool_fetch
    monkeypatch.setattr(Hp, "lstm_pool_fetch", lambda *a, **kw: calls.append(1) or inner(*a, **kw))
    return calls


def _train_two_epochs(at, ds):
    at.lstm.train()
    return [at._epoch(_loader(ds), True) for _ in range(2)]


def test_train_epochs_equal_the_file_loader(folder, monkeypatch):
    import egaze_amd.AT as at_mod
    from egaze_amd.data.LSTMdatas import lstmDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    monkeypatch.setattr(at_mod, "AT_GRAPH", True)
    F = sum(n for _, n in VIDEOS)
    ref = _bare_at()
    want = _train_two_epochs(ref, lstmDataset(folder))
    calls = _count_fetches(monkeypatch)
    got_at = _bare_at()
    ds = ResidentLSTMDataset(folder).fill(DEV)
    assert ds.filled and ds.pool.shape == (F, 512) and ds.pool.dtype == torch.float32 and ds.n_steps == F - 2
    assert ds.needed_bytes == F * 512 * 4 + 9 * (F - 2)
    got = []
    for epoch in range(2):
        got_at.lstm.train()
        got.append(got_at._epoch(_loader(ds), True))
        # the warm-up steps and the capture: not one Python call per sample
        assert len(calls) == (epoch + 1) * (at_mod._GraphedSampleStep.WARM + 1)
    print("mean losses, files:", want, "resident:", got)
    assert got == want and all(np.isfinite(want)) and want[0] != want[1]
    for (name, p), q in zip(ref.lstm.named_parameters(), got_at.lstm.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(ref.optimizer_lstm.flat_m, got_at.optimizer_lstm.flat_m)
    assert torch.equal(ref.optimizer_lstm.flat_v, got_at.optimizer_lstm.flat_v)
    assert ref.optimizer_lstm.step_count == got_at.optimizer_lstm.step_count == 2 * (F - 2)
    ds.release()
    assert ds.pool is None and ds.plan is None and not ds.filled


def test_eval_epoch_equals_the_file_loader(folder, monkeypatch):
    from egaze_amd.data.LSTMdatas import lstmDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    at = _bare_at(seed=7)
    before = [p.detach().clone() for p in at.lstm.parameters()]
    at.lstmValLoader = _loader(lstmDataset(folder))
    want = at.testLSTM()
    calls = _count_fetches(monkeypatch)
    at.lstmValLoader = _loader(ResidentLSTMDataset(folder).fill(DEV))
    got = at.testLSTM()
    assert len(calls) == 4                                  # three warm-up steps and the capture
    print("mean validation loss, files:", want, "resident:", got)
    assert got == want and np.isfinite(want) and want > 0
    assert at.testLSTM() == want                            # a second epoch starts from a zeroed cursor
    for p, q in zip(at.lstm.parameters(), before):
        assert torch.equal(p, q)


@pytest.mark.parametrize("F", [2, 1])
def test_short_sets_launch_nothing(tmp_path, F, monkeypatch):
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    for i in range(F):
        torch.save(torch.ones(512), str(tmp_path / f"fix_Ahmad_Pizza1_{i + 1:010d}.pth.tar"))
    calls = _count_fetches(monkeypatch)
    at = _bare_at()
    ds = ResidentLSTMDataset(str(tmp_path)).fill(DEV)
    assert ds.filled and ds.n_steps == 0
    at.lstm.train()
    assert at._epoch(_loader(ds), True) == 0
    at.lstmValLoader = _loader(ds)
    assert at.testLSTM() == 0
    assert calls == [] and at.optimizer_lstm.step_count == 0


def test_fallback_without_the_fused_step_reads_the_files(folder, monkeypatch):
    """LSTMnet.B1_FUSED = False: the filled resident set is iterated as the file set it also is."""
    import egaze_amd.AT as at_mod
    from egaze_amd.data.LSTMdatas import lstmDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    from egaze_amd.models import LSTMnet
    monkeypatch.setattr(at_mod, "AT_GRAPH", False)          # launch by launch, on the sequence kernels
    monkeypatch.setattr(LSTMnet, "B1_FUSED", False)
    ref, got_at = _bare_at(), _bare_at()
    ref.lstm.train(); got_at.lstm.train()
    want = ref._epoch(_loader(lstmDataset(folder)), True)
    calls = _count_fetches(monkeypatch)
    ds = ResidentLSTMDataset(folder).fill(DEV)
    got = got_at._epoch(_loader(ds), True)
    assert calls == [] and got == want and np.isfinite(want)
    for p, q in zip(ref.lstm.parameters(), got_at.lstm.parameters()):
        assert torch.equal(p, q)
    got_at.lstmValLoader, ref.lstmValLoader = _loader(ds), _loader(lstmDataset(folder))
    assert got_at.testLSTM() == ref.testLSTM() and calls == []


def test_driver_resident_equals_the_file_driver(tmp_path):
    """AT(...).train() over two epochs on the folders test_hip_drivers builds: the checkpoints hold equal tensors."""
    from egaze_amd.AT import AT
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import make_layers, cfg
    from oracle import synth
    torch.manual_seed(0)
    sp = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    torch.save({'state_dict': sp.state_dict()}, str(tmp_path / "sp.pth.tar"))
    del sp
    for sub in ("train", "test"):
        d = tmp_path / "512w" / sub
        d.mkdir(parents=True)
        ins, _ = synth.synth_at_batch(6, 1, seed=1)
        for i in range(6):
            vid = "Ahmad_Pizza1" if i < 4 else "Carlos_Tea2"
            torch.save(ins[i, 0].clone(), str(d / f"fix_{vid}_{i:010d}.pth.tar"))
    saved = {}
    for resident in (False, True):
        save = tmp_path / ("save_resident" if resident else "save_files")
        save.mkdir()
        torch.manual_seed(3)                               # the LSTM's initial weights
        at = AT(pretrained_model=str(tmp_path / "sp.pth.tar"), num_epoch_lstm=2, save_path=str(save), device='0',
                lstm_data_path=str(tmp_path / "512w"), resident=resident, resident_gb=0.001 if resident else None)
        if resident:
            assert at.lstmTrainLoader.dataset.filled and at.lstmValLoader.dataset.filled
        at.train()
        if resident:                                       # the pools are released when the training is done
            assert not at.lstmTrainLoader.dataset.filled and not at.lstmValLoader.dataset.filled
        saved[resident] = {n: torch.load(str(save / n), map_location='cpu', weights_only=False)
                           for n in ("best_lstm.pth.tar", "valbest_lstm.pth.tar")}
        del at
    for n, want in saved[False].items():
        got = saved[True][n]
        assert list(got) == list(want) and len(want) == 10
        for k in want:
            assert torch.equal(got[k], want[k]), (n, k)
