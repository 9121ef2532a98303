"""Host side of the sharded AT extraction: the chunk-to-rank plan (dp.chunk_shards), the loader a rank builds over its own
frames, the refusals, and extractw's share of the second fixation frames.  No GPU."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset

import egaze_amd  # noqa: F401
from egaze_amd import dp
from egaze_amd import extractLSTMw as ex

GRID = [(n, chunk, world) for n in range(41) for chunk in range(1, 6) for world in range(1, 5)]


def test_chunk_shards_partition_and_ownership():
    for n, chunk, world in GRID:
        plan = dp.chunk_shards(n, chunk, world)
        own = [plan.indices(r) for r in range(world)]
        assert sorted(i for o in own for i in o) == list(range(n)), (n, chunk, world)          # a partition of range(n)
        for o in own:
            assert all(a < b for a, b in zip(o, o[1:]))                                        # increasing per rank
        n_chunks = -(-n // chunk)
        assert plan.n_chunks == n_chunks and plan.windows == -(-n_chunks // world)
        for k in range(n_chunks + world):                                                      # ... and past the last chunk
            want = range(k * chunk, min(n, (k + 1) * chunk)) if k < n_chunks else range(0)
            assert plan.owner(k) == k % world
            assert list(plan.frames(k)) == list(want)
            if k < plan.windows * world:
                assert list(plan.window(k // world, k % world)) == list(want)                  # window w = chunks w*world ...
        for r in range(world):                                                                 # the same windows on every rank
            assert [i for w in range(plan.windows) for i in plan.window(w, r)] == own[r]
            assert all(len(plan.window(w, r)) == chunk for w in range(plan.windows - 1))       # only the last window is short
        if world == 1:                                                                         # the plain chunking
            assert [list(plan.window(w, 0)) for w in range(plan.windows)] == \
                   [list(range(s, min(n, s + chunk))) for s in range(0, n, chunk)]


def test_chunk_shards_refuses_bad_arguments():
    for bad in ((10, 0, 2), (10, -1, 2), (10, 3, 0), (10, 3, -2), (-1, 3, 2)):
        with pytest.raises(ValueError):
            dp.chunk_shards(*bad)
    plan = dp.chunk_shards(10, 3, 2)
    for r in (-1, 2, 5):
        with pytest.raises(ValueError):
            plan.indices(r)
        with pytest.raises(ValueError):
            plan.window(0, r)
    with pytest.raises(ValueError):
        plan.window(plan.windows, 0)
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            dp.check_shard(bad)
    with pytest.raises(ValueError, match="process group"):          # two ranks claimed, no process group behind them
        dp.check_shard((1, 2))
    assert dp.check_shard((0, 1)) == (0, 1)


class _Flags(Dataset):
    def __init__(self, flags):
        self.fixsac = np.asarray(flags, dtype=float)

    def __len__(self):
        return len(self.fixsac)

    def __getitem__(self, i):
        rs = np.random.RandomState(100 + i)
        return {"fixsac": torch.FloatTensor([self.fixsac[i]]), "imname": "vid_%05d.jpg" % i,
                "image": torch.from_numpy(rs.standard_normal((3, 224, 224)).astype(np.float32)),
                "gt": torch.from_numpy(rs.uniform(size=(1, 224, 224)).astype(np.float32))}


def _collate(batch):
    out = torch.utils.data.default_collate(batch)
    out["collated_here"] = True
    return out


def test_owned_loader_keeps_the_loader_and_walks_own_frames():
    ds = _Flags([0] * 9)
    base = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, pin_memory=False, collate_fn=_collate)
    own = dp.owned_loader(base, dp.chunk_shards(9, 2, 2).indices(1))
    assert own.batch_size == 1 and own.collate_fn is _collate and own.num_workers == 0 and own.pin_memory is False
    got = list(own)
    assert [s["imname"][0] for s in got] == ["vid_%05d.jpg" % i for i in (2, 3, 6, 7)]
    assert all(s["collated_here"] for s in got)
    with pytest.raises(ValueError, match="batch size"):
        dp.owned_loader(DataLoader(ds, batch_size=2), [0])
    with pytest.raises(TypeError, match="DataLoader"):
        dp.owned_loader([ds[0]], [0])


def test_extract_late_refuses_a_shuffling_loader(tmp_path):
    """Refused before anything is touched: no model, no device, no output folder."""
    from egaze_amd.AT import AT
    at = AT.__new__(AT)
    pred, feat = str(tmp_path / "pred"), str(tmp_path / "feat")
    with pytest.raises(ValueError, match="shuffles.*dataset index"):
        at.extract_late(DataLoader(_Flags([0, 1, 0]), batch_size=1, shuffle=True), pred, feat, chunk=2, shard=(0, 1))
    assert not os.path.exists(pred) and not os.path.exists(feat)


class _Fake(torch.nn.Module):
    def forward(self, x):
        p = torch.nn.functional.avg_pool2d(x, 16)
        k = torch.arange(512, dtype=torch.float32).view(1, 512, 1, 1)
        return torch.relu(p[:, 0:1] * torch.sin(k * 0.37) + p[:, 1:2] * torch.cos(k * 0.11) + p[:, 2:3] * 0.5)


def test_extractw_shards_the_second_fixation_frames(tmp_path, monkeypatch):
    flags = [0, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1]             # second frames: 2, 6, 10, 15
    assert ex.fixation_second_frames(flags) == [2, 6, 10, 15]
    with pytest.raises(RuntimeError):
        ex.fixation_second_frames([1, 0])
    ds = _Flags(flags)
    loader = DataLoader(ds, batch_size=1, shuffle=False)
    ex.extractw(loader, _Fake(), str(tmp_path / "one"), device="cpu")
    want = {k: torch.load(str(tmp_path / "one" / k)) for k in sorted(os.listdir(str(tmp_path / "one")))}
    assert sorted(want) == ["fix_vid_%05d.pth.tar" % i for i in (2, 6, 10, 15)]
    ex.extractw(loader, _Fake(), str(tmp_path / "s01"), device="cpu", shard=(0, 1))
    assert sorted(os.listdir(str(tmp_path / "s01"))) == sorted(want)
    loaded = []
    real = _Flags.__getitem__
    monkeypatch.setattr(_Flags, "__getitem__", lambda self, i: (loaded.append(i), real(self, i))[1])
    for r, mine in ((0, (2, 15)), (1, (6,)), (2, (10,))):             # rank r takes (2, 6, 10, 15)[r::3]
        monkeypatch.setattr(dp, "world_size", lambda: 3)                  # a rank's place, without a process group: no collective runs
        monkeypatch.setattr(dp, "rank", lambda r=r: r)
        del loaded[:]
        out = str(tmp_path / ("r%d" % r))
        ex.extractw(loader, _Fake(), out, device="cpu", shard=(r, 3))
        assert tuple(loaded) == mine                                      # loads its own frames and no others
        assert sorted(os.listdir(out)) == ["fix_vid_%05d.pth.tar" % i for i in mine]
        for k in os.listdir(out):
            assert torch.equal(torch.load(os.path.join(out, k)), want[k])
    with pytest.raises(ValueError, match="fixsac"):                       # flags only reachable by loading every frame
        ex.extractw(DataLoader([ds[0], ds[1]], batch_size=1), _Fake(), str(tmp_path / "x"), device="cpu", shard=(0, 1))
    with pytest.raises(ValueError, match="shuffles"):
        ex.extractw(DataLoader(ds, batch_size=1, shuffle=True), _Fake(), str(tmp_path / "y"), device="cpu", shard=(0, 1))
