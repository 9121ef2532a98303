"""Host side of what the training drivers share (trainloop.py, utils.load_merged): the loaders against the literal ones the
drivers used to write out, the meters against AverageMeter, the file lists against the reference's comprehensions, the life
cycle of a captured step and the merged state-dict load.  No GPU: nothing here touches a device."""
import os

import pytest
import torch
from torch.utils.data import DataLoader, Dataset, RandomSampler, SequentialSampler


class _Plain(Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {'i': i}


class _Declaring(_Plain):
    loader_workers = 0

    @staticmethod
    def collate_fn(items):
        return {'i': [it['i'] for it in items]}


def _literal_loaders(traindata, valdata, batch_size, default):
    """SP.__init__'s loaders as they stood before trainloop.rank_loaders (``default`` was 1 in SP, 0 in LF and streamtrain)."""
    from egaze_amd import dp
    train_sampler = dp.RankShardSampler(traindata, True, batch_size) if dp.world_size() > 1 else None
    val_sampler = dp.RankShardSampler(valdata, False, batch_size, pad=False) if dp.world_size() > 1 else None
    train = DataLoader(dataset=traindata, batch_size=batch_size, shuffle=train_sampler is None,
                       sampler=train_sampler, num_workers=getattr(traindata, 'loader_workers', default),
                       pin_memory=True,
                       collate_fn=getattr(traindata, 'collate_fn', None))
    val = DataLoader(dataset=valdata, batch_size=batch_size, shuffle=False, sampler=val_sampler,
                     num_workers=getattr(valdata, 'loader_workers', default), pin_memory=True,
                     collate_fn=getattr(valdata, 'collate_fn', None))
    return train, val, train_sampler


@pytest.mark.parametrize("default", [1, 0])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("cls", [_Plain, _Declaring])
def test_rank_loaders_are_the_literal_loaders(cls, world, default, monkeypatch):
    from egaze_amd import dp, trainloop
    monkeypatch.setattr(dp, "world_size", lambda: world)
    train_set, val_set = cls(11), cls(5)
    got = trainloop.rank_loaders(train_set, val_set, 3, default)
    want = _literal_loaders(train_set, val_set, 3, default)
    assert (got[2] is None) == (want[2] is None) == (world == 1)
    assert got[2] is got[0].sampler or world == 1
    kinds = (RandomSampler, SequentialSampler) if world == 1 else (dp.RankShardSampler, dp.RankShardSampler)
    for g, w, data, kind in zip(got[:2], want[:2], (train_set, val_set), kinds):
        assert g.dataset is data
        assert g.num_workers == w.num_workers == (0 if cls is _Declaring else default)
        assert g.pin_memory is True and w.pin_memory is True
        assert g.collate_fn is w.collate_fn
        assert (g.collate_fn is _Declaring.collate_fn) == (cls is _Declaring)
        assert type(g.sampler) is type(w.sampler) is kind
        assert g.batch_sampler.batch_size == w.batch_sampler.batch_size == 3
        assert g.batch_sampler.drop_last is w.batch_sampler.drop_last is False
        torch.manual_seed(0)
        order = list(g.batch_sampler)
        torch.manual_seed(0)
        assert order == list(w.batch_sampler)
        assert sum(len(b) for b in order) == len(g.sampler)
    if world == 2:                                  # rank 0's share: padded to whole batches in training, not in validation
        assert len(got[0].sampler) == 6 and len(got[1].sampler) == 3 and got[1].sampler.shuffle is False


def test_extraction_loader_forms():
    from egaze_amd import trainloop
    for data, workers, collate in ((_Plain(4), 1, None), (_Declaring(4), 0, _Declaring.collate_fn)):
        files = trainloop.extraction_loader(data)
        assert files.num_workers == workers and files.pin_memory is True and files.collate_fn is (collate or files.collate_fn)
        assert files.batch_size == 1 and type(files.sampler) is SequentialSampler
        memory = trainloop.extraction_loader(data, workers=0)
        assert memory.num_workers == 0 and memory.pin_memory is False and memory.batch_size == 1
        assert type(memory.sampler) is SequentialSampler and (collate is None or memory.collate_fn is collate)


@pytest.mark.parametrize("weight", [1, 7])
@pytest.mark.parametrize("updates", [1, 2, 1000])
def test_epoch_meters_average_is_average_meter_avg(updates, weight):
    from egaze_amd import trainloop
    from egaze_amd.utils import AverageMeter
    g = torch.Generator().manual_seed(updates * 10 + weight)
    vals = torch.rand(updates, 3, generator=g, dtype=torch.float64).tolist()
    meters = trainloop.EpochMeters(timed=False)
    loss, auc, aae = AverageMeter(), AverageMeter(), AverageMeter()
    for a, b, c in vals:
        meters.update(a, weight, b, c)
        loss.update(a, weight)
        auc.update(b)
        aae.update(c)
    assert meters.averages() == (loss.avg, auc.avg, aae.avg)
    assert meters.batch_time.count == 0
    timed = trainloop.EpochMeters()
    timed.update(vals[0][0], weight)                 # a subset: the loss alone, as the training loops feed it
    alone = AverageMeter()
    alone.update(vals[0][0], weight)
    assert timed.averages() == (alone.avg, 0, 0) and timed.batch_time.count == 1
    assert timed.batch_time.val >= 0


def test_epoch_meters_never_updated():
    from egaze_amd import trainloop
    assert trainloop.EpochMeters().averages() == (0, 0, 0)


NAMES = ["Ahmad_American_1.png", "Ahmad_Pizza_2.png", "Alireza_American_1.png", "Alireza_Pizza_3.png", "Yin_American_9.png",
         "Yin_Pizza_10.png", "Yin_Pizza_2.png", "Carlos_Snack_1.png", "Alireza_Snack_4.png", "Ahmad_Snack_1.png",
         "Carlos_Pizza_5.png", "Alireza_American_11.png"]


def _tree(root, sub):
    folder = os.path.join(str(root), sub)
    os.makedirs(folder)
    for name in NAMES:
        open(os.path.join(folder, name), "w").close()
    return folder


@pytest.mark.parametrize("task", [None, "Pizza", "Tea"])
def test_split_by_is_the_references_comprehensions(tmp_path, task):
    from egaze_amd import trainloop
    from egaze_amd.gaze_full import _split as gaze_full_split
    from egaze_amd.LF import _split as lf_split
    folder, val_name = _tree(tmp_path, "gt"), "Alireza"
    # gaze_full.py:61-71
    listGtFiles = [k for k in os.listdir(folder) if val_name not in k]
    listGtFiles.sort()
    listValGtFiles = [k for k in os.listdir(folder) if val_name in k]
    listValGtFiles.sort()
    if task is not None:                             # LF.py:58-63
        listGtFiles = [k for k in listGtFiles if task in k]
        listValGtFiles = [k for k in listValGtFiles if task in k]
    assert trainloop.split_by(folder, val_name, task) == (listGtFiles, listValGtFiles)
    assert lf_split(folder, val_name, task) == (listGtFiles, listValGtFiles)
    assert len(listGtFiles) + len(listValGtFiles) == {None: 12, "Pizza": 5, "Tea": 0}[task]
    if task is None:
        assert trainloop.split_by(folder, val_name) == gaze_full_split(folder, val_name) == (listGtFiles, listValGtFiles)


def test_st_datasets_lists_and_prints(tmp_path, monkeypatch, capsys):
    """The STDataset pair gets the reference's lists (gaze_full.py:60-76): the sorted flow folders and the three splits."""
    import argparse
    from egaze_amd import trainloop
    import egaze_amd.data.STdatas as st
    paths = {k: _tree(tmp_path, k) for k in ("flowPath", "imagePath", "gtPath", "fixsacPath")}
    made = []

    class Recorder:
        def __init__(self, *a, **kw):
            made.append((a, kw))
    monkeypatch.setattr(st, "STDataset", Recorder)
    train, val = trainloop.st_datasets(argparse.Namespace(val_name="Yin", device="0", **paths), key="flow")
    ours = sorted(k for k in NAMES if "Yin" not in k)
    theirs = sorted(k for k in NAMES if "Yin" in k)
    common = (paths["flowPath"], paths["imagePath"], paths["gtPath"], sorted(NAMES))
    kw = dict(raw_u8=True, decode='host')
    assert made == [(common + (ours, ours, ours, paths["fixsacPath"]), kw), (common + (theirs, theirs, theirs, paths["fixsacPath"]), kw)]
    assert train.gpu_fields == val.gpu_fields == ("flow", "gt")
    assert capsys.readouterr().out == "num of training samples:  9\nnum of val samples:  3\n"
    train, val = trainloop.st_datasets(argparse.Namespace(val_name="Yin", device="0", gpu_decode=True, **paths))
    assert made[2][1] == made[3][1] == dict(raw_u8=True, decode='gpu')
    assert not hasattr(train, "gpu_fields") and not hasattr(val, "gpu_fields")


class _FakeStep:
    def __init__(self, example):
        self.shape, self.closed = tuple(example[0].shape), 0

    def close(self):
        self.closed += 1


def _replay(wanted, leave):
    from egaze_amd import trainloop
    built = []

    def build(example):
        built.append(_FakeStep(example))
        return built[-1]
    full, part = (torch.zeros(4, 3),), (torch.zeros(2, 3),)
    picks = []
    try:
        with trainloop.ReplayOrEager(wanted, build) as replay:
            assert not built                         # nothing is built before the first batch
            for example in (full, full, part, full):
                picks.append(replay.pick(tuple(example[0].shape), example))
            if leave is not None:
                raise leave
    except (RuntimeError, KeyboardInterrupt) as e:
        assert e is leave
    else:
        assert leave is None
    return built, picks, replay


@pytest.mark.parametrize("leave", [None, RuntimeError("boom"), KeyboardInterrupt()], ids=["normal", "error", "interrupt"])
def test_replay_or_eager_builds_once_and_closes_once(leave):
    built, picks, replay = _replay(True, leave)
    assert len(built) == 1 and built[0].shape == (4, 3)
    assert picks == [built[0], built[0], None, built[0]]      # another shape: eager, and no second build
    assert built[0].closed == 1 and replay.step is None


@pytest.mark.parametrize("leave", [None, RuntimeError("boom")], ids=["normal", "error"])
def test_replay_or_eager_disabled_never_builds(leave):
    built, picks, replay = _replay(False, leave)
    assert built == [] and picks == [None] * 4 and replay.step is None


def test_load_merged():
    from egaze_amd.utils import load_merged
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 2))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    new = torch.full((2, 3), 0.5)
    load_merged(net, {"0.weight": new})
    after = net.state_dict()
    assert torch.equal(after["0.weight"], new)
    for k in ("0.bias", "1.weight", "1.bias"):
        assert torch.equal(after[k], before[k]), k
    with pytest.raises(RuntimeError, match="Unexpected key"):
        load_merged(net, {"0.bias": torch.ones(2), "classifier.weight": torch.zeros(1)})
    load_merged(net, {"0.weight": new * 2, "classifier.weight": torch.zeros(1)}, strict=False)
    assert torch.equal(net.state_dict()["0.weight"], new * 2) and torch.equal(net.state_dict()["1.weight"], before["1.weight"])
    load_merged(net, {"0.weight": new * 3, "classifier.weight": torch.zeros(1)}, known_only=True)     # strict, but filtered first
    assert torch.equal(net.state_dict()["0.weight"], new * 3) and torch.equal(net.state_dict()["1.bias"], before["1.bias"])
