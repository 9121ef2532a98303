"""The AT extraction passes sharded over ranks (AT.extract_late / extractLSTMw.extractw with ``shard=(rank, world)``): two
ranks share the one GPU of the test box over gloo (the recipe of tests/test_hip_dp.py) and must write, between them, exactly
the files a one-rank ``shard=None`` run with the same ``chunk`` writes -- byte for byte, no tolerance: chunks are dealt out by
chunk index, so every frame goes through the same launches, and every rank runs the whole LSTM chain from gathered crop means.

The runs are made once per module (tests/extract_shard_worker.py: one one-rank process, then one two-rank launch, each a
fresh child under a timeout; nothing is started after a non-zero exit status) and the tests compare the files they left."""
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "extract_shard_worker.py")
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env():
    env = dict(os.environ)
    env.update(EGAZE_SINGLE_DEVICE="1", EGAZE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("EGAZE_PRECISION", None)
    env.pop("EGAZE_STREAMS", None)
    return env


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    sys.path.insert(0, os.path.dirname(WORKER))
    try:
        import extract_shard_worker as worker
    finally:
        sys.path.pop(0)
    work = str(tmp_path_factory.mktemp("extract_shard"))
    worker.save_weights(work)
    one = subprocess.run([sys.executable, WORKER, work], env=_env(), capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stdout[-3000:] + one.stderr[-3000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                          "127.0.0.1", "--master-port", str(_free_port()), WORKER, work],
                         env=_env(), capture_output=True, text=True, timeout=600)
    assert two.returncode == 0, two.stdout[-3000:] + two.stderr[-3000:]
    return work, worker


def _files(folder):
    """{name: bytes} of a folder ({} if it was never made: a rank without a frame makes the folder but writes nothing)."""
    if not os.path.isdir(folder):
        return {}
    out = {}
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.mark.parametrize("case", ["n11", "n7"])
def test_two_ranks_write_the_one_rank_files(runs, case):
    work, worker = runs
    n, flags = worker.CASES[case]
    names = {"f%05d.png" % i for i in range(n)}
    plan_owner = {"f%05d.png" % i: (i // worker.CHUNK) % 2 for i in range(n)}
    for kind in ("pred", "feat"):
        want = _files(os.path.join(work, "one", case, kind))
        assert set(want) == names
        assert len(set(want.values())) == n                    # the reference files differ frame by frame: equality below is not vacuous
        got = [_files(os.path.join(work, "rank%d" % r, case, kind)) for r in range(2)]
        assert not set(got[0]) & set(got[1])                     # disjoint ...
        assert set(got[0]) | set(got[1]) == names                # ... and together all N names: every file exactly once
        for r in range(2):
            assert {k for k, o in plan_owner.items() if o == r} == set(got[r])      # chunk k on rank k % world
            for name, data in got[r].items():
                assert data == want[name], (kind, name, r)


def test_carried_state_shows_in_the_files(runs):
    """The equality above guards the state carried across the rank border only if that state shows in the files.  A one-rank
    run over n7 WITHOUT its first chunk forms the same chunks (3 4 5)(6) -- so its pred files are the full run's, byte for
    byte -- but starts the LSTM from zero at frame 3, which is what rank 1 would do if it did not run rank 0's part of the
    chain: the AT map of saccade frame 3 must differ."""
    work, worker = runs
    full_pred, tail_pred = (_files(os.path.join(work, tag, "n7", "pred")) for tag in ("one", "one_tail"))
    full_feat, tail_feat = (_files(os.path.join(work, tag, "n7", "feat")) for tag in ("one", "one_tail"))
    assert sorted(tail_pred) == ["f%05d.png" % i for i in range(3, 7)]
    assert all(tail_pred[k] == full_pred[k] for k in tail_pred)
    assert worker.CASES["n7"][1][2:4] == [0, 0]                 # saccade frames on both sides of the border 2|3
    assert tail_feat["f00003.png"] != full_feat["f00003.png"]


def test_one_rank_shard_equals_unsharded(runs):
    """``shard=(0, 1)`` takes the sharded code path (owned loader, windows, gather of one) without a process group."""
    work, _ = runs
    for kind in ("pred", "feat"):
        want = _files(os.path.join(work, "one", "n7", kind))
        got = _files(os.path.join(work, "one_sharded", "n7", kind))
        assert len(want) == 7 and got == want


def test_extractw_two_ranks(runs):
    work, worker = runs
    for sub in ("train", "test"):
        want = {k: torch.load(os.path.join(work, "one", "w", sub, k)) for k in sorted(os.listdir(os.path.join(work, "one", "w", sub)))}
        assert sorted(want) == ["fix_f00001.pth.tar", "fix_f00004.pth.tar"]
        assert not torch.equal(want["fix_f00001.pth.tar"], want["fix_f00004.pth.tar"])
        got = [sorted(os.listdir(os.path.join(work, "rank%d" % r, "w", sub))) for r in range(2)]
        assert got == [["fix_f00001.pth.tar"], ["fix_f00004.pth.tar"]]
        for r in range(2):
            for k in got[r]:
                v = torch.load(os.path.join(work, "rank%d" % r, "w", sub, k))
                assert v.dtype == want[k].dtype and torch.equal(v, want[k]), (sub, k)
