"""Worker of tests/test_hip_extract_sharded.py: runs the AT extraction passes on seeded in-memory frames and leaves the files
for the test to compare.  argv: workdir.  ``workdir`` holds sp.pth.tar / lstm.pth.tar (saved once by the test).

  * started directly: the one-rank runs -- ``shard=None`` for every case (the reference files) into workdir/one/..., ``shard=(0, 1)``
    for the small one (one_sharded/), the small one without its first chunk (one_tail/), the unsharded extractw (one/w/)
  * started by torch.distributed.run with two ranks (both on GPU 0, gloo): the same cases with ``shard=(rank, world)`` into
    workdir/rank<r>/...

Every run of one process goes through the SAME ``AT`` object, one after the other, as gaze_full.main does (val, then train)."""
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 3
# 1 = fixation frame, 0 = saccade frame (the LSTM branch).  Chunks of 3 are dealt 0, 1, 0, 1 to two ranks.
CASES = {
    # chunks (1 1 0)(0 0 0)(1 1 1)(0 0): saccade frames on both sides of the border 2|3 (a chunk and a rank border), an
    # all-saccade chunk, a chunk without a saccade frame (no LSTM call: the state passes it untouched)
    "n11": (11, [1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0]),
    # chunks (0 1 0)(0 0 1)(0): in the last window rank 0 has one frame and rank 1 none
    "n7": (7, [0, 1, 0, 0, 0, 1, 0]),
}
EXTRACTW_FLAGS = [1, 1, 0, 1, 1]          # N = 5: two fixations, second frames 1 and 4 -> one per rank


class Frames(Dataset):
    """Seeded 224 x 224 frames in memory, in STDataset's sample layout: ``raw`` = uint8 fields (raw_u8=True, what gaze_full
    hands to extract_late), else the normalised fp32 fields.  ``fixsac`` per sample is kept as STDataset keeps it."""

    def __init__(self, flags, seed, raw=True):
        from oracle import synth
        n = len(flags)
        rs = np.random.RandomState(seed)
        self.image = torch.from_numpy(rs.randint(0, 256, (n, 3, 224, 224)).astype(np.uint8))
        self.flow = torch.from_numpy(rs.randint(0, 256, (n, 20, 224, 224)).astype(np.uint8))
        self.gt = torch.from_numpy(np.round(synth.synth_gt(n, 224, rs) * 255).astype(np.uint8))
        self.fixsac = np.asarray(flags, dtype=float)
        self.raw = raw

    def __len__(self):
        return len(self.fixsac)

    def __getitem__(self, i):
        image, flow, gt = self.image[i], self.flow[i], self.gt[i]
        if not self.raw:
            image, flow, gt = image.float() / 255 - 0.45, flow.float() / 255 - 0.5, gt.float() / 255
        return {'image': image, 'flow': flow, 'gt': gt, 'fixsac': torch.FloatTensor([self.fixsac[i]]),
                'imname': 'f%05d.png' % i}


def save_weights(workdir):
    """Random-initialised model_SP and lstmnet from fixed seeds (variance-preserving, so the gaze maps are not flat)."""
    from oracle import egaze_oracle as O
    from oracle import synth
    torch.save({'state_dict': synth.synth_state_dict(O.sp_shapes(), seed=1, head_gain=0.25)}, os.path.join(workdir, "sp.pth.tar"))
    torch.save(synth.synth_state_dict(O.lstm_shapes(), seed=2), os.path.join(workdir, "lstm.pth.tar"))
    for sub in ("train", "test"):                      # AT's constructor lists the LSTM training folders
        os.makedirs(os.path.join(workdir, "512w", sub))
        for i in range(2):
            torch.save(torch.zeros(512), os.path.join(workdir, "512w", sub, f"fix_v_{i:010d}.pth.tar"))


def main():
    workdir = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import egaze_amd  # noqa: F401
    from egaze_amd.AT import AT
    from egaze_amd.extractLSTMw import extract_LSTM_training_data

    sp = os.path.join(workdir, "sp.pth.tar")
    at = AT(pretrained_model=sp, pretrained_lstm=os.path.join(workdir, "lstm.pth.tar"), save_path=workdir, device='0',
            lstm_data_path=os.path.join(workdir, "512w"))

    def late(tag, case, shard, start=0):
        n, flags = CASES[case]
        out = os.path.join(workdir, tag, case)
        at.extract_late(DataLoader(Subset(Frames(flags, seed=40 + n), range(start, n)), batch_size=1, shuffle=False),
                        os.path.join(out, "pred") + "/", os.path.join(out, "feat") + "/", chunk=CHUNK, shard=shard)

    def lstm_data(tag, shard):
        ds = Frames(EXTRACTW_FLAGS, seed=77, raw=False)
        extract_LSTM_training_data(save_path=os.path.join(workdir, tag, "w"), trained_model=sp, device='0', traindata=ds,
                                   valdata=ds, **({} if shard is None else {"shard": shard}))

    if world == 1:
        for case in CASES:
            late("one", case, None)
        late("one_sharded", "n7", (0, 1))
        late("one_tail", "n7", None, start=CHUNK)      # the same chunks from chunk 1 on, the LSTM state starting at zero there
        lstm_data("one", None)
    else:
        for case in CASES:
            late("rank%d" % rank, case, (rank, world))
        lstm_data("rank%d" % rank, (rank, world))
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
