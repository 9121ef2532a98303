"""The late-fusion hand-over resident in HBM (``--late_resident``): every distinct file of a ``lateDataset`` -- the SP
prediction, the AT map and the ground-truth map of each frame, as ``AT.extract_late`` and the dataset preparation wrote them --
is decoded ONCE into a uint8 plane pool on the device, and a batch is one gather launch over that pool
(hipops.late_gather: the gather, the three u8 / 255 normalisations and late_fusion's two-plane concatenation).  The loop then
opens no file, decodes nothing and copies no pixel over PCIe.  DESIGN.md section 16 has the memory arithmetic.

``ResidentLateDataset.from_st`` plans the same set from a resident ST dataset without any hand-over file; its pool is written on
the device by ``AT.extract_late(into=...)`` (``gaze_full --late_handover``).

As with data.resident, a sample of this dataset is its number: the collated batch carries the numbers and the dataset,
LF's stage function turns it into tensors, and the DataLoader, its samplers and their RNG draws are the host dataset's."""
import os

import numpy as np
import torch

from .lateDataset import lateDataset
from .resident import HandoverPool, _size_of, fill_planned

COLS = 3                                    # table columns: SP prediction, AT map, ground truth


class ResidentLateDataset(HandoverPool, lateDataset):
    """``lateDataset`` whose planes live on the device.  ``decode`` selects how ``fill`` decodes ('gpu': hipops.jpeg_decode
    for the files ``sniff`` takes, the host for the rest).  Usage: ``ds.fill(device)`` once, then any DataLoader with
    ``collate_fn=ds.collate_fn`` and ``num_workers=ds.loader_workers``."""
    loader_workers = 0                      # the pool must not be pickled into a worker

    def __init__(self, *args, decode='host', **kwargs):
        super().__init__(*args, **kwargs)
        if decode not in ('host', 'gpu'):
            raise ValueError(f"decode must be 'host' or 'gpu', got {decode!r}")
        self.decode = decode
        self.collate_fn = self._collate
        self.pool = self.table = None       # device tensors after fill()
        self._plan = None

    def _files(self, index):
        return (os.path.join(self.imgPath_s, self.listFiles[index]), os.path.join(self.featPath, self.listFeat[index]),
                os.path.join(self.gtPath, self.listGtFiles[index]))

    # ------------------------------------------------------------------ plan (host only)
    def plan(self):
        """Lists the distinct files, gives each one plane of the pool and builds the (N, 3) table of plane numbers (pred, feat,
        gt).  Reads one file header for the plane size; touches no device.  Sets ``files`` [(path, plane, 1)], ``planes``,
        ``hw``, ``plane_table`` (host) and ``needed_bytes``."""
        N = len(self)
        if N == 0:
            raise RuntimeError("ResidentLateDataset.plan: no files (an empty dataset)")
        table = np.empty((N, COLS), dtype=np.int64)
        files, where = [], {}
        for c in range(COLS):               # column by column: the planes of one kind of map lie together
            for i in range(N):
                path = self._files(i)[c]
                p = where.get(path)
                if p is None:
                    p = where[path] = len(files)
                    files.append((path, p, 1))
                table[i, c] = p
        self.files = files
        self.planes = len(files)
        self.hw = _size_of(files[0][0], 1)
        self.plane_table = torch.from_numpy(table)
        self.needed_bytes = self.planes * self.hw[0] * self.hw[1] + table.nbytes
        self._plan = True
        return self

    # ------------------------------------------------------------------ planned from the ST dataset (no hand-over file)
    @classmethod
    def from_st(cls, st_dataset, task=None):
        """The set ``LF`` would build from the files ``AT.extract_late`` writes for ``st_dataset`` (a ResidentSTDataset),
        planned without touching a file: N = the samples that pass ``task``; ``plane_table`` is what plan() builds for N
        distinct files per column (pred planes 0 .. N - 1, feat planes N .. 2N - 1, gt planes 2N .. 3N - 1); ``st_index`` (N,)
        is the ST sample behind each row.  ``allocate(device)`` creates the zero-filled pool, ``AT.extract_late(into=...)``
        writes it and marks the set complete; ``gather`` refuses until then.

        The rows must be the rows ``LF`` lists: it sorts the written file names (the ``imname``s) and pairs them BY POSITION
        with the sorted ground-truth names.  So the ``imname``s must be unique, in ``sorted()`` order, and sample i's own
        ground-truth file the i-th of the dataset's sorted ground-truth list; anything else is refused, naming the first
        offending sample."""
        who = "ResidentLateDataset.from_st"
        names, gts = list(st_dataset.listTrainFiles), list(st_dataset.listGtFiles)
        if len(names) != len(gts):
            raise ValueError(f"{who}: {len(names)} images but {len(gts)} ground-truth maps")
        seen = {}
        for i, name in enumerate(names):
            if name in seen:
                raise ValueError(f"{who}: sample {i} ({name}) has the name of sample {seen[name]}: both would be written to "
                                 f"one hand-over file")
            seen[name] = i
        for i in range(1, len(names)):
            if names[i - 1] > names[i]:
                raise ValueError(f"{who}: sample {i} ({names[i]}) sorts before sample {i - 1} ({names[i - 1]}): LF lists the "
                                 f"hand-over files in sorted order")
        for i, (own, listed) in enumerate(zip(gts, sorted(gts))):
            if own != listed:
                raise ValueError(f"{who}: sample {i} ({names[i]}) has ground truth {own}, LF would pair it by position with "
                                 f"{listed}")
        keep = [i for i in range(len(names)) if task is None or task in names[i]]
        if [gts[i] for i in keep] != [g for g in gts if task is None or task in g]:
            bad = next(i for i in range(len(names)) if (task in names[i]) != (task in gts[i]))
            raise ValueError(f"{who}: task {task!r} selects sample {bad}'s image ({names[bad]}) but not its ground truth "
                             f"({gts[bad]}), or the reverse")
        N = len(keep)
        if N == 0:
            raise RuntimeError(f"{who}: no samples (an empty dataset)")
        if getattr(st_dataset, 'hw', None) is None:
            st_dataset.plan()
        kept = [names[i] for i in keep]
        ds = cls(None, st_dataset.gtPath, None, kept, [gts[i] for i in keep], list(kept))
        ds.files = None                      # nothing is decoded: extract_late writes the planes
        ds.planes = COLS * N
        ds.hw = tuple(st_dataset.hw)
        ds.plane_table = torch.arange(COLS * N, dtype=torch.int64).view(COLS, N).t().contiguous()
        ds.needed_bytes = ds.planes * ds.hw[0] * ds.hw[1] + ds.plane_table.numel() * 8
        ds.st_index = torch.tensor(keep, dtype=torch.int64)
        ds._plan = ds._handover = True
        return ds

    _READS, _WRITER = "decode", "AT.extract_late(into=...)"
    _OVER_BUDGET = "run without --late_handover (there is no partial cache)"

    def _allocation_needs(self):
        return (f"the late-fusion planes need {self.needed_bytes} bytes ({self.planes} planes of {self.hw[0]} x "
                f"{self.hw[1]})")

    def _allocate_empty(self, device):
        self.pool = torch.zeros((self.planes,) + self.hw, dtype=torch.uint8, device=device)
        self.table = self.plane_table.to(device)

    # ------------------------------------------------------------------ fill (decode once)
    def fill(self, device, budget_bytes=None, chunk=2048):
        """ResidentSTDataset.fill's rules: decodes every distinct file once, ``chunk`` files at a time, into its plane of the
        pool on ``device``; a pool that does not fit ``budget_bytes`` (None: 0.8 x the free device memory) raises before
        anything is allocated; corrupt data warns, an unsupported, unreadable or wrongly sized file raises, both naming the
        file."""
        self._refuse_fill_of_handover()
        if not self._plan:
            self.plan()
        return fill_planned(self, device, budget_bytes, chunk, "ResidentLateDataset.fill", "--late_resident")

    # ------------------------------------------------------------------ samples
    def __getitem__(self, index):
        return {'index': index}

    def _collate(self, batch):
        return {'resident': self, 'index': torch.LongTensor([s['index'] for s in batch])}

    def gather(self, sample, device, raw=False):
        """The collated ``sample`` as device tensors: ``index`` crosses PCIe (non-blocking), one gather launch follows on the
        current stream; its status word is left on ``sample`` for check_decode_status.  -> hipops.late_gather's result."""
        from .. import hipops as H
        if self.pool is None:
            raise RuntimeError("ResidentLateDataset: fill(device) has not run (the pool is not on the device)")
        if not self.filled:
            raise RuntimeError("ResidentLateDataset: the pool is allocated but AT.extract_late(into=...) has not completed it")
        if torch.device(device) != self.pool.device:
            raise RuntimeError(f"ResidentLateDataset: the pool is on {self.pool.device}, the batch is asked for on {device}")
        idx = sample['index'].to(self.pool.device, non_blocking=True)
        return H.late_gather(self.pool, self.table, idx, raw=raw, status_to=sample)
