"""The AT stage's LSTM vectors resident in HBM (``--lstm_resident``): every ``fix_*.pth.tar`` vector of a ``lstmDataset`` folder
is read ONCE into an fp32 pool on the device, and each step of ``AT.trainLSTM`` / ``AT.testLSTM`` fetches its input, its target
and its state reset there (hipops.lstm_pool_fetch, captured at the head of the step's hipGraph, stepping off a cursor on the
device).  The loop then unpickles no file and copies no vector over PCIe.  DESIGN.md section 17 has the plan derivation.

Unlike data.resident / data.late_resident a sample of this dataset is NOT its number: ``__getitem__`` is lstmDataset's, so the
dataset is also the file set -- what AT iterates before ``fill()``, after ``release()`` and wherever the fused single-step path
is off.

``ResidentLSTMDataset.from_st`` plans the same set from a resident ST dataset without any ``fix_*.pth.tar`` file; its pool is
written on the device by ``extractLSTMw.extractw(into=...)`` (``gaze_full --lstm_handover``)."""
import os

import numpy as np
import torch

from .LSTMdatas import deferred_steps, lstmDataset
from .resident import HandoverPool, resident_budget

FILL_THREADS = 16                           # file reads of fill() in flight at most
VECTOR_WIDTH = 512                          # channels of conv5_3: the length of an extracted vector (a from_st set has no file to ask)


def lstm_plan(listFiles):
    """The steps of one epoch over the sorted file list, from the names alone -> (in_row, tgt_row int32, reset uint8), one entry
    per step.  The schedule is LSTMdatas.deferred_steps, the one the file loop runs (AT._epoch_graphed), fed with file rows in
    place of vectors: sample i is (file i, file i + 1, lstmDataset's ``same`` flag).  Step k = 1 .. F - 2 therefore reads file
    k - 1 as its input and file k + 1 as its target, and resets the state first where file k - 1 and file k belong to
    different videos, or nothing ran before (k = 1).  Fewer than three files: no step."""
    samples = ((i, i + 1, listFiles[i + 1][:-14] == listFiles[i][:-14]) for i in range(len(listFiles) - 1))
    steps = np.array(list(deferred_steps(samples)), dtype=np.int64).reshape(-1, 3)
    return steps[:, 0].astype(np.int32), steps[:, 1].astype(np.int32), steps[:, 2].astype(np.uint8)


class ResidentLSTMDataset(HandoverPool, lstmDataset):
    """``lstmDataset`` whose vectors can live on the device.  Usage: ``ds.fill(device)`` once; AT._epoch then runs the plan
    (``pool`` (F, W) fp32, ``plan`` = (in_row, tgt_row, reset) on the device, ``n_steps``) instead of iterating the files."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pool = self.plan = None        # device tensors after fill()
        self.plan_host = lstm_plan(self.listFiles)
        self.n_steps = len(self.plan_host[0])
        self.needed_bytes = None            # known once the first file gave the vector length

    # ------------------------------------------------------------------ planned from the ST dataset (no vector file)
    @classmethod
    def from_st(cls, st_dataset, task=None):
        """The set ``lstmDataset(folder, task)`` would list after ``extractLSTMw.extractw`` had written its files for
        ``st_dataset`` (an STDataset: ``fixsac``, ``listTrainFiles``), planned without looking at a folder.  The extracted
        frames are the second frames of the fixations (a one-frame fixation raises the file path's RuntimeError here, before
        anything is allocated); frame ``imname`` is file ``'fix_' + imname[:-4] + '.pth.tar'``; ``task`` keeps the names that
        contain it; ``listFiles`` is the sorted names, and the row of a frame is its name's position there -- whatever the
        order of the dataset.  Two frames with one name are refused (the file path would keep the later one only).
        Sets ``plan_host`` = lstm_plan(listFiles), ``n_steps``, ``st_index`` (F,) int64, the ST sample behind each row, and
        ``needed_bytes`` = F x 512 x 4 + 9 n_steps.  ``allocate(device)`` creates the zero-filled pool, ``extractw(into=...)``
        writes it and marks the set complete; ``filled`` is False until then."""
        from ..extractLSTMw import fixation_second_frames
        who = "ResidentLSTMDataset.from_st"
        names, flags = list(st_dataset.listTrainFiles), list(st_dataset.fixsac)
        if len(flags) < len(names):
            raise ValueError(f"{who}: {len(names)} frames but {len(flags)} fixation flags")
        rows, seen = [], {}
        for i in fixation_second_frames(flags[:len(names)]):
            name = 'fix_' + names[i][:-4] + '.pth.tar'
            if name in seen:
                raise ValueError(f"{who}: sample {i} ({names[i]}) has the name of sample {seen[name]}: both would be written "
                                 f"to {name}")
            seen[name] = i
            if task is None or task in name:
                rows.append((name, i))
        rows.sort()
        ds = cls.__new__(cls)
        ds.Path = None                          # no folder: the vectors exist in device memory only
        ds.listFiles = [name for name, _ in rows]
        ds.pool = ds.plan = None
        ds.plan_host = lstm_plan(ds.listFiles)
        ds.n_steps = len(ds.plan_host[0])
        ds.width = VECTOR_WIDTH
        ds.st_index = torch.tensor([i for _, i in rows], dtype=torch.int64)
        ds.needed_bytes = len(rows) * ds.width * 4 + 9 * ds.n_steps
        ds._handover = True
        return ds

    _READS, _WRITER, _RELEASE_FIRST = "read", "extractLSTMw.extractw(into=...)", True
    _OVER_BUDGET = "raise --gpu_resident_gb or run without --lstm_handover"

    def _refuse_allocation(self, who):
        if not self.listFiles:
            raise RuntimeError(f"{who}: no vectors (no second fixation frame passes the task filter)")

    def _allocation_needs(self):
        return f"{len(self.listFiles)} vectors of {self.width} need {self.needed_bytes} bytes"

    def _allocate_empty(self, device):
        self.pool = torch.zeros((len(self.listFiles), self.width), dtype=torch.float32, device=device)
        self.plan = tuple(torch.from_numpy(a).to(device) for a in self.plan_host)

    def __getitem__(self, index):
        """lstmDataset's sample.  A from_st set has no files: it serves the same dict from its pool rows (a read-back per
        sample; only AT's paths beside the resident loop come here), and raises once the pool is gone."""
        if not self._handover:
            return super().__getitem__(index)
        if not self.filled:
            raise RuntimeError("ResidentLSTMDataset: the vectors of an in-memory hand-over (from_st, --lstm_handover) exist in "
                               "device memory only, and the pool " +
                               ("is not there (released, or never allocated)" if self.pool is None
                                else "has not been completed by extractw(into=...)"))
        if not 0 <= index < len(self):
            raise IndexError(index)
        a, b = self.listFiles[index], self.listFiles[index + 1]
        pair = self.pool[index:index + 2].cpu()
        return {'input': pair[0].clone(), 'gt': pair[1].clone(), 'same': b[:-14] == a[:-14]}

    def _read(self, name, want=None):
        v = torch.load(os.path.join(self.Path, name), map_location='cpu')
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
            raise ValueError(f"ResidentLSTMDataset.fill: {os.path.join(self.Path, name)} holds "
                             f"{v.dtype if isinstance(v, torch.Tensor) else type(v).__name__}, expected a float32 tensor")
        v = v.detach().reshape(-1)
        if want is not None and v.numel() != want:
            raise ValueError(f"ResidentLSTMDataset.fill: {os.path.join(self.Path, name)} holds {v.numel()} values, "
                             f"{self.listFiles[0]} holds {want}")
        return v

    def fill(self, device, budget_gb=None):
        """Reads every listed file once (on the host, at most FILL_THREADS at a time) into one pinned (F, W) buffer and uploads
        it in one copy; the plan follows.  ``budget_gb`` GB (None: 0.8 x the free device memory) must cover F W 4 + 9 n_steps
        bytes, else RuntimeError before anything is allocated.  A file that is not float32, or not of the first file's length,
        raises ValueError naming it; the pool is None after either."""
        from concurrent.futures import ThreadPoolExecutor
        self._refuse_fill_of_handover()
        self.release()
        device = torch.device(device)
        F = len(self.listFiles)
        if F == 0:
            raise RuntimeError(f"ResidentLSTMDataset.fill: no files in {self.Path}")
        first = self._read(self.listFiles[0])
        W = first.numel()
        need = F * W * 4 + 9 * self.n_steps
        allowed = resident_budget(device, budget_gb)
        self.needed_bytes = need
        if need > allowed:
            raise RuntimeError(f"ResidentLSTMDataset.fill: {self.Path} ({F} vectors of {W}) needs {need} bytes, {allowed} bytes "
                               f"are allowed: raise --gpu_resident_gb or run without --lstm_resident")
        with ThreadPoolExecutor(max_workers=FILL_THREADS) as ex:
            # (map re-raises a reader's exception here: a bad file is refused before the pinned buffer exists)
            vectors = [first] + list(ex.map(lambda name: self._read(name, W), self.listFiles[1:]))
        host = torch.empty((F, W), dtype=torch.float32).pin_memory()
        torch.stack(vectors, out=host)
        del vectors
        pool = host.to(device)                          # one copy; synchronous, so the pinned buffer can go
        plan = tuple(torch.from_numpy(a).to(device) for a in self.plan_host)
        self.pool, self.plan = pool, plan
        return self

    def release(self):
        """Drops the pool and the plan: the dataset is the file set again (a from_st set has none: its samples are gone)."""
        self.pool = self.plan = None
        self._complete = False
