"""The AT stage's LSTM vectors resident in HBM (``--lstm_resident``): every ``fix_*.pth.tar`` vector of a ``lstmDataset`` folder
is read ONCE into an fp32 pool on the device, and each step of ``AT.trainLSTM`` / ``AT.testLSTM`` fetches its input, its target
and its state reset there (hipops.lstm_pool_fetch, captured at the head of the step's hipGraph, stepping off a cursor on the
device).  The loop then unpickles no file and copies no vector over PCIe.  DESIGN.md section 17 has the plan derivation.

Unlike data.resident / data.late_resident a sample of this dataset is NOT its number: ``__getitem__`` is lstmDataset's, so the
dataset is also the file set -- what AT iterates before ``fill()``, after ``release()`` and wherever the fused single-step path
is off."""
import os

import numpy as np
import torch

from .LSTMdatas import deferred_steps, lstmDataset

FILL_THREADS = 16                           # file reads of fill() in flight at most


def lstm_plan(listFiles):
    """The steps of one epoch over the sorted file list, from the names alone -> (in_row, tgt_row int32, reset uint8), one entry
    per step.  The schedule is LSTMdatas.deferred_steps, the one the file loop runs (AT._epoch_graphed), fed with file rows in
    place of vectors: sample i is (file i, file i + 1, lstmDataset's ``same`` flag).  Step k = 1 .. F - 2 therefore reads file
    k - 1 as its input and file k + 1 as its target, and resets the state first where file k - 1 and file k belong to
    different videos, or nothing ran before (k = 1).  Fewer than three files: no step."""
    samples = ((i, i + 1, listFiles[i + 1][:-14] == listFiles[i][:-14]) for i in range(len(listFiles) - 1))
    steps = np.array(list(deferred_steps(samples)), dtype=np.int64).reshape(-1, 3)
    return steps[:, 0].astype(np.int32), steps[:, 1].astype(np.int32), steps[:, 2].astype(np.uint8)


class ResidentLSTMDataset(lstmDataset):
    """``lstmDataset`` whose vectors can live on the device.  Usage: ``ds.fill(device)`` once; AT._epoch then runs the plan
    (``pool`` (F, W) fp32, ``plan`` = (in_row, tgt_row, reset) on the device, ``n_steps``) instead of iterating the files."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pool = self.plan = None        # device tensors after fill()
        self.plan_host = lstm_plan(self.listFiles)
        self.n_steps = len(self.plan_host[0])
        self.needed_bytes = None            # known once the first file gave the vector length

    @property
    def filled(self):
        return self.pool is not None

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
        self.release()
        device = torch.device(device)
        F = len(self.listFiles)
        if F == 0:
            raise RuntimeError(f"ResidentLSTMDataset.fill: no files in {self.Path}")
        first = self._read(self.listFiles[0])
        W = first.numel()
        need = F * W * 4 + 9 * self.n_steps
        allowed = int(budget_gb * 1e9) if budget_gb is not None else int(0.8 * torch.cuda.mem_get_info(device)[0])
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
        """Drops the pool and the plan: the dataset is the file set again."""
        self.pool = self.plan = None
