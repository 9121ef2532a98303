"""The decoded dataset resident in HBM (``--gpu_resident``): every distinct file of an ``STDataset`` is decoded ONCE into a
uint8 plane pool on the device, and a batch is one gather launch over that pool (hipops.resident_gather: gather, the three
normalisations, the flow stack's NHWC-32 form and its abs-max).  Per frame the distinct data is one colour image, one flow_x,
one flow_y and one ground-truth map -- 6 planes -- while a sample reads 24 planes from 22 files and consecutive samples share 18
of their 20 flow files; the loop then does no decode, no PCIe copy of pixels and no re-read of the flow window.  DESIGN.md
section 15 has the memory arithmetic.

A sample of this dataset is its number; the collated batch carries the numbers and the dataset, and the two staging choke
points (data.STdatas.stage_batch / to_raw_u8, streamtrain.stage_stream) turn it into tensors.  The DataLoader, its samplers and
their RNG draws are those of the host dataset, so a seeded run visits the same samples in the same batches."""
import contextlib
import os
import time
import warnings
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._io import imread
from .STdatas import STDataset, sniff

COLS = 22                                   # table columns: image, 20 flow planes, ground truth


class FlowFrom(NamedTuple):
    """Where the flow planes of a resident dataset come from when not from files: data.extract_flow.flows_into computes them
    from the frames under ``framePath`` (one folder per video, img_%05d.jpg) with these arguments of its own."""
    framePath: str
    bound: float = 20.0
    quality: int = 95
    chunk: int = 32
    params: Optional[dict] = None


# ----------------------------------------------------------------------------- the one-time fill, shared by the resident datasets
# (this class and data.late_resident.ResidentLateDataset): a planned dataset has ``files`` [(path, first plane, channels)],
# ``planes``, ``hw``, ``plane_table``, ``needed_bytes`` and ``decode``
def _read(path):
    try:
        with open(path, 'rb') as f:
            return f.read()
    except OSError as e:
        raise RuntimeError(f"{path}: unreadable: {e}") from e


def _host_decode(path, channels):
    try:
        a = imread(path, gray=channels == 1)
    except Exception as e:
        raise RuntimeError(f"{path}: unreadable: {e}") from e
    return a[None] if a.ndim == 2 else a.transpose((2, 0, 1))


def _size_of(path, channels):
    size = sniff(_read(path))
    return tuple(size) if size is not None else tuple(_host_decode(path, channels).shape[1:])


def fill_pool(files, hw, decode, device, chunk, planes=None):
    """Decodes ``files`` [(path, first plane, channels)], ``chunk`` files at a time, straight into their planes of a new uint8
    (planes, h, w) pool on ``device`` (``planes`` None: up to the last file's; planes no file names stay undefined -- the
    flow planes of a dataset planned with ``flow_from``, which flows_into writes): decode='gpu' sends the files ``sniff`` takes through hipops.jpeg_decode, everything else
    goes through _io.imread and a pinned staging buffer.  Corrupt data warns, naming the file; an unsupported, unreadable or
    wrongly sized file raises, naming it.  -> the pool; the work may still be in flight on the current stream."""
    from .. import hipops as H
    h, w = hw
    pool = torch.empty((files[-1][1] + files[-1][2] if planes is None else planes, h, w), dtype=torch.uint8, device=device)
    if not files:
        return pool
    stage = torch.empty((min(chunk, len(files)) * max(f[2] for f in files), h, w), dtype=torch.uint8, pin_memory=True)
    pending = []                            # (host status words, event, paths) of the decode launches in flight
    for c0 in range(0, len(files), chunk):
        streams, offs, planes, chans, paths, host_idx, n_host = [], [0], [], [], [], [], 0
        if pending:                         # the staging buffer is reused: the chunk before has left it
            pending[-1][1].synchronize()
        for path, plane, channels in files[c0:c0 + chunk]:
            data = _read(path) if decode == 'gpu' else None
            size = sniff(data) if data is not None else None
            if size is not None:
                streams.append(data)
                offs.append(offs[-1] + len(data))
                planes.append(plane)
                chans.append(channels)
                paths.append(path)
            else:
                a = _host_decode(path, channels)
                size = a.shape[1:]
                if tuple(size) == (h, w):
                    stage[n_host:n_host + channels].copy_(torch.from_numpy(np.array(a)))
                    host_idx.extend(range(plane, plane + channels))
                    n_host += channels
            if tuple(size) != (h, w):
                raise RuntimeError(f"{path}: {tuple(size)} pixels, the dataset's first file has {(h, w)}")
        host = None
        if streams:
            blob = torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8).to(device)
            _, status = H.jpeg_decode(blob, offs, (h, w), chans, out=pool, planes=planes, n3=sum(c == 3 for c in chans))
            host = torch.empty(len(streams), dtype=torch.int32, pin_memory=True)
            host.copy_(status, non_blocking=True)
        if n_host:
            pool.index_copy_(0, torch.tensor(host_idx, dtype=torch.int64).to(device, non_blocking=True),
                             stage[:n_host].to(device, non_blocking=True))
        ev = torch.cuda.Event()
        ev.record()
        pending.append((host, ev, paths))
    for host, ev, paths in pending:         # check_decode_status's rules
        ev.synchronize()
        if host is None:
            continue
        for i in torch.nonzero(host).flatten().tolist():
            st = int(host[i])
            if st == 1:
                warnings.warn(f"{paths[i]}: {H.JPEG_STATUS[1]} (decoded with zero padding, as libjpeg does)", RuntimeWarning)
            else:
                raise RuntimeError(f"{paths[i]}: GPU JPEG decode failed: {H.JPEG_STATUS.get(st, st)}")
    return pool


# ----------------------------------------------------------------------------- the memory budget of everything resident
def resident_budget(device, gb=None, spent=0):
    """The bytes that resident pools may take on ``device``: ``gb`` GB (--gpu_resident_gb) less the ``spent`` bytes of the
    pools already there, or, without a figure, 0.8 x what is free on the device now."""
    if gb is not None:
        return int(gb * 1e9) - spent
    return int(0.8 * torch.cuda.mem_get_info(torch.device(device))[0])


def under_budget(sets, budget, refusal, action):
    """Several sets under ONE ``budget`` (bytes): their ``needed_bytes`` are summed and a total above the budget raises
    ``refusal(needed, budget)`` (-> the message) before anything is allocated; then ``action(ds, what is left)`` -- a fill
    or an allocate -- runs per set, each taking its bytes off.  A set that needs exactly what is left fits."""
    needed = sum(ds.needed_bytes for ds in sets)
    if needed > budget:
        raise RuntimeError(refusal(needed, budget))
    for ds in sets:
        action(ds, budget)
        budget -= ds.needed_bytes


class HandoverPool:
    """The life cycle of a resident dataset whose pool is written on the device by an extraction, not read from files (the
    ``from_st`` sets): ``from_st`` sets ``_handover``; ``allocate`` creates the empty pool; the extraction writes it and calls
    ``mark_filled``; ``filled`` is False in between, and the consumers refuse until then.  A set listed from files
    (``_handover`` False) is refused by ``allocate``, a from_st set by ``fill``.  The class beside it supplies the nouns
    (``_READS``: what its fill does with files; ``_WRITER``: the extraction call), ``_allocation_needs()`` (-> the "... need
    N bytes" half of the over-budget message), ``_OVER_BUDGET`` (the advice that ends that message),
    ``_allocate_empty(device)`` (the zero-filled pool and what lies beside it) and, where it applies, ``_refuse_allocation(who)``
    (raises for a set with nothing to allocate) and ``_RELEASE_FIRST`` with a ``release()`` (a new pool must not live
    beside the old one)."""
    _handover = _complete = False
    _RELEASE_FIRST = False

    def _refuse_allocation(self, who):
        pass

    def allocate(self, device, budget_bytes=None):
        """The zero-filled pool of a from_st set on ``device``: a set that does not fit ``budget_bytes`` (None:
        resident_budget's 0.8 x the free device memory) raises before anything is allocated."""
        who = f"{type(self).__name__}.allocate"
        if not self._handover:
            raise RuntimeError(f"{who}: only a from_st set is allocated empty; fill() {self._READS}s the files")
        if self._RELEASE_FIRST:
            self.release()
        device = torch.device(device)
        self._refuse_allocation(who)
        if budget_bytes is None:
            budget_bytes = resident_budget(device)
        if self.needed_bytes > budget_bytes:
            raise RuntimeError(f"{who}: {self._allocation_needs()}, {budget_bytes} bytes are allowed: {self._OVER_BUDGET}")
        self._allocate_empty(device)
        self._complete = False
        return self

    def mark_filled(self):
        """The extraction's last act: every row has been written, the set may be read."""
        if self.pool is None:
            raise RuntimeError(f"{type(self).__name__}.mark_filled: allocate(device) has not run")
        self._complete = True
        return self

    @property
    def filled(self):
        """The pool is on the device and all of it has been written (by fill, or by the extraction of a from_st set)."""
        return self.pool is not None and (not self._handover or self._complete)

    def _refuse_fill_of_handover(self):
        if self._handover:
            raise RuntimeError(f"{type(self).__name__}.fill: a from_st set has no files to {self._READS} (allocate(), then "
                               f"{self._WRITER})")


def check_st_source(st_set, dev, who, fields, loader, stage, why):
    """The ST half of an ``into=`` extraction's preconditions: ``st_set`` is a ResidentSTDataset, filled, on ``dev``, with
    ``fields`` in its plan.  ``loader`` / ``stage`` / ``why`` are the caller's words for where the set came from, what runs on
    ``dev`` and what is taken from the pool."""
    if not isinstance(st_set, ResidentSTDataset):
        raise ValueError(f"{who}: {loader}.dataset must be a ResidentSTDataset (--gpu_resident), got {type(st_set).__name__}: "
                         f"{why}")
    if st_set.pool is None:
        raise ValueError(f"{who}: the ResidentSTDataset has not been filled (fill(device))")
    if st_set.pool.device != dev:
        raise ValueError(f"{who}: the ST pool is on {st_set.pool.device}, the {stage} runs on {dev}")
    missing = [f for f in fields if f not in (st_set._plan or ())]
    if missing:
        raise ValueError(f"{who}: field(s) {missing} were not in gpu_fields when the ST pool was filled")


def fill_planned(ds, device, budget_bytes, chunk, who, flag):
    """``fill`` of a planned resident dataset ``ds``: refuses before allocating when ``needed_bytes`` exceeds ``budget_bytes``
    (None: 0.8 x the free device memory; ``who`` / ``flag`` name the caller and its CLI switch in the message), fills the pool
    (fill_pool), puts the table beside it and prints the number of files, the bytes and the seconds once."""
    device = torch.device(device)
    if budget_bytes is None:
        budget_bytes = resident_budget(device)
    if ds.needed_bytes > budget_bytes:
        raise RuntimeError(f"{who}: the decoded dataset needs {ds.needed_bytes} bytes "
                           f"({ds.planes} planes of {ds.hw[0]} x {ds.hw[1]}), {budget_bytes} bytes are allowed: "
                           f"run without {flag} (there is no partial cache)")
    t0 = time.perf_counter()
    skip = {path for path, _ in getattr(ds, 'flow_keys', ())}     # planned with flow_from: keys, not files
    files = [f for f in ds.files if f[0] not in skip] if skip else ds.files
    pool = fill_pool(files, ds.hw, ds.decode, device, chunk, planes=ds.planes)
    ds.table = ds.plane_table.to(device)
    torch.cuda.synchronize(device)          # the gathers run on other streams (staged_batches' copy stream)
    ds.pool = pool
    ds.fill_seconds = time.perf_counter() - t0
    print(f"resident dataset: {len(files)} files decoded ({ds.decode}) into {ds.planes} planes, "
          f"{ds.needed_bytes} bytes on {device}, {ds.fill_seconds:.2f} s")
    return ds


class ResidentSTDataset(STDataset):
    """``STDataset`` whose planes live on the device.  ``decode`` selects how ``fill`` decodes ('gpu': hipops.jpeg_decode
    for the files ``sniff`` takes, the host for the rest); ``gpu_fields`` is honoured as in ``STDataset``: files of a field
    not in it are neither read nor given planes.  Usage: ``ds.fill(device)`` once, then any DataLoader with
    ``collate_fn=ds.collate_fn`` and ``num_workers=ds.loader_workers``."""
    loader_workers = 0                      # the pool must not be pickled into a worker

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.collate_fn = self._collate
        self.pool = self.table = None       # device tensors after fill()
        self._plan = None
        self.flow_from = None               # a FlowFrom: the flow paths are keys, flows_into fills their planes
        self.flow_keys = []                 # [(flow path, plane)] under flow_from
        self.flow_counts = None             # flows_into's counts after such a fill
        self._augment = None                # (AugSpec, epoch) inside augmenting()

    # ------------------------------------------------------------------ plan (host only)
    def plan(self):
        """Lists the distinct files of the fields in use, gives each its planes in the pool and builds the (N, 22) table of
        plane numbers (-1 in the columns of a field not in use).  Reads one file header for the plane size; touches no device.
        Sets ``files`` [(path, first plane, channels)], ``planes``, ``hw``, ``plane_table`` (host) and ``needed_bytes``.
        With ``flow_from`` the flow paths are listed and given planes all the same -- table and bytes are those of the plan
        over files -- but as keys (``flow_keys``): no flow file is opened, and a sample whose stack needs a flow the frames
        cannot give is refused here, before anything is allocated."""
        fields = tuple(self.gpu_fields)
        N = len(self)
        table = np.full((N, COLS), -1, dtype=np.int64)
        files, where = [], {}

        def plane_of(path, channels):
            p = where.get(path)
            if p is None:
                p = where[path] = (files[-1][1] + files[-1][2]) if files else 0
                files.append((path, p, channels))
            return p
        for i in range(N):
            paths = self._files(i)
            if 'image' in fields:
                table[i, 0] = plane_of(paths[0], 3)
        for i in range(N):
            if 'flow' in fields:
                for j, path in enumerate(self._files(i)[1:21]):
                    table[i, 1 + j] = plane_of(path, 1)
        for i in range(N):
            if 'gt' in fields:
                table[i, 21] = plane_of(self._files(i)[21], 1)
        if not files:
            raise RuntimeError("ResidentSTDataset.plan: no files (an empty dataset or no field in gpu_fields)")
        self.flow_keys = []
        if self.flow_from is not None and 'flow' in fields:
            self._check_flows(table)
            flow_planes = set(table[:, 1:21].flatten().tolist())
            self.flow_keys = [(path, p) for path, p, _ in files if p in flow_planes]
        self.files = files
        self.planes = files[-1][1] + files[-1][2]
        keys = {path for path, _ in self.flow_keys}
        sized = next((f for f in files if f[0] not in keys), None)
        self.hw = self._size_of(sized[0], sized[2]) if sized is not None else self._frame_size()
        self.plane_table = torch.from_numpy(table)
        self.needed_bytes = self.planes * self.hw[0] * self.hw[1] + table.nbytes
        self._plan = fields
        return self

    def _check_flows(self, table):
        """Refuses the first sample one of whose flows the frames under ``flow_from.framePath`` cannot give: flow n runs from
        frame n to frame n + 1 (extract_flow's numbering), so both must be there."""
        from .extract_flow import flow_key, list_frames, missing_frame
        numbers = {}
        for i in range(len(self)):
            for path in self._files(i)[1:21]:
                folder, _, n = flow_key(path)
                if folder not in numbers:
                    src = os.path.join(self.flow_from.framePath, folder)
                    numbers[folder] = {k for k, _ in list_frames(src)} if os.path.isdir(src) else set()
                miss = missing_frame(numbers[folder], n)
                if miss is not None:
                    raise RuntimeError(f"ResidentSTDataset.plan: sample {i} ({self.listGtFiles[i]}) needs "
                                       f"{os.path.basename(path)} of {folder}, which the frames cannot give: "
                                       f"{os.path.join(self.flow_from.framePath, folder, 'img_%05d.jpg' % miss)} is missing")

    def _frame_size(self):
        """Plane size of a plan that holds flow keys only: the first frame's."""
        from .extract_flow import flow_key, list_frames
        src = os.path.join(self.flow_from.framePath, flow_key(self.flow_keys[0][0])[0])
        return self._size_of(os.path.join(src, list_frames(src)[0][1]), 3)

    _read, _host_decode = staticmethod(_read), staticmethod(_host_decode)

    def _size_of(self, path, channels):
        return _size_of(path, channels)

    # ------------------------------------------------------------------ fill (decode once)
    def fill(self, device, budget_bytes=None, chunk=704, flow_from=None, run_flows=True):
        """Decodes every distinct file once, ``chunk`` files at a time, straight into its planes of the pool on ``device``.
        ``budget_bytes`` None: 0.8 x the free device memory.  A pool that does not fit raises before anything is allocated
        (there is no partial cache).  Corrupt data warns, naming the file; an unsupported, unreadable or wrongly sized file
        raises, naming it.  Prints the number of files, the bytes and the seconds once.  ``flow_from`` (a FlowFrom): the flow
        planes are not decoded from files but computed from the frames by data.extract_flow.flows_into, here unless
        ``run_flows`` is False (fill_all runs it once for all its datasets); its counts are left in ``flow_counts``."""
        if self._plan != tuple(self.gpu_fields) or flow_from != self.flow_from:
            self.flow_from = flow_from
            self.plan()
        fill_planned(self, device, budget_bytes, chunk, "ResidentSTDataset.fill", "--gpu_resident")
        if flow_from is not None and run_flows:
            run_flows_into([self], device, flow_from)
        return self

    # ------------------------------------------------------------------ samples
    def __getitem__(self, index):
        return {'index': index, 'fixsac': torch.FloatTensor([self.fixsac[index]]), 'imname': self.listTrainFiles[index]}

    def _collate(self, batch):
        out = {'resident': self, 'index': torch.LongTensor([s['index'] for s in batch]),
               'fixsac': torch.stack([s['fixsac'] for s in batch]), 'imname': [s['imname'] for s in batch]}
        if self._augment is not None:       # inside augmenting(): the batch is gathered through resident_gather_aug
            out['augment'] = self._augment
        return out

    @contextlib.contextmanager
    def augmenting(self, spec, epoch):
        """While inside, every batch this dataset collates is stamped with ``(spec, epoch)`` (a hipops.AugSpec and the driver's
        epoch number) and ``gather`` augments it on the device (hipops.resident_gather_aug); outside nothing is stamped.  The
        stamp is put on at collation, and ``loader_workers`` is 0, so collation happens in the consuming process: the batch
        that data.STdatas.staged_batches collates and stages one step ahead gets the stamp of the block its loop runs in.  A
        training loop wraps its iteration in this and leaves it in a ``finally``; validation and the extraction passes run
        outside and never see an augmented batch."""
        from ..hipops import AugSpec
        if not isinstance(spec, AugSpec):
            raise ValueError(f"ResidentSTDataset.augmenting: spec must be a hipops.AugSpec, got {type(spec).__name__}")
        before, self._augment = self._augment, (spec, int(epoch))
        try:
            yield self
        finally:
            self._augment = before

    def gather(self, sample, device, fields=None, raw=False, prepare=True):
        """The collated ``sample`` as device tensors: ``index`` crosses PCIe (non-blocking), one gather launch follows on the
        current stream; its status word is left on ``sample`` for check_decode_status.  A sample stamped by ``augmenting`` goes
        through hipops.resident_gather_aug (and refuses ``raw``).  -> hipops.resident_gather's result."""
        from .. import hipops as H
        stamp = sample.get('augment')
        if stamp is not None and raw:       # the AT extraction reads raw bytes: it must never be augmented by accident
            raise RuntimeError("ResidentSTDataset: a batch collated inside augmenting() was asked for as raw bytes "
                               "(raw=True is the extraction path, which is never augmented)")
        if self.pool is None:
            raise RuntimeError("ResidentSTDataset: fill(device) has not run (the pool is not on the device)")
        if torch.device(device) != self.pool.device:
            raise RuntimeError(f"ResidentSTDataset: the pool is on {self.pool.device}, the batch is asked for on {device}")
        fields = tuple(self.gpu_fields) if fields is None else tuple(fields)
        missing = [f for f in fields if f not in self._plan]
        if missing:
            raise RuntimeError(f"ResidentSTDataset: field(s) {missing} were not in gpu_fields when the pool was filled")
        idx = sample['index'].to(self.pool.device, non_blocking=True)
        if stamp is not None:
            return H.resident_gather_aug(self.pool, self.table, idx, stamp[0], stamp[1], fields=fields, prepare=prepare,
                                         status_to=sample)
        return H.resident_gather(self.pool, self.table, idx, fields=fields, raw=raw, prepare=prepare, status_to=sample)


def run_flows_into(datasets, device, flow_from):
    """flows_into over filled ``datasets`` with the record's arguments; leaves the counts on each and prints them once."""
    from .extract_flow import flows_into
    t0 = time.perf_counter()
    counts = flows_into(datasets, flow_from.framePath, device, bound=flow_from.bound, quality=flow_from.quality,
                        chunk=flow_from.chunk, params=flow_from.params)
    for ds in datasets:
        ds.flow_counts = counts
    print(f"flow hand-over: {counts['pairs']} frame pairs computed, {counts['planes']} planes written, "
          f"{counts['files']} files, {time.perf_counter() - t0:.2f} s")
    return counts


def fill_all(datasets, device, budget_gb=None, flag="--gpu_resident", flow_from=None):
    """Fills several resident datasets (the training and the validation set of a script; ResidentSTDatasets,
    ResidentLateDatasets or a mix) under ONE budget: ``budget_gb`` GB, or 0.8 x the free memory of ``device``.  All are planned
    first, so a set that does not fit raises before any pool is allocated.  ``flag``: the CLI switch the refusal names.
    ``flow_from`` (a FlowFrom, ResidentSTDatasets only): the flow planes of all of them are computed from the frames in one
    flows_into pass after the fills."""
    datasets = [ds for ds in datasets if len(ds)]
    for ds in datasets:
        if flow_from is not None:
            ds.flow_from = flow_from
        ds.plan()
    flows = {} if flow_from is None else dict(flow_from=flow_from, run_flows=False)
    under_budget(datasets, resident_budget(device, budget_gb),
                 lambda needed, budget: f"{flag}: the decoded datasets need {needed} bytes, {budget} bytes are allowed: "
                                        f"run without {flag} (there is no partial cache)",
                 lambda ds, left: ds.fill(device, budget_bytes=left, **flows))
    if flow_from is not None:
        run_flows_into(datasets, device, flow_from)
