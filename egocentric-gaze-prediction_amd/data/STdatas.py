"""Mirror of the reference's ``data/STdatas.py``: RGB frame + 10-pair optical-flow stack + ground-truth gaze map
+ fixation flag per sample (data/STdatas.py:9-73).  Host-side disk I/O, out of the kernel scope; what the hot path
relies on is the tensor contract: 'image' (3,H,W) = (u8/255 - mean)/std on BGR-ordered channels, 'flow' (20,H,W) =
(u8/255 - 0.5)/0.5 ordered x_t, y_t, x_{t-1}, y_{t-1}, ..., 'gt' (1,H,W) = u8/255, 'fixsac' (1,), 'imname'."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from ._io import imread

_MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
_STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def build_temporal_list(imgPath, gtPath, listFolders, listGtFiles):
    """Flow window looks backwards: frames n, n-1, ..., n-9 (data/STdatas.py:18-20); file-name parsing is
    positional like the reference (gt[:-17] = folder, gt[-9:-4] = frame number)."""
    imgx, imgy = [], []
    for gt in listGtFiles:
        folder, number = gt[:-17], int(gt[-9:-4])
        assert folder in listFolders
        imgx.append([os.path.join(imgPath, folder, 'flow_x_%05d.jpg' % (number - m)) for m in range(10)])
        imgy.append([os.path.join(imgPath, folder, 'flow_y_%05d.jpg' % (number - m)) for m in range(10)])
    return imgx, imgy


IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # applied to BGR-ordered channels (:51-55)
FLOW_MEAN, FLOW_STD = (0.5,) * 20, (0.5,) * 20                             # (:59-68)


def stage_batch(sample, device):
    """('image', 'flow', 'gt') of a collated sample as normalised fp32 tensors on ``device``.  A dataset built with
    ``raw_u8=True`` hands over bytes: they cross PCIe at a quarter of the fp32 size and are normalised by
    ``egz_u8_normalize`` with the reference's own three fp32 operations (bit-exact with the host expression below)."""
    if 'resident' in sample:            # data.resident: the planes are on the device already, one gather launch builds the batch
        return sample['resident'].gather(sample, device, fields=('image', 'flow', 'gt'))
    if 'jpeg_blob' in sample:           # decode='gpu': one H2D copy, one decode launch, then the raw_u8 path below
        from .. import hipops as H
        image, flow, gt = decode_to_u8(sample, device)
        return (H.u8_normalize(image, IMAGE_MEAN, IMAGE_STD), H.u8_normalize(flow, FLOW_MEAN, FLOW_STD),
                H.u8_normalize(gt, (0.0,), (1.0,)))
    if sample['image'].dtype == torch.uint8:
        from .. import hipops as H
        put = lambda t: t.contiguous().to(device, non_blocking=True)
        return (H.u8_normalize(put(sample['image']), IMAGE_MEAN, IMAGE_STD),
                H.u8_normalize(put(sample['flow']), FLOW_MEAN, FLOW_STD),
                H.u8_normalize(put(sample['gt']), (0.0,), (1.0,)))
    return (sample['image'].float().to(device, non_blocking=True), sample['flow'].float().to(device, non_blocking=True),
            sample['gt'].float().to(device, non_blocking=True))


def staged_batches(loader, device, stage=None):
    """Iterates ``loader`` one batch ahead: yields ``(sample, (image, flow, gt))`` with the NEXT batch's host-to-device copy
    and normalisation (stage_batch) already issued on a copy stream, so that batch k + 1 crosses PCIe while step k computes
    (the reference copies inside the step, SP.py:126-131).  Ordering is by stream events only; the yielded tensors are
    handed to the consumer's stream (record_stream) so the caching allocator cannot recycle them early.  Falls back to
    in-step staging when HIP streams are switched off (EGAZE_STREAMS=0) or the device is not a GPU.  ``stage(sample,
    device) -> tuple of device tensors`` defaults to stage_batch (the SP / AT sample layout); LF passes its own."""
    from .. import streams
    stage = stage or stage_batch
    device = torch.device(device)
    if device.type != 'cuda' or not streams.ENABLED:
        for sample in loader:
            staged = stage(sample, device)
            check_decode_status(sample)
            yield sample, staged
        return
    copy = streams.side_stream("h2d")

    def issue(sample):
        with torch.cuda.stream(copy):
            staged = stage(sample, device)
            if stage is stage_batch:
                # the flow stack's NHWC-32 form and its abs-max, behind the copy on the same stream (hipops.prepare_network_input):
                # two weight-independent HBM passes less at the head of the consumer's forward pass
                from .. import hipops
                hipops.prepare_network_input(staged[1])
        ev = torch.cuda.Event()
        ev.record(copy)
        return sample, staged, ev

    it = iter(loader)
    try:
        nxt = issue(next(it))
    except StopIteration:
        return
    while nxt is not None:
        sample, staged, ev = nxt
        try:
            nxt = issue(next(it))          # issued BEFORE the consumer's kernels of this batch: overlaps with them
        except StopIteration:
            nxt = None
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for t in staged:
            t.record_stream(cur)
        check_decode_status(sample)        # decode='gpu': status words read at hand-over (issued a step ago), not at issue
        yield sample, staged


def augmenting(dataset, spec, epoch):
    """The context a training loop iterates in: ``dataset.augmenting(spec, epoch)`` when ``spec`` (a hipops.AugSpec) is set and
    the dataset is a resident one, else a no-op -- the host path has no augmentation (the CLIs refuse the flag without
    --gpu_resident)."""
    import contextlib
    if spec is not None and hasattr(dataset, 'augmenting'):
        return dataset.augmenting(spec, epoch)
    return contextlib.nullcontext()


# ----------------------------------------------------------------------------- decode='gpu'
# A sample holds its 22 files as bytes; the worker's collate (collate_gpu) joins a batch's streams into one pinned buffer,
# stage_batch copies it in one H2D transfer and hipops.jpeg_decode decodes every stream into its plane of one uint8 batch
# buffer.  Files the decoder does not take (sniff() is None: progressive, arithmetic-coded, 12-bit, CMYK / Adobe-RGB JPEGs,
# PNG ground truth, ...) are decoded in the worker by _io.imread, as with decode='host', and ship as uint8 planes.
PLANES = 24                                                   # image 3 + flow 20 + gt 1
_CHANNELS = (3,) + (1,) * 21


def sniff(data):
    """(height, width) if the GPU decoder takes this file (baseline / 8-bit extended Huffman JPEG, 1 or 3 components, luma
    1x1 / 2x1 / 2x2 with 1x1 chroma, YCbCr, every component in the first scan), else None.  Reads only the header."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    pos, size, jfif, adobe_rgb, ids, nf = 2, None, False, False, (), 0
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            return None
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos + 3 > n:
            return None
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        L = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + L]
        if L < 2 or pos + L > n:
            return None
        pos += L
        if m in (0xC0, 0xC1):
            if len(seg) < 6 or seg[0] != 8 or seg[5] not in (1, 3) or len(seg) != 6 + 3 * seg[5]:
                return None
            h, w, nf = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if h == 0 or w == 0:
                return None
            samp = [seg[7 + 3 * c] for c in range(nf)]
            ids = tuple(seg[6 + 3 * c] for c in range(nf))
            if nf == 3 and (samp[0] not in (0x11, 0x21, 0x22) or samp[1] != 0x11 or samp[2] != 0x11):
                return None
            size = (h, w)
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8) or m == 0xDC:
            return None                                           # progressive, lossless, arithmetic, DNL
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe_rgb = seg[11] == 0
        elif m == 0xDA:
            if size is None or not seg or seg[0] != nf or len(seg) != 4 + 2 * nf or bytes(seg[-3:]) != b"\x00\x3f\x00":
                return None
            if nf == 3 and not jfif and (adobe_rgb or ids == (82, 71, 66)):
                return None
            return size
        elif m in (0xD8, 0xD9):
            return None
    return None


def collate_gpu(batch):
    """DataLoader collate of decode='gpu' samples, run in the worker: the batch's streams in one uint8 buffer behind an offsets
    / planes / channels table, the host-decoded files as uint8 planes.  Output plane p of the batch: image (b, c) at 3 b + c,
    flow (b, j) at 3 B + 20 b + j, gt b at 23 B + b -- three contiguous (B, C, H, W) tensors (decode_to_u8)."""
    B = len(batch)
    hw = None
    streams, offs, planes, chans, files, host, host_idx = [], [0], [], [], [], [], []
    for b, s in enumerate(batch):
        for k, (item, path) in enumerate(zip(s['jpeg'], s['files'])):
            if item is None:                # a field the consumer does not use
                continue
            plane = 3 * b if k == 0 else (3 * B + 20 * b + k - 1 if k <= 20 else 23 * B + b)
            if isinstance(item, tuple):
                data, size = item
                streams.append(data)
                offs.append(offs[-1] + len(data))
                planes.append(plane)
                chans.append(_CHANNELS[k])
                files.append(path)
            else:
                size = item.shape[1:]
                host.append(item)
                host_idx.extend(range(plane, plane + item.shape[0]))
            if hw is None:
                hw = tuple(size)
            elif tuple(size) != hw:
                raise RuntimeError(f"{path}: {tuple(size)} pixels, the batch's first file has {hw}")
    n = len(streams)
    head = 8 * (2 * n + 1) + 4 * n
    head += -head % 8
    blob = torch.empty(head + offs[-1], dtype=torch.uint8)
    if n:
        blob[:8 * (2 * n + 1)].view(torch.int64).copy_(torch.tensor(offs + planes, dtype=torch.int64))
        blob[8 * (2 * n + 1):8 * (2 * n + 1) + 4 * n].view(torch.int32).copy_(torch.tensor(chans, dtype=torch.int32))
        blob[head:].copy_(torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8))
    return {'jpeg_blob': blob, 'jpeg_n': n, 'jpeg_n3': sum(c == 3 for c in chans), 'jpeg_files': files,
            'jpeg_hw': hw, 'batch': B,
            'host_planes': torch.from_numpy(np.concatenate(host)) if host else torch.empty((0,) + hw, dtype=torch.uint8),
            'host_index': torch.tensor(host_idx, dtype=torch.int64),
            'fixsac': torch.stack([s['fixsac'] for s in batch]), 'imname': [s['imname'] for s in batch]}


def decode_to_u8(sample, device):
    """A collate_gpu batch -> ('image' (B,3,H,W), 'flow' (B,20,H,W), 'gt' (B,1,H,W)) uint8 on ``device``, the layout a
    ``raw_u8`` dataset's batch has after its H2D copy.  Issued on the current stream; the status words are read later by
    check_decode_status (a pinned copy behind the decode)."""
    from .. import hipops as H
    B, (h, w), n = sample['batch'], sample['jpeg_hw'], sample['jpeg_n']
    HW = h * w
    flat = torch.empty(B * PLANES * HW, dtype=torch.uint8, device=device)
    if n:
        blob = sample['jpeg_blob'].to(device, non_blocking=True)
        t = 8 * (2 * n + 1)
        head = t + 4 * n
        head += -head % 8
        _, status = H.jpeg_decode(blob[head:], blob[:8 * (n + 1)].view(torch.int64), (h, w), blob[t:t + 4 * n].view(torch.int32),
                                  out=flat, planes=blob[8 * (n + 1):t].view(torch.int64), n3=sample['jpeg_n3'])
        host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
    if sample['host_index'].numel():
        src = sample['host_planes'].to(device, non_blocking=True).view(-1, HW)
        flat.view(-1, HW).index_copy_(0, sample['host_index'].to(device, non_blocking=True), src)
    if n:
        ev = torch.cuda.Event()
        ev.record()                        # behind the whole batch: check_decode_status's wait covers the staged planes too
        sample['_jpeg_status'] = (host, ev)
    return (flat[:3 * B * HW].view(B, 3, h, w), flat[3 * B * HW:23 * B * HW].view(B, 20, h, w),
            flat[23 * B * HW:].view(B, 1, h, w))


def check_decode_status(sample):
    """Reads the status words of a decode_to_u8 batch (waits for that batch's decode only): corrupt data warns, as cv2 does, and
    keeps the partially decoded image; an unsupported file or a size mismatch raises.  No-op for other samples."""
    if not isinstance(sample, dict):
        return
    resident = sample.pop('_resident_status', None)
    if resident is not None:               # data.resident: the gather skipped a sample whose index was out of range
        from ..hipops import check_resident_status
        check_resident_status(resident)
    pending = sample.pop('_jpeg_status', None)
    if pending is None:
        return
    host, ev = pending
    ev.synchronize()
    import warnings
    from ..hipops import JPEG_STATUS
    for i in torch.nonzero(host).flatten().tolist():
        st, path = int(host[i]), sample['jpeg_files'][i]
        if st == 1:
            warnings.warn(f"{path}: {JPEG_STATUS[1]} (decoded with zero padding, as libjpeg does)", RuntimeWarning)
        else:
            raise RuntimeError(f"{path}: GPU JPEG decode failed: {JPEG_STATUS.get(st, st)}")


def to_raw_u8(sample, device):
    """A decode='gpu' batch in the layout of a ``raw_u8`` batch on ``device`` (uint8 'image' / 'flow' / 'gt', the other
    fields as they are), status words checked; other batches are returned unchanged.  For consumers that index the fields."""
    if 'resident' in sample:               # data.resident: the bytes gathered from the pool, no file is read
        raw = sample['resident'].gather(sample, device, raw=True)
        check_decode_status(sample)
        image, flow, gt = raw[:, :3], raw[:, 3:23], raw[:, 23:]
        if raw.shape[0] > 1:
            image, flow, gt = image.contiguous(), flow.contiguous(), gt.contiguous()
        return {'image': image, 'flow': flow, 'gt': gt, 'fixsac': sample['fixsac'], 'imname': sample['imname']}
    if 'jpeg_blob' not in sample:
        return sample
    image, flow, gt = decode_to_u8(sample, device)
    check_decode_status(sample)
    return {'image': image, 'flow': flow, 'gt': gt, 'fixsac': sample['fixsac'], 'imname': sample['imname']}


class STDataset(Dataset):
    def __init__(self, imgPath, imgPath_s, gtPath, listFolders, listTrainFiles, listGtFiles, listfixsacTrain,
                 fixsacPath, raw_u8=False, decode='host'):
        if decode not in ('host', 'gpu'):
            raise ValueError(f"decode must be 'host' or 'gpu', got {decode!r}")
        self.decode = decode
        # the package's DataLoaders pass collate_fn=dataset.collate_fn (None: torch's default_collate)
        self.collate_fn = collate_gpu if decode == 'gpu' else None
        # decode='gpu': the fields a consumer uses; the files of the others are not read (their planes stay undefined) --
        # the single-stream pre-training scripts set ('image', 'gt') or ('flow', 'gt')
        self.gpu_fields = ('image', 'flow', 'gt')
        self.raw_u8 = raw_u8
        self.listFolders, self.listGtFiles = listFolders, listGtFiles
        self.imgPath, self.imgPath_s, self.gtPath = imgPath, imgPath_s, gtPath
        self.listTrainFiles = listTrainFiles
        self.imgx, self.imgy = build_temporal_list(imgPath, gtPath, listFolders, listGtFiles)
        chunks = []
        for f in listfixsacTrain:          # dilate the fixation labels by one frame each side (:37-41)
            a = np.loadtxt(os.path.join(fixsacPath, f))
            chunks.append((np.convolve(a, np.array([1, 1, 1]))[1:-1] > 0).astype(float))
        self.fixsac = np.concatenate(chunks) if chunks else np.zeros(0)

    def __len__(self):
        return len(self.listGtFiles)

    def _files(self, index):
        flow = [f for pair in zip(self.imgx[index], self.imgy[index]) for f in pair]
        return ([os.path.join(self.imgPath_s, self.listTrainFiles[index])] + flow +
                [os.path.join(self.gtPath, self.listGtFiles[index])])

    def __getitem__(self, index):
        if self.decode == 'gpu':            # file bytes out (collate_gpu joins them); the rest host-decoded as (C, H, W) u8
            files = self._files(index)
            items = []
            for k, path in enumerate(files):
                if ('image' if k == 0 else 'flow' if k <= 20 else 'gt') not in self.gpu_fields:
                    items.append(None)
                    continue
                with open(path, 'rb') as f:
                    data = f.read()
                size = sniff(data)
                if size is not None:
                    items.append((data, size))
                else:
                    a = imread(path, gray=_CHANNELS[k] == 1)
                    items.append(a[None] if a.ndim == 2 else a.transpose((2, 0, 1)).copy())
            return {'jpeg': items, 'files': files, 'fixsac': torch.FloatTensor([self.fixsac[index]]),
                    'imname': self.listTrainFiles[index]}
        im = torch.from_numpy(imread(os.path.join(self.imgPath_s, self.listTrainFiles[index])).transpose((2, 0, 1)).copy())
        if self.raw_u8:            # bytes out; stage_batch() normalises on the device
            planes = []
            for fx, fy in zip(self.imgx[index], self.imgy[index]):
                planes.append(torch.from_numpy(imread(fx, gray=True)))
                planes.append(torch.from_numpy(imread(fy, gray=True)))
            gt = torch.from_numpy(imread(os.path.join(self.gtPath, self.listGtFiles[index]), gray=True))
            return {'image': im, 'flow': torch.stack(planes), 'gt': gt.unsqueeze(0),
                    'fixsac': torch.FloatTensor([self.fixsac[index]]), 'imname': self.listTrainFiles[index]}
        im = (im.float().div(255) - _MEAN) / _STD
        planes = []
        for fx, fy in zip(self.imgx[index], self.imgy[index]):
            planes.append(torch.from_numpy(imread(fx, gray=True)))
            planes.append(torch.from_numpy(imread(fy, gray=True)))
        flow = (torch.stack(planes).float().div_(255) - 0.5) / 0.5
        gt = torch.from_numpy(imread(os.path.join(self.gtPath, self.listGtFiles[index]), gray=True)).float().div(255)
        return {'image': im, 'flow': flow, 'gt': gt.unsqueeze(0),
                'fixsac': torch.FloatTensor([self.fixsac[index]]), 'imname': self.listTrainFiles[index]}
