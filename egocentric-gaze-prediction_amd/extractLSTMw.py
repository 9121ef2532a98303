"""Mirror of the reference's ``extractLSTMw.py`` (offline data preparation between SP and AT, extractLSTMw.py:21-138):
run ``features_s`` alone over a dataset and store, for the second frame of every fixation, the spatial mean of a window
of the conv5_3 map around the ground-truth gaze cell as ``fix_<name>.pth.tar``.  The encoder forward is the same fused
HIP path the SP model uses; the window mean is one small kernel (egz_window_mean).

Reproduced, not "fixed" (checked against the reference by tests/golden/extract_lstm.npz):
  * the gaze cell is the arg-max of the ``AvgPool2d(16)``-downsampled ground truth (extractLSTMw.py:66,85-88), not of the
    full-resolution map;
  * ``crop_feature_var`` clips with FLOAT bounds and slices with ``int()`` (extractLSTMw.py:46-58): for crop_size 3 the
    window is rows/cols [int(f - 1.5), int(f + 2)) with f clipped to [1.5, H - 2] -- 4 x 4 cells in the interior and
    3 at the low border, unlike AT.crop_feature's 3 x 3;
  * the fixation state machine (extractLSTMw.py:74-111): the first frame of a fixation arms it, the second is extracted,
    the rest are skipped until a saccade frame; a fixation that ends after one frame raises RuntimeError.
"""
import math
import os

import torch
import torch.nn as nn

from .trainloop import extraction_loader
from .utils import cfg, load_merged, make_layers


def var_window(ind, size, H, W):
    """Half-open cell window (y0, y1, x0, x1) of extractLSTMw.crop_feature_var for the flat arg-max ``ind`` of an
    H x W map: float clip, then int() truncation of both slice bounds (extractLSTMw.py:52-54)."""
    up = int(math.ceil(size / 2.0))
    out = []
    for f, n in ((ind // W, H), (ind % W, H)):          # the reference clips both coordinates with H (square maps)
        f = min(max(float(f), size / 2), float(n - up))
        out += [int(f - size / 2), int(f + up)]
    return tuple(out)


def crop_feature_var(feature, maxind, size):
    """(B,C,H,W) map, (B,...) flat arg-max indices -> the windows stacked along the batch dim (all samples of a batch
    must produce the same window shape, as in the reference's torch.cat)."""
    H, W = feature.size(2), feature.size(3)
    out = []
    for b in range(feature.size(0)):
        y0, y1, x0, x1 = var_window(int(maxind[b].item()), size, H, W)
        out.append(feature[b:b + 1, :, y0:y1, x0:x1])
    return torch.cat(out, 0)


def crop_feature_align(feature, maxind, size):
    """``--align`` variant on the x16 bilinearly upsampled map (extractLSTMw.py:32-44): integer clip, size*16 window."""
    size *= 16
    H, W = feature.size(2), feature.size(3)
    out = []
    for b in range(feature.size(0)):
        ind = int(maxind[b].item())
        fy = min(max(ind // W, size // 2), H - size // 2)
        fx = min(max(ind % W, size // 2), H - size // 2)
        out.append(feature[b:b + 1, :, fy - size // 2:fy + size // 2, fx - size // 2:fx + size // 2])
    return torch.cat(out, 0)


def channel_weight(feat, gt, crop_size, align):
    """chn_weight (512,) of one sample: feat (1,512,14,14) on the device, gt (1,1,224,224) on the host."""
    if align:
        flat = gt.float().view(gt.size(0), gt.size(1), -1)
        _, maxind = torch.max(flat, 2)
        if feat.is_cuda:             # the window mean of the x16 bilinear upsampling as one kernel on the 14 x 14 map
            from .AT import crop_align_mean
            full = feat.size(3) * 16
            gp = [[int(maxind[b].item()) // full, int(maxind[b].item()) % full] for b in range(feat.size(0))]
            return crop_align_mean(feat, gp, crop_size).squeeze(0)
        up = nn.functional.interpolate(feat.contiguous(), scale_factor=16, mode='bilinear', align_corners=True)
        crop = crop_feature_align(up, maxind, crop_size).contiguous()
        return crop.view(crop.size(0), crop.size(1), -1).mean(2).squeeze(0)
    pooled = nn.functional.avg_pool2d(gt.float(), 16)                  # the reference's nn.AvgPool2d(16) (host: 14 x 14)
    _, maxind = torch.max(pooled.view(pooled.size(0), pooled.size(1), -1), 2)
    win = [var_window(int(maxind[b].item()), crop_size, feat.size(2), feat.size(3)) for b in range(feat.size(0))]
    if feat.is_cuda:
        from . import hipops as H
        from .functions import to_nhwc
        return H.window_mean(to_nhwc(feat), win).squeeze(0)
    return sequential_mean(crop_feature_var(feat, maxind, crop_size)).squeeze(0)


def sequential_mean(crop):
    """(B,C,h,w) window -> (B,C) spatial mean with egz_window_mean's arithmetic: the cells added one after the other in (y, x)
    order in fp32, then one divide by their number.  torch's ``mean`` adds in several partial sums from 16 elements on, which
    differs in the last bits; with this order host tensors and device tensors give channel_weight the same bits."""
    flat = crop.reshape(crop.size(0), crop.size(1), -1)
    s = torch.zeros_like(flat[:, :, 0])
    for k in range(flat.size(2)):
        s = s + flat[:, :, k]
    return s / flat.size(2)


class _SecondFrame:
    """The fixation state machine (extractLSTMw.py:74-111) fed one flag per frame: the first frame of a fixation arms it,
    the second is the one to extract (True), the rest are skipped until a saccade frame."""
    OUT, ARMED, TAKEN = 0, 1, 2           # no fixation / first fixation frame seen / second frame extracted

    def __init__(self):
        self.state = self.OUT

    def __call__(self, flag):
        fix = float(flag) == 1.0
        if self.state == self.OUT:
            self.state = self.ARMED if fix else self.OUT
        elif self.state == self.ARMED:
            if not fix:
                raise RuntimeError('fixation is not processed.')       # extractLSTMw.py:110-111
            self.state = self.TAKEN
            return True
        elif not fix:
            self.state = self.OUT
        return False


def fixation_second_frames(flags):
    """Indices of the frames extractw extracts, from the fixation flags alone."""
    second = _SecondFrame()
    return [i for i, f in enumerate(flags) if second(f)]


def _shard_loader(loader, shard):
    """The loader of one rank of a sharded extractw: over every ``world``-th of the frames a one-rank run extracts.  Which
    frames those are depends on the flags of ALL frames, so they are read from ``dataset.fixsac`` (STDataset keeps them in
    memory) -- loading every frame on every rank just for its flag would undo the sharding."""
    from . import dp
    rank_, world_ = dp.check_shard(shard)
    flags = getattr(getattr(loader, 'dataset', None), 'fixsac', None)
    if flags is None or len(flags) != len(loader.dataset):
        raise ValueError("a sharded extractw picks the second frame of every fixation before it loads a frame: the dataset "
                         "has to keep one fixation flag per sample in ``dataset.fixsac`` (as STDataset does)")
    return dp.owned_loader(loader, fixation_second_frames(flags)[rank_::world_])


def _check_into(st_set, into, dev):
    """extractw(into=...)'s preconditions, checked before any launch."""
    from .data.lstm_resident import ResidentLSTMDataset
    from .data.resident import check_st_source
    who = "extractw(into=)"
    check_st_source(st_set, dev, who, ('image', 'gt'), "loader", "extraction",
                    "the frames and the ground truth are taken from its pool on the device")
    if not (isinstance(into, ResidentLSTMDataset) and into._handover):
        raise ValueError(f"{who}: into must be a ResidentLSTMDataset.from_st set")
    if into.pool is None or into.pool.device != dev:
        raise ValueError(f"{who}: into.allocate({dev}) has not run")
    index = into.st_index.tolist()
    if (index and max(index) >= len(st_set)) or \
            ['fix_' + st_set.listTrainFiles[i][:-4] + '.pth.tar' for i in index] != list(into.listFiles):
        raise ValueError(f"{who}: into was not planned from this ST dataset")


def _extract_into(loader, model, crop_size, dev, into, chunk):
    """The ``into=`` form of extractw: the set's frames in dataset order, ``chunk`` at a time -- one gather launch over the ST
    pool (the image alone), one encoder forward, one lstm_store launch that reads the ground truth where it lies in the pool
    and writes the vectors into their rows.  Nothing is read back before the last chunk has been queued."""
    from . import hipops as H
    from .functions import to_nhwc
    st_set = loader.dataset
    rows_of = {i: r for r, i in enumerate(into.st_index.tolist())}
    frames = sorted(rows_of)                                      # dataset order; a frame `task` filters out is not forwarded
    index = torch.tensor(frames, dtype=torch.int64)
    rows = torch.tensor([rows_of[i] for i in frames], dtype=torch.int64)      # (host rows: lstm_store checks them without a read-back)
    index_dev = index.to(dev)
    gt_src = st_set.table[:, 21].index_select(0, index_dev).contiguous()
    pending = []
    with torch.no_grad():
        for k0 in range(0, len(frames), chunk):
            k1, status = min(k0 + chunk, len(frames)), {}
            image = H.resident_gather(st_set.pool, st_set.table, index_dev[k0:k1], fields=('image',), status_to=status)[0]
            feat = model(image)                                   # (n,512,14,14)
            H.lstm_store(to_nhwc(feat), st_set.pool, gt_src[k0:k1], into.pool, rows[k0:k1], crop_size, status_to=status)
            pending.append((f"extractw(into=): vectors {k0} .. {k1 - 1}", status))
    # The one place that waits for the device, once (drain_status: the words were copied on this stream, in order).
    H.drain_status(pending, '_lstm_store_status', H.lstm_store_status, H.check_lstm_store_status, H.judge_resident_status)
    into.mark_filled()


def extractw(loader, model, savepath=None, crop_size=3, device='0', align=False, shard=None, into=None, chunk=1):
    """``shard=(rank, world)``: this rank extracts every ``world``-th of the frames a one-rank run extracts and loads no
    others (frames are independent and forwarded at batch 1, so its files are the one-rank run's bit for bit); no
    collective, and file names are per frame, so ranks never collide.

    ``into=lstm_set`` (a data.lstm_resident.ResidentLSTMDataset.from_st set of ``loader.dataset``, allocated on this device):
    no file is written and ``savepath`` is not looked at; every vector goes straight into its row of the set's pool
    (hipops.lstm_store) and the set is marked complete at the end.  ``loader.dataset`` must be a filled ResidentSTDataset on
    this device with the image and the ground truth; the loader itself is not iterated.  The ground truth never leaves the
    device: the gaze cell is found by the kernel, with the summation order of the host's avg_pool2d.  ``chunk`` frames share
    one forward; at ``chunk=1`` (the default) every launch is the file path's, so the pool equals what
    ResidentLSTMDataset.fill reads from that path's files, bit for bit.  A batched forward is another tensor (the abs-max
    scales are per tensor, the conv launches pick their geometry by batch size): ``chunk > 1`` is an opt-in that equals
    model(batch) -> to_nhwc -> window_mean on the same batches, not the files."""
    dev = torch.device(device if str(device).startswith(('cuda', 'cpu')) else 'cuda:' + str(device))
    if into is not None:
        if shard is not None:
            raise ValueError("extractw: into= with shard= is not supported (a sharded extraction leaves every rank with its "
                             "own vectors only)")
        if align:
            raise ValueError("extractw: into= with align=True is not supported (the aligned window is a weight map built on "
                             "the host from the full-resolution arg-max; the in-memory hand-over has no device form of it)")
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f"extractw: chunk must be a positive integer, got {chunk!r}")
        _check_into(getattr(loader, 'dataset', None), into, dev)
        print('extracting lstm training data into device memory...')
        # The file path creates one iterator over the loader, and creating it draws the loader's base seed from torch's global
        # generator.  The same draw is made here (no sample is fetched), so that whatever is seeded after the extraction is
        # what it is after the file path.
        if getattr(loader, 'num_workers', None) == 0:
            iter(loader)
        _extract_into(loader, model, crop_size, dev, into, chunk)
        print('done')
        return
    second = _SecondFrame()
    if shard is not None:
        loader, second = _shard_loader(loader, shard), (lambda flag: True)
    if savepath is None:
        raise ValueError("extractw: savepath is needed (only into= writes no file)")
    print('extracting lstm training data...')
    os.makedirs(savepath, exist_ok=True)
    with torch.no_grad():
        for i, sample in enumerate(loader):
            if not second(sample['fixsac']):
                continue
            if 'jpeg_blob' in sample or 'resident' in sample:     # decode='gpu' / resident pool: the host path's normalised fields, made on the device
                from .data.STdatas import check_decode_status, stage_batch
                image, _, gt = stage_batch(sample, dev)
                check_decode_status(sample)
                sample = dict(sample, image=image, gt=gt.cpu())
            feat = model(sample['image'].float().to(dev))                      # (1,512,14,14)
            w = channel_weight(feat, sample['gt'], crop_size, align).cpu()
            torch.save(w, os.path.join(savepath, 'fix_' + sample['imname'][0][:-4] + '.pth.tar'))
    print('done')


def extract_LSTM_training_data(save_path='../512w', trained_model='save/best_fusion.pth.tar', device='0', crop_size=3,
                               traindata=None, valdata=None, align=False, shard=None, into=None, chunk=1):
    """``into=(train_set, val_set)``: the two ResidentLSTMDataset.from_st sets that take the vectors in device memory
    (extractw(into=...), ``chunk`` frames per forward); nothing is written under ``save_path``."""
    if into is not None and len(into) != 2:
        raise ValueError("extract_LSTM_training_data: into must be (train_set, val_set)")
    model = make_layers(cfg['D'], 3)
    sd = torch.load(trained_model, map_location='cpu', weights_only=False)['state_dict']
    load_merged(model, {k[len('features_s.'):]: v for k, v in sd.items() if k.startswith('features_s.')})
    model.to(torch.device('cuda:' + device)).eval()
    for k, (data, sub) in enumerate(((traindata, 'train'), (valdata, 'test'))):
        loader = extraction_loader(data)
        if into is not None:
            extractw(loader, model, None, crop_size, device, align, shard=shard, into=into[k], chunk=chunk)
            continue
        extractw(loader, model, os.path.join(save_path, sub), crop_size, device, align, shard=shard)
    print('Attention weight for training LSTMnet successfully extracted.')
