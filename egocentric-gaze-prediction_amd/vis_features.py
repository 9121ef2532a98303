"""Mirror of the reference's ``vis_features.py``: what the attention-transition module does, drawn over the frames.

For every visualised batch, three channel-weighted maps of the spatial encoder's output ``features_s`` (B, 512, 14, 14),
each min-max normalised, truncated to uint8, resized to 224 x 224 (INTER_LINEAR), coloured with COLORMAP_JET and blended over
the frame (``heatmap * 0.3 + img * 0.5``):
  gt_        weights = mean of the 5 x 5 / 6 x 6 window of features_s around the ground-truth gaze cell
  noweight_  weights of one (a plain channel sum)
  pred_      weights = the LSTM output of the previous visualised batch (from the second visualised batch on)
and the ground-truth map itself (gaze_).  The reference does not run as written (``batch_size`` undefined, a four-argument
model call, ``torch.cat`` of windows of different shapes); the meaning pinned here is listed in INTEGRATION.md.

Device side: the model_SP forward (eval, no_grad) with features_s hooked, the gt cell (egz_cell_argmax_u8), the window means
(egz_window_mean), the weighted maps (egz_weighted_minmax), the uint8 truncation, the LSTM (lstmnet, T = B at batch 1, state
carried across batches) and every overlay of a batch in ONE egz_heatmap_overlay launch, read back once into pinned memory.
Only the file writing runs on the host; with ``--gpu_encode`` the JPEG encoding of the overlays and the gaze map runs on the
device too (hipops.jpeg_encode, quality 95, byte-identical files) and the host writes the bytes.

    python -m egaze_amd.vis_features --flowPath ../gtea_imgflow --imagePath ../gtea_images --gtPath ../gtea_gts \\
        --fixsacPath ../fixsac --trained_model save/best_fusion.pth.tar --trained_lstm save/valbest_lstm.pth.tar \\
        --savefolder vis
"""
import argparse
import math
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from .data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD, STDataset, to_raw_u8
from .data._io import imwrite_bgr
from .models.LSTMnet import lstmnet
from .models.model_SP import model_SP
from .utils import cfg, load_merged, make_layers, repackage_hidden

hook_name = 'features_s'

features_blobs = []

FRAME_HW = (224, 224)
CROP = 5
CELL = 16


def hook_feature(module, input, output):
    features_blobs.append(output)


def crop_window(ind, H, W, size=CROP):
    """The reference's crop of vis_features.crop_feature_var for the flat cell index ``ind`` of an H x W map: both
    coordinates clipped (as integers) to [int(size / 2), H - ceil(size / 2)], then rows int(r - size / 2) : r + ceil(size / 2)
    and columns int(c - size / 2) : c + ceil(size / 2).  For size 5: a 5-cell window at clipped index 2, 6 cells elsewhere.
    -> (y0, y1, x0, x1), half-open."""
    r, c = np.unravel_index(int(ind), (H, W))
    hi = int(math.ceil(size / 2.0))
    r, c = np.clip((r, c), int(size / 2), H - hi)
    return int(r - size / 2), int(r + hi), int(c - size / 2), int(c + hi)


def crop_feature_var(feature, maxind, size):
    """Per row b of ``feature`` (B, C, H, W) on the GPU: the mean over the crop_window of cell maxind[b] -> (B, C).  The
    reference concatenates the crops (and raises when their shapes differ) only to take this mean."""
    from . import hipops as H
    from .functions import to_nhwc
    fn = to_nhwc(feature)
    inds = maxind.reshape(-1).tolist() if isinstance(maxind, torch.Tensor) else [int(v) for v in np.ravel(maxind)]
    return H.window_mean(fn, [crop_window(v, fn.shape[1], fn.shape[2], size) for v in inds])


class _Pinned:
    """Grow-only pinned host buffer for the per-batch read-back."""

    def __init__(self):
        self.buf = None

    def take(self, src):
        n = src.numel()
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(n, dtype=torch.uint8).pin_memory()
        dst = self.buf[:n].view(src.shape)
        dst.copy_(src, non_blocking=True)
        return dst


def _is_jpeg(name):
    return name.lower().endswith(('.jpg', '.jpeg'))


def _write_bytes(path, data):
    with open(path, 'wb') as fh:
        fh.write(data)


def vis_features(st_loader, model, modelw, savefolder, first=100, last=1000, all_frames=False, lut=None, writer=None,
                 gpu_encode=False):
    """Visualise batches first .. last of ``st_loader`` (the reference's ``i < 100`` / ``i > 1000`` window) into
    ``savefolder``.  The loader must deliver bytes: an ``STDataset(raw_u8=True)`` or ``decode='gpu'`` loader, frames of
    224 x 224.  model: a model_SP (its features_s output is hooked); modelw: an lstmnet.  Row 0 of each batch is written, as in the
    reference; ``all_frames`` writes every row.  lut: (256, 3) uint8 BGR colormap (default hipops.jet_lut).  writer:
    callable (path, uint8 array) -- default cv2.imwrite, or PIL at JPEG quality 95.  gpu_encode: images whose name ends in
    .jpg / .jpeg are encoded on the device (hipops.jpeg_encode, quality 95) and written as bytes; others go to the default
    writer.  A ``writer`` receives arrays, so it cannot be combined with gpu_encode."""
    from . import hipops as H
    if gpu_encode and writer is not None:
        raise ValueError("vis_features: gpu_encode writes encoded files itself; it cannot be combined with writer=")
    dev = next(model.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError("vis_features: the model must live on a HIP device -- this package has no CPU path")
    model.eval()
    modelw.eval()
    if lut is None:
        lut = H.jet_lut(dev)
    else:
        lut = torch.as_tensor(np.asarray(lut.cpu() if isinstance(lut, torch.Tensor) else lut, dtype=np.uint8))
        lut = lut.reshape(256, 3).contiguous().to(dev)
    writer = writer or imwrite_bgr
    # features_s as a full model_SP forward hooks it: the spatial encoder run alone gives values that differ in the last bits
    # (DESIGN.md section 12), so the whole forward runs and its output is dropped
    seen = []
    handle = model.features_s.register_forward_hook(lambda m, i, o: seen.append(o))
    try:
        _run(st_loader, model, modelw, savefolder, first, last, all_frames, lut, writer, dev, seen, gpu_encode)
    finally:
        handle.remove()
    H.lstm_persist_check()


def _run(st_loader, model, modelw, savefolder, first, last, all_frames, lut, writer, dev, seen, gpu_encode=False):
    from . import hipops as H
    from .functions import to_nhwc
    pinned = _Pinned()
    hidden = None
    pred = None                                   # (B, 512): the previous visualised batch's LSTM output
    with torch.no_grad():
        for i, sample in enumerate(st_loader):
            if i < first:
                continue
            if i > last:
                break
            sample = to_raw_u8(sample, dev)
            image, gt = sample['image'], sample['gt']
            if image.dtype != torch.uint8 or gt.dtype != torch.uint8:
                raise ValueError("vis_features: the loader must deliver bytes (STDataset(raw_u8=True) or decode='gpu')")
            if tuple(image.shape[-2:]) != FRAME_HW or tuple(gt.shape[-2:]) != FRAME_HW:
                raise ValueError(f"vis_features: frames and gaze maps must be {FRAME_HW} (the reference resizes its maps to "
                                 f"224 x 224 and blends them over the frame), got {tuple(image.shape)} / {tuple(gt.shape)}")
            image = image.to(dev, non_blocking=True).contiguous()
            gt = gt.to(dev, non_blocking=True).contiguous()
            B = image.shape[0]
            flow = sample['flow'].to(dev, non_blocking=True).contiguous()
            del seen[:]
            model(H.u8_normalize(image, IMAGE_MEAN, IMAGE_STD), H.u8_normalize(flow, FLOW_MEAN, FLOW_STD))
            feat = to_nhwc(seen[0])                                        # hooked features_s: (B, 14, 14, 512)
            Hf, Wf = feat.shape[1], feat.shape[2]
            cells = H.cell_argmax_u8(gt, CELL).cpu().tolist()
            chn_weight = H.window_mean(feat, [crop_window(c, Hf, Wf, CROP) for c in cells])     # (B, 512)
            weights = [('gt_', chn_weight), ('noweight_', torch.ones_like(chn_weight))]
            if pred is not None:
                if pred.shape[0] < B:
                    raise ValueError(f"vis_features: batch of {B} after a batch of {pred.shape[0]}")
                weights.append(('pred_', pred[:B].contiguous()))
            rows = list(range(B)) if all_frames else [0]
            maps = [(255 * H.weighted_minmax(feat, w)).to(torch.uint8) for _, w in weights]   # np.uint8(255 * x)
            sel = torch.stack([m[b] for m in maps for b in rows]).contiguous()
            ov = H.heatmap_overlay(sel, image, [b for _ in maps for b in rows], lut)
            names = sample['imname']
            enc = gpu_encode and all(_is_jpeg(names[b]) for b in rows)
            if enc:
                ov_j = H.jpeg_encode(ov, quality=95)
                gaze_j = H.jpeg_encode(gt[rows].reshape(len(rows), *FRAME_HW), quality=95)
            else:
                ov_h = pinned.take(ov)
                gaze_h = gt[rows].reshape(len(rows), *FRAME_HW).cpu()
            # the recurrence: the batch's rows are a T = B sequence at batch 1, the state carried over from the previous batch
            hidden = repackage_hidden(hidden)
            out, hidden = modelw(chn_weight.unsqueeze(1), hidden)         # (B, 1, 512)
            pred = out.reshape(B, -1)
            torch.cuda.current_stream().synchronize()
            if enc:
                (ov_b, ov_o), (gz_b, gz_o) = ((j[0].cpu().numpy(), j[1].cpu().tolist()) for j in (ov_j, gaze_j))
                for k, (prefix, _) in enumerate(weights):
                    for j, b in enumerate(rows):
                        m = k * len(rows) + j
                        _write_bytes(os.path.join(savefolder, prefix + names[b]), ov_b[ov_o[m]:ov_o[m + 1]])
                for j, b in enumerate(rows):
                    _write_bytes(os.path.join(savefolder, 'gaze_' + names[b]), gz_b[gz_o[j]:gz_o[j + 1]])
                continue
            for k, (prefix, _) in enumerate(weights):
                for j, b in enumerate(rows):
                    writer(os.path.join(savefolder, prefix + names[b]), ov_h[k * len(rows) + j].numpy())
            for j, b in enumerate(rows):
                writer(os.path.join(savefolder, 'gaze_' + names[b]), gaze_h[j].numpy())


def _load_into(module, path):
    """The reference's ``model_dict.update(torch.load(path)); load_state_dict(model_dict)`` (a checkpoint holding a
    'state_dict' entry is unwrapped first)."""
    sd = torch.load(path, map_location='cpu', weights_only=False)
    if isinstance(sd, dict) and 'state_dict' in sd:
        sd = sd['state_dict']
    load_merged(module, sd)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--flowPath', default='../gtea_imgflow')
    p.add_argument('--imagePath', default='../gtea_images')
    p.add_argument('--gtPath', default='../gtea_gts')
    p.add_argument('--fixsacPath', default='../fixsac')
    p.add_argument('--val_name', default='Alireza')
    p.add_argument('--batch_size', type=int, default=10)
    p.add_argument('--trained_model', default='save/best_fusion.pth.tar')
    p.add_argument('--trained_lstm', default='save/valbest_lstm.pth.tar')
    p.add_argument('--savefolder', default='vis')
    p.add_argument('--first', type=int, default=100)
    p.add_argument('--last', type=int, default=1000)
    p.add_argument('--all_frames', action='store_true')
    p.add_argument('--gpu_decode', action='store_true', help="decode the JPEG frames on the GPU (STDataset(decode='gpu'))")
    p.add_argument('--gpu_encode', action='store_true', help="encode the written JPEGs on the GPU (hipops.jpeg_encode)")
    p.add_argument('--device', default='0', help='GPU index')
    args = p.parse_args(argv)

    folders = sorted(os.listdir(args.flowPath))
    val_gts = sorted(k for k in os.listdir(args.gtPath) if args.val_name in k)
    val_fixsac = sorted(k for k in os.listdir(args.fixsacPath) if args.val_name in k)
    val_files = sorted(k for k in os.listdir(args.imagePath) if args.val_name in k)
    print('num of val samples: ', len(val_files))
    data = STDataset(args.flowPath, args.imagePath, args.gtPath, folders, val_files, val_gts, val_fixsac, args.fixsacPath,
                     raw_u8=True, decode='gpu' if args.gpu_decode else 'host')
    loader = DataLoader(dataset=data, batch_size=args.batch_size, shuffle=False, num_workers=0, pin_memory=True,
                        collate_fn=data.collate_fn)
    device = torch.device('cuda:' + args.device)
    torch.cuda.set_device(device)
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    _load_into(model, args.trained_model)
    model.to(device)
    lstm = lstmnet()
    _load_into(lstm, args.trained_lstm)
    lstm.to(device)
    os.makedirs(args.savefolder, exist_ok=True)
    vis_features(loader, model, lstm, args.savefolder, first=args.first, last=args.last, all_frames=args.all_frames,
                 gpu_encode=args.gpu_encode)


if __name__ == '__main__':
    main()
