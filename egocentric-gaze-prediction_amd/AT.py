"""Mirror of the reference's ``AT.py``: driver of the attention-transition module (AT.py:68-253) -- LSTM training /
validation loops (batch 1, sequence 1, truncated BPTT via repackage_hidden, one Adam step per fixation sample) and
the extraction of the late-fusion training data with the SP model + a forward hook on ``features_s``.
Quirks reproduced, not fixed: the prediction made from sample i-1 is scored against
tanh(target_i) (off-by-one), the loss also crosses video boundaries, and ``prevt`` is never updated so the train
checkpoint is rewritten whenever the epoch loss is below 999."""
import functools
import itertools
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from .data._io import imwrite, resize
from .data.LSTMdatas import deferred_steps
from .data.STdatas import stage_batch, to_raw_u8
from . import hipops as H
from .functions import MSELoss
from .models.LSTMnet import lstmnet
from .models.model_SP import model_SP
from .optim import FusedAdam
from .trainloop import progress as _progress
from .utils import (AverageMeter, cfg, computeAAEAUC, generalException, load_merged, make_layers, owned_state_dict,
                    plot_loss, repackage_hidden)

hook_name = 'features_s'
features_blobs = []


def hook_feature(module, input, output):
    features_blobs.append(output)


def crop_feature(feature, maxind, size):
    """size x size window of the (B,512,14,14) map around gaze_point // 16, clipped to the map (AT.py:25-39)."""
    H = feature.size(2)
    lo, hi = size // 2, int(math.ceil(size / 2.0))
    out = []
    for b in range(feature.size(0)):
        f = np.clip(np.array(maxind[b]) // 16, lo, H - hi)
        out.append(feature[b:b + 1, :, f[0] - lo:f[0] + hi, f[1] - lo:f[1] + hi])
    return torch.cat(out, 0)


def crop_align_feature(feature, maxind, size):
    """Same crop on the bilinearly x16-upsampled map (AT.py:41-56; ``--align``)."""
    size *= 16
    feature = nn.functional.interpolate(feature.contiguous(), scale_factor=16, mode='bilinear', align_corners=True)
    out = []
    for b in range(feature.size(0)):
        f = np.clip(np.array(maxind[b]), size // 2, 224 - size // 2)
        out.append(feature[b:b + 1, :, f[0] - size // 2:f[0] + size // 2, f[1] - size // 2:f[1] + size // 2])
    return torch.cat(out, 0)


def align_window_weights(gp, size, cells=14, scale=16):
    """Per-cell weights W (cells x cells, float64) with  mean(crop of the bilinear x``scale`` upsampling around gp)
    = sum_cells W * map:  the upsampling (align_corners=True, as nn.functional.upsample_bilinear) and the window mean are
    both linear and separable, so W = outer(wy, wx) with 1-D sums of the interpolation weights over the window rows /
    columns.  Window as AT.crop_align_feature (AT.py:41-56): ``size * scale`` pixels around gp, clipped to the image."""
    full, win = cells * scale, size * scale
    out = []
    for f in gp:
        f = min(max(int(f), win // 2), full - win // 2)
        w = np.zeros(cells)
        for y in range(f - win // 2, f + win // 2):
            sy = y * (cells - 1) / (full - 1)
            i0 = min(int(math.floor(sy)), cells - 1)
            i1 = min(i0 + 1, cells - 1)
            fr = sy - i0
            w[i0] += 1 - fr
            w[i1] += fr
        out.append(w / win)
    return np.outer(out[0], out[1])


def crop_align_mean(feature, maxind, size):
    """chn_weight of the ``--align`` path: spatial mean of crop_align_feature(feature, maxind, size) (AT.py:41-56 + :229).
    On the GPU it is one small kernel on the 14 x 14 map (no x16 upsampled tensor, no tensor-library interpolation)."""
    if feature.is_cuda:
        if feature.size(2) != feature.size(3):
            raise NotImplementedError("crop_align_mean on the device is built for square feature maps (the reference's 14 x 14)")
        from . import hipops as H
        from .functions import to_nhwc
        wm = np.stack([align_window_weights(list(map(int, m)), size, feature.size(2)) for m in maxind])
        return H.pixel_weighted_sum(to_nhwc(feature), wm)
    # host tensors: the reference's own formulation (what the device kernel is checked against, tests/test_hip_metrics.py)
    c = crop_align_feature(feature, maxind, size).contiguous()
    return c.view(c.size(0), c.size(1), -1).mean(2)


def crop_mean_weight(feature, maxind, size):
    """chn_weight = spatial mean of crop_feature(feature, maxind, size) (AT.py:25-39 + :229) in one kernel
    (egz_crop_mean) when the map lives on the GPU."""
    if feature.is_cuda:
        from . import hipops as H
        from .functions import to_nhwc
        if isinstance(maxind, torch.Tensor) and maxind.is_cuda:         # gaze points already on the device: no host round trip
            return H.crop_mean(to_nhwc(feature), maxind, size, 16)
        return H.crop_mean(to_nhwc(feature), [list(map(int, m)) for m in maxind], size, 16)
    # host tensors: the reference's own formulation (the device kernel's comparison baseline, tests/test_hip_metrics.py)
    c = crop_feature(feature, maxind, size).contiguous()
    return c.view(c.size(0), c.size(1), -1).mean(2)


def get_weighted_batch(chn_weights, feature):
    """get_weighted for every frame of a chunk: chn_weights (n,512), feature (n,512,14,14) -> (n,14,14), each map
    min-max normalised on its own (AT.py:58-66 applied per frame).  One launch on the GPU (one block per frame)."""
    if feature.is_cuda:
        from . import hipops as H
        from .functions import to_nhwc
        return H.weighted_minmax(to_nhwc(feature), chn_weights.reshape(feature.size(0), -1).contiguous().float())
    # host tensors: AT.py:58-66 per frame (the device kernel's comparison baseline, tests/test_hip_metrics.py)
    f = torch.sum(feature * chn_weights.view(feature.size(0), -1, 1, 1), 1)
    f = f - f.flatten(1).min(1)[0].view(-1, 1, 1)
    return f / f.flatten(1).max(1)[0].view(-1, 1, 1)


def get_weighted(chn_weight, feature):
    """Channel-weighted sum of the (1,512,14,14) map, min-max normalised (AT.py:58-66)."""
    if feature.is_cuda:
        if feature.size(0) != 1:
            raise NotImplementedError("get_weighted takes one frame, like its call sites (AT.py:246); use get_weighted_batch")
        from . import hipops as H
        from .functions import to_nhwc
        return H.weighted_minmax(to_nhwc(feature), chn_weight.reshape(1, -1).contiguous().float())
    # host tensors: the reference's own lines (the device kernel's comparison baseline, tests/test_hip_metrics.py)
    feature = torch.sum(feature * chn_weight.view(1, 512, 1, 1), 1)
    feature = feature - torch.min(feature)
    return feature / torch.max(feature)


AT_GRAPH = os.environ.get("EGAZE_AT_GRAPH", "1") != "0"      # A/B knob: 0 = issue every sample step launch by launch


def _carry_state(state, hn, cn):
    """state (2, L, 1, C) = (hn, cn) of a step.  They share one buffer on the single-step path: one copy carries both."""
    base = getattr(hn, "_base", None)
    if base is not None and base is getattr(cn, "_base", None) and base.numel() == state.numel() and base.is_contiguous():
        H.copy_into(state, base.detach())
    else:
        H.copy_into(state[0], hn.detach().contiguous())
        H.copy_into(state[1], cn.detach().contiguous())


class _GraphedSampleStep:
    """One training step of AT.trainLSTM's loop captured into a hipGraph (the reference issues it per fixation sample,
    AT.py:127-145; ~20 launches plus autograd and optimizer bookkeeping on the host every time):

        pred, (h, c) = lstm(inp, (h, c));  loss = MSE(pred, tanh(target));  zero_grad;  backward;  Adam step

    The forward pass is that of the sample BEFORE the one whose target it is scored against (the schedule:
    data.LSTMdatas.deferred_steps) -- the parameters it sees are the same as in the reference's order (those after the update
    of iteration i-1) and so is every loss, every update and the carried state.  Inputs, state and loss live
    in static buffers; the Adam step counter lives on the device (FusedAdam.set_capturable).  The first ``WARM`` steps run
    eagerly through the same function (they are real training steps), then the step is captured once and replayed.

    ``fetch = (pool, plan, cursor, status)`` (a filled data.lstm_resident.ResidentLSTMDataset): the step's first launch is
    hipops.lstm_pool_fetch, which writes ``both`` and resets ``state`` off the device-side cursor -- in place of step()'s
    host copy and the caller's reset_state(); every launch after it is the same.

    ``optimizer=None``: a step of AT.testLSTM's loop, captured under the caller's torch.no_grad() -- the same unit without
    zero_grad / backward / Adam.  The loss kernel stays hipops.mse_fwd_grad (its gradient output is discarded, its loss is
    bit-identical with hipops.mse_fwd's, csrc/head_loss.hip) because it can park the loss itself.

    Unlike graphs.GraphedTrainStep a replay here repeats no host-side write declaration (hipops.note_replay): the LSTM path
    reads its nn.Parameters directly (GEMM and gate kernels on the flat buffer's views) -- no packed copy, BatchNorm fold or eval
    row keyed by hipops.packing._tag exists for them, so nothing host-side can go stale behind a replay."""
    WARM = 3

    def __init__(self, lstm, optimizer, device, width, ring, counter=None, fetch=None):
        self.lstm, self.opt = lstm, optimizer
        self.fetch = fetch
        self.both = torch.zeros((2, 1, 1, width), device=device)          # (input, target) of the step: ONE host copy fills it
        self.state = torch.zeros((2, lstm.num_layer, 1, lstm.num_channel), device=device)      # (h, c)
        from .models import LSTMnet as _L
        # the (1, 1, C) step runs on the fused single-step path AND every gradient is written in full by a sink -- with
        # hipops.DIRECT_GRADS = False (tests): gradients go through AccumulateGrad and the flat buffer must be zeroed every step
        self.single_step = bool(_L.B1_FUSED) and bool(H.DIRECT_GRADS)
        self.loss = None                     # the loss tensor of the last step (a graph-owned tensor once captured)
        self.graph, self.calls = None, 0
        if optimizer is not None:
            optimizer.set_capturable(True)
            counter = optimizer.step_dev
        # ``ring``: device float tensor in which the loss of every step is parked, slot = counter[0] % len(ring) -- written by the
        # loss kernel itself, so reading the losses back once per ring costs no launch per replay.  ``counter`` is the
        # optimizer's device-side step counter (slot = optimizer steps completed before the step); without an optimizer the
        # caller names it: the step number the fetch left in cursor[1], with one slot per step
        self.ring, self.counter = ring, counter

    def _unit(self):
        if self.fetch is not None:
            pool, plan, cursor, status = self.fetch
            H.lstm_pool_fetch(pool, plan, cursor, self.both[0], self.both[1], self.state, status)
        pred, (hn, cn) = self.lstm(self.both[0], (self.state[0], self.state[1]))
        # criterion(pred, tanh(target)) AND its gradient for the unit seed of loss.backward() in one kernel (AT.py:138-141), which
        # also parks the loss in the ring: the backward pass starts at the network's output
        loss, dpred = H.mse_fwd_grad(H._req(pred.detach().contiguous(), "pred"), self.both[1].view_as(pred).contiguous(), True,
                                     self.ring, self.counter)
        if self.opt is not None:
            # every gradient of a batch-1 step is written in full by the backward kernels (csrc/lstm_b1.hip): no zero fill
            self.opt.zero_grad(all_overwritten=self.single_step)
            pred.backward(gradient=dpred.view_as(pred))
            self.opt.step()
        _carry_state(self.state, hn, cn)       # after the backward pass, which reads the incoming state
        self.loss = loss

    def reset_state(self):
        H.fill_zero(self.state)

    def step(self, host_pair=None):
        """host_pair: pinned (2, width) tensor = (input of the deferred sample, target of the current one) -> loss (0-d);
        None with ``fetch``: the step takes both from the pool."""
        if (host_pair is None) != (self.fetch is not None):
            raise RuntimeError("_GraphedSampleStep.step: a host pair or a resident fetch feeds the step, one of the two")
        if host_pair is not None:
            self.both.copy_(host_pair.view_as(self.both), non_blocking=True)
        if self.graph is None:
            self.calls += 1
            if self.calls <= self.WARM:
                self._unit()
                return self.loss
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            count = self.opt.step_count if self.opt is not None else None
            with H.capture(g, eager_arena=False):
                self._unit()
            if self.opt is not None:
                self.opt.step_count = count    # the capture ran the host side of step() without executing anything
            self.graph = g
        self.graph.replay()
        if self.opt is not None:
            self.opt.note_replays(1)
        return self.loss

    def close(self):
        if self.opt is not None:
            self.opt.set_capturable(False)


RING = 64                                     # _LossRing holds RING // 2 losses and is read back when it is full


class _LossRing:
    """The losses that graphed training steps parked on the device (_GraphedSampleStep's ``ring``), read back for many steps at
    once.  The reference reads every sample's loss back (`losses.update(loss.item())`, AT.py:140) only to average it at the end
    of the epoch: same values, same average, but the host no longer waits for the device after every sample, so replays
    queue back to back (110 -> ~90 us per sample).  ``stepped()`` after every step; ``drain()`` before ``pending`` exceeds
    len(ring) -> the losses of the steps since the last drain, in order.

    ``extra_check(steps since this object was made)`` runs inside the same synchronisation point (the resident loop looks at
    its cursor and status word there)."""

    def __init__(self, ring, optimizer, extra_check=None):
        self.ring, self.opt, self.extra_check = ring, optimizer, extra_check
        self.start = self.first = optimizer.step_count
        self.pending = 0

    def stepped(self):
        self.pending += 1

    def drain(self):
        first, pending = self.first, self.pending
        vals = self.ring.cpu().tolist()                     # one synchronising read-back for `pending` samples
        # the slots are addressed by the DEVICE step counter (egz_mse_fwd_grad parks a loss in ring[counter % len]):
        # an eager optimizer step, a load_state_dict or a skipped replay between two drains would shift them
        # silently -- the counter is read back with the ring and must be where the host thinks it is
        done = int(self.opt.step_dev[0].item())
        if done != first + pending:
            raise RuntimeError(f"AT loss ring out of step: device counter {done}, host expected {first + pending}")
        if self.extra_check is not None:
            self.extra_check(first + pending - self.start)
        # the same synchronisation point also looks at the two device-side failure words: a persistent
        # LSTM hand-off that timed out, and gradient elements the optimizer skipped because they were NaN / inf
        H.lstm_persist_check()
        self.opt.check_finite()
        self.first, self.pending = first + pending, 0
        return [vals[(first + i) % len(vals)] for i in range(pending)]   # slot of a step = optimizer steps completed before it


class AT():
    def __init__(self, pretrained_model=None, pretrained_lstm=None, extract_lstm=False, crop_size=3,
                 num_epoch_lstm=30, lstm_save_img='loss_lstm.png', save_path='save', save_name='best_lstm.pth.tar',
                 device='0', lstm_data_path='../512w', traindata=None, valdata=None, task=None, align=False,
                 shard=None, resident=False, resident_gb=None, lstm_handover=False, lstm_handover_chunk=1):
        """``shard=(rank, world)``: with ``extract_lstm`` every rank of the default process group extracts its share of the
        LSTM training data (extractLSTMw.extractw), then all meet at a barrier so that each lists the complete folders.
        ``resident``: both LSTM datasets are data.lstm_resident.ResidentLSTMDatasets, filled here on the device (``resident_gb``:
        the device memory both pools may take, default 0.8 x what is free); trainLSTM / testLSTM then fetch every step on the
        GPU (_epoch_resident) and compute what they compute from the files, bit for bit.
        ``lstm_handover``: with ``extract_lstm`` and resident ST datasets (data.resident.ResidentSTDataset, filled), no
        ``shard`` and no ``align``: both LSTM datasets are planned from the ST datasets (ResidentLSTMDataset.from_st),
        allocated under what the ST pools left of ``resident_gb``, written on the device by the extraction
        (extractLSTMw.extractw(into=...), ``lstm_handover_chunk`` frames per forward; 1 is the file path's schedule, bit for
        bit) and used as they are: no folder under ``lstm_data_path`` is written, listed or read."""
        if pretrained_model is None:
            raise generalException('AT module have to use pretrained SP module.')
        handover_sets = None
        if lstm_handover:
            handover_sets = self._plan_lstm_handover(extract_lstm, traindata, valdata, shard, align, task)
        self.device = torch.device('cuda:' + device)
        self.lstm = lstmnet().to(self.device)
        if pretrained_lstm is not None:
            self.reload_LSTM(pretrained_lstm)
        self.criterion_lstm = MSELoss.apply
        self.optimizer_lstm = FusedAdam(self.lstm.parameters(), lr=1e-4)
        if handover_sets is not None:
            from .extractLSTMw import extract_LSTM_training_data
            from .data.resident import resident_budget, under_budget
            # both pools before the extraction starts: a pool that does not fit refuses here
            under_budget(handover_sets,
                         resident_budget(self.device, resident_gb, sum(d.needed_bytes for d in (traindata, valdata))),
                         lambda needed, budget: f"lstm_handover: the LSTM vectors need {needed} bytes, {budget} bytes are left "
                                                f"of the budget beside the resident dataset: raise --gpu_resident_gb or run "
                                                f"without --lstm_handover",
                         lambda d, left: d.allocate(self.device, left))
            extract_LSTM_training_data(save_path=None, trained_model=pretrained_model, device=device, crop_size=crop_size,
                                       traindata=traindata, valdata=valdata, align=align, into=handover_sets,
                                       chunk=lstm_handover_chunk)
        elif extract_lstm:
            from .extractLSTMw import extract_LSTM_training_data
            extract_LSTM_training_data(save_path=lstm_data_path, trained_model=pretrained_model, device=device,
                                       crop_size=crop_size, traindata=traindata, valdata=valdata, align=align, shard=shard)
            if shard is not None:
                from . import dp
                dp.barrier()
        self.crop_size, self.num_epoch_lstm, self.epochnow = crop_size, num_epoch_lstm, 0
        self.lstm_save_img, self.save_path, self.save_name = lstm_save_img, save_path, save_name
        self.lstm_data_path, self.batch_size, self.align = lstm_data_path, 1, align
        self.model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
        load_merged(self.model, torch.load(pretrained_model, map_location='cpu', weights_only=False)['state_dict'], strict=False)
        self.model.to(self.device)
        self.model._modules.get(hook_name).register_forward_hook(hook_feature)
        if handover_sets is not None:          # the datasets are the sets the extraction has just written
            self.lstmTrainLoader = DataLoader(dataset=handover_sets[0], batch_size=1, shuffle=False, num_workers=0)
            self.lstmValLoader = DataLoader(dataset=handover_sets[1], batch_size=1, shuffle=False, num_workers=0)
            return
        from .data.LSTMdatas import lstmDataset
        if resident:                           # the vectors live on the device; every step fetches there (data/lstm_resident.py)
            from .data.lstm_resident import ResidentLSTMDataset as lstmDataset
        self.lstmTrainLoader = DataLoader(dataset=lstmDataset(os.path.join(lstm_data_path, 'train'), task),
                                          batch_size=1, shuffle=False, num_workers=0)
        self.lstmValLoader = DataLoader(dataset=lstmDataset(os.path.join(lstm_data_path, 'test'), task),
                                        batch_size=1, shuffle=False, num_workers=0)
        if resident:                           # (after extract_lstm and its barrier: the folders are complete)
            # (not under_budget's shape: a folder's size is known only once its fill has read the first file)
            for loader in (self.lstmTrainLoader, self.lstmValLoader):
                loader.dataset.fill(self.device, resident_gb)
                if resident_gb is not None:    # one budget for both pools
                    resident_gb -= loader.dataset.needed_bytes / 1e9

    @staticmethod
    def _plan_lstm_handover(extract_lstm, traindata, valdata, shard, align, task):
        """``lstm_handover``'s preconditions, then the two planned sets (nothing is allocated, nothing launched)."""
        from .data.lstm_resident import ResidentLSTMDataset
        from .data.resident import ResidentSTDataset
        if not extract_lstm:
            raise ValueError("AT(lstm_handover=True) needs extract_lstm: the vectors exist only in the memory of the run "
                             "that extracts them")
        if shard is not None:
            raise ValueError("AT(lstm_handover=True) runs in one process: a sharded extraction leaves every rank with its "
                             "own vectors only")
        if align:
            raise ValueError("AT(lstm_handover=True) does not take align: the aligned window is built on the host")
        for data in (traindata, valdata):
            if not isinstance(data, ResidentSTDataset) or data.pool is None:
                raise ValueError(f"AT(lstm_handover=True) needs filled ResidentSTDatasets (--gpu_resident), got "
                                 f"{type(data).__name__}: the frames and the ground truth are taken from the pool on the device")
        return tuple(ResidentLSTMDataset.from_st(data, task=task) for data in (traindata, valdata))

    def release_resident(self):
        """Frees the pools of ``resident=True``; the loaders go on reading the files."""
        for loader in (self.lstmTrainLoader, self.lstmValLoader):
            if hasattr(loader.dataset, 'release'):
                loader.dataset.release()

    def reload_LSTM(self, pretrained_lstm):
        load_merged(self.lstm, torch.load(pretrained_lstm, map_location='cpu', weights_only=False))
        print('loaded pretrained lstm from ' + pretrained_lstm)

    def _train_graphed(self, width, steps, feed, fetch=None, extra_check=None):
        """One epoch of trainLSTM with the per-sample step replayed from a hipGraph (_GraphedSampleStep) and the losses read
        back RING // 2 samples at a time (_LossRing).  ``feed(runner, slot, step)`` issues one step of ``steps``; ``slot``
        counts the steps since the last read-back."""
        losses = AverageMeter()
        ring = torch.zeros(RING // 2, device=self.device)
        runner = _GraphedSampleStep(self.lstm, self.optimizer_lstm, self.device, width, ring, fetch=fetch)
        parked = _LossRing(ring, self.optimizer_lstm, extra_check)
        try:
            for step in steps:
                feed(runner, parked.pending, step)
                parked.stepped()
                if parked.pending == RING // 2:
                    for v in parked.drain():
                        losses.update(v)
            if parked.pending:                  # (no read-back for nothing)
                for v in parked.drain():
                    losses.update(v)
        finally:
            runner.close()
        return losses.avg

    def _epoch_graphed(self, loader):
        """trainLSTM's loop over the files: every step's (deferred input, target) pair crosses PCIe out of a pinned stage."""
        steps = deferred_steps((s['input'].reshape(-1).clone(),          # the loader may reuse the storage of a deferred input
                                s['gt'].reshape(-1), int(s['same'])) for s in loader)
        head = next(steps, None)
        if head is None:                        # fewer than two samples: nothing is scored
            return AverageMeter().avg
        width = head[0].numel()
        # The pinned staging ring is as deep as the loss ring: a slot is rewritten only after the read-back that proves its
        # upload was consumed.
        stage = torch.empty((RING // 2, 2, width), dtype=torch.float32).pin_memory()

        def feed(runner, slot, step):
            inp, target, reset = step
            # step on the previous sample's input (forward) scored against THIS sample's target
            pair = stage[slot]
            pair[0].copy_(inp)
            pair[1].copy_(target)
            if reset:                           # the state is reset before the deferred sample's forward pass (AT.py:129-130)
                runner.reset_state()
            runner.step(pair)
        return self._train_graphed(width, itertools.chain((head,), steps), feed)

    def _epoch_resident(self, dataset, train):
        """trainLSTM's / testLSTM's loop over a filled ResidentLSTMDataset: the plan of the epoch (which vector is the input,
        which the target, where the state is reset) is on the device beside the vectors, the step's graph begins with the
        fetch that reads it off a device-side cursor, and the host issues one replay per sample and nothing else."""
        n = dataset.n_steps
        if n == 0:                              # fewer than three files: no scored sample, as over the files
            return AverageMeter().avg
        width = dataset.pool.shape[1]
        # {next step, step being run} and the fetch's sticky status word side by side, then (eval) one loss slot per step as
        # float bits: ONE read-back covers all of them
        buf = torch.zeros(3 + (0 if train else n), dtype=torch.int32, device=self.device)
        fetch = (dataset.pool, dataset.plan, buf[:2], buf[2:3])

        def check_ctl(words, done):
            H.check_lstm_pool_status(words[2])
            if words[0] != done:
                raise RuntimeError(f"AT resident plan out of step: device cursor {words[0]}, host expected {done}")

        if train:
            return self._train_graphed(width, range(n), lambda runner, slot, step: runner.step(), fetch=fetch,
                                       extra_check=lambda done: check_ctl(buf.tolist(), done))
        # validation: the loss of step k is parked in slot k -- the step number the fetch left in cursor[1] is the counter
        runner = _GraphedSampleStep(self.lstm, None, self.device, width, buf[3:].view(torch.float32), counter=buf[1:2],
                                    fetch=fetch)
        with torch.no_grad():
            for _ in range(n):
                runner.step()
        host = buf.cpu()                        # the one synchronising read-back of the epoch
        check_ctl(host[:3].tolist(), n)
        losses = AverageMeter()
        for v in host[3:].view(torch.float32).tolist():
            losses.update(v)
        return losses.avg

    def _epoch(self, loader, train):
        dataset = getattr(loader, 'dataset', None)
        if getattr(dataset, 'filled', False) and self.device.type == 'cuda':
            from .models import LSTMnet as _L
            if _L.B1_FUSED:
                return self._epoch_resident(dataset, train)
        if train and AT_GRAPH and self.device.type == 'cuda':
            return self._epoch_graphed(loader)
        losses = AverageMeter()
        hidden, pred_chn_weight, stage = None, None, None
        for i, sample in enumerate(loader):
            if int(sample['same']) == 0:             # reset the state only when a video is over
                hidden = None
            # (1, 1, 512) input and target: both vectors cross PCIe in ONE asynchronous copy out of a pinned two-slot ring
            # (a pageable .to() is a synchronous staged copy, ~0.1 ms each; the loss read-back below fences slot reuse)
            if stage is None or stage.shape[2] != sample['input'].numel():
                stage = torch.empty((2, 2, sample['input'].numel()), dtype=torch.float32).pin_memory()
            slot = stage[i & 1]
            slot[0].copy_(sample['input'].reshape(-1))
            slot[1].copy_(sample['gt'].reshape(-1))
            both = slot.to(self.device, non_blocking=True)
            inp, target = both[0].view(1, 1, -1), both[1].view(1, 1, -1)
            if pred_chn_weight is not None:
                loss = MSELoss.apply(pred_chn_weight, target, True)       # criterion(pred, tanh(target)), AT.py:138
                if train:
                    self.optimizer_lstm.zero_grad()
                    loss.backward()
                    self.optimizer_lstm.step()
                losses.update(loss.item())
            hidden = repackage_hidden(hidden)
            pred_chn_weight, hidden = self.lstm(inp, hidden)
        if train and self.device.type == 'cuda':
            H.lstm_persist_check()
            self.optimizer_lstm.check_finite()
        return losses.avg

    def trainLSTM(self):
        self.lstm.train()
        return self._epoch(self.lstmTrainLoader, True)

    def testLSTM(self):
        self.lstm.eval()
        with torch.no_grad():
            return self._epoch(self.lstmValLoader, False)

    def train(self):
        print('begin training LSTM...')
        prev, prevt, loss_train, loss_val = 999, 999, [], []
        for epoch in _progress(range(self.num_epoch_lstm)):
            self.epochnow = epoch
            l = self.trainLSTM()
            loss_train.append(l)
            if l < prevt:
                torch.save(owned_state_dict(self.lstm), os.path.join(self.save_path, self.save_name))
            l = self.testLSTM()
            loss_val.append(l)
            if l < prev:
                prev = l
                torch.save(owned_state_dict(self.lstm), os.path.join(self.save_path, 'val' + self.save_name))
            plot_loss(loss_train, loss_val, os.path.join(self.save_path, self.lstm_save_img))
        self.release_resident()                # nothing after the training reads the pools of ``resident=True``
        print('lstm training finished!')

    def _check_into(self, st_set, into):
        """extract_late(into=...)'s preconditions, checked before any launch -> the ResidentSTDataset."""
        from .data.late_resident import ResidentLateDataset
        from .data.resident import check_st_source
        who = "extract_late(into=)"
        check_st_source(st_set, self.device, who, ('image', 'flow', 'gt'), "st_loader", "AT stage",
                        "the frames are taken from its pool on the device")
        if not (isinstance(into, ResidentLateDataset) and into._handover):
            raise ValueError(f"{who}: into must be a ResidentLateDataset.from_st set")
        if into.pool is None or into.pool.device != self.device:
            raise ValueError(f"{who}: into.allocate({self.device}) has not run")
        if len(into.st_index) and int(into.st_index.max()) >= len(st_set) or \
                [st_set.listTrainFiles[i] for i in into.st_index.tolist()] != list(into.listFiles):
            raise ValueError(f"{who}: into was not planned from this ST dataset")
        return st_set

    def extract_late(self, st_loader, pred_folder='../new_pred/', feat_folder='../new_feat/', chunk=32, shard=None, into=None):
        """pred = SP gaze map, feat = AT-weighted conv5_3 map, both written as uint8 PNGs (AT.py:199-253).

        The same sequential LSTM state as the reference's batch-1 loop, but the frames of the (batch-1) loader are gathered
        ``chunk`` at a time: staging (every frame copied into its row of one device buffer per field, on a copy stream, while the
        previous chunk computes), the SP forward (eval mode, every sample independent), the uint8 quantisation, the gaze-point metric, the crop means, the weighted maps and their quantisation
        run once per chunk on the device; the recurrence runs as ONE lstmnet call over the chunk's saccade frames (batch 1, state
        carried in and out), and only the image hand-over (host I/O) stays per frame.  ``chunk=1`` is the reference's schedule.
        A batched forward is NOT bitwise equal to a batch-1 forward (the conv launches pick tile / split-K geometry by batch size, i.e. another fp32 summation order),
        and ``(255 * output).to(uint8)`` truncates: a 1-ulp difference next to an integer flips that pixel by one level.
        Against the reference's own output the chunked path differs by +-1 LSB on < 0.2 % of the pixels
        (tests/test_hip_config5.py), the same class of difference as chunk=1 vs the reference's CPU arithmetic; pass
        ``chunk=1`` when the written PNGs must not depend on the batching.

        ``shard=(rank, world)``: this process is one of ``world`` ranks of the default process group and extracts its share.
        The chunks are dealt out by chunk index (dp.chunk_shards: chunk k on rank k % world), so every frame sits in the chunk
        it has in a one-rank run with the same ``chunk`` -- same launches, same bits.  Per window of ``world`` chunks a rank
        stages and forwards its own chunk only (stage A), the crop means and fixation flags of all chunks are all-gathered,
        EVERY rank runs the window's LSTM calls in chunk order (so the carried state is the same everywhere, bit for bit)
        and keeps the outputs of its own chunk, then weights, quantises and writes its own frames (stage B).  Each rank
        loads only its own frames, through a loader built over its indices of ``st_loader.dataset`` (a shuffling loader is
        refused).  The files written are byte for byte those of ``shard=None``; ``shard=(0, 1)`` needs no process group.

        ``into=late_set`` (a data.late_resident.ResidentLateDataset.from_st set of ``st_loader.dataset``, allocated on this
        device): nothing is written to the folders; every chunk's two planes and its ground truth go straight into the
        set's pool on the device (hipops.late_store) and the set is marked complete at the end.  ``st_loader.dataset`` must be
        a filled ResidentSTDataset on this device with all three fields; its frames are gathered from the pool a chunk at
        a time in dataset order (the loader itself is not iterated), the fixation flags are the dataset's host array, and
        the only waits are for the status words, read once after the last chunk.  The forward of a chunk sees the bits and
        runs the launches of the file path with the same ``chunk``, so the pool equals, byte for byte, what
        ResidentLateDataset.fill decodes from that path's files -- for finite maps in [0, 1]; a NaN AT map (weighted_minmax of
        a constant map) is stored as late_input's 0, which torch's float -> uint8 cast on the file path does not promise."""
        from . import dp
        cap = max(1, int(chunk))
        plan = None
        if into is not None:
            if shard is not None:
                raise ValueError("extract_late: into= with shard= is not supported (a sharded extraction leaves every rank "
                                 "with its own chunks only)")
            st_set = self._check_into(getattr(st_loader, 'dataset', None), into)
        if shard is not None:
            rank_, world_ = dp.check_shard(shard)
            plan = dp.chunk_shards(len(getattr(st_loader, 'dataset', ())), cap, world_)
            st_loader = dp.owned_loader(st_loader, plan.indices(rank_))
        print('begin to extract files for training LF module ...')
        if into is None:
            os.makedirs(pred_folder, exist_ok=True)
            os.makedirs(feat_folder, exist_ok=True)
        global features_blobs
        self.model.eval()
        self.lstm.eval()
        hidden = None

        # Two chunks in flight: while the GPU works on chunk k (queued, results copied to pinned memory asynchronously), the host
        # stages the frames of chunk k + 1 row by row on a copy stream; chunk k's images are handed over (host I/O) when chunk
        # k + 1 has been queued.  The LSTM state is carried on the device in stream order, so the chunks stay sequential.
        from . import streams
        use_copy_stream = self.device.type == 'cuda' and streams.ENABLED
        copy_stream = streams.side_stream("h2d") if use_copy_stream else None
        keys = ('image', 'flow', 'gt')
        prof = getattr(self, "extract_profile", None)                 # optional dict: phase -> seconds (tools/bench_pipeline.py)

        def mark(name, t0):
            if prof is not None:
                torch.cuda.synchronize()
                prof[name] = prof.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()

        class _Chunk:
            def __init__(self):
                self.samples, self.bufs, self.sig, self.done, self.out = [], None, None, None, None

            def add(self, sample, cap):
                """Stage one frame: every field goes straight into its row of ONE device buffer per field (no device-side cat),
                in the loader's own dtype -- bytes for raw_u8 datasets, normalised by one kernel per field at launch."""
                sig = tuple((sample[k].dtype, tuple(sample[k].shape[1:])) for k in keys)
                if self.bufs is None or sig != self.sig or self.bufs[keys[0]].shape[0] < cap:
                    self.sig = sig
                    self.bufs = {k: torch.empty((cap,) + tuple(sample[k].shape[1:]), dtype=sample[k].dtype, device=dev_)
                                 for k in keys}
                    if copy_stream is not None:       # (the blocks may have been freed by work still queued on this stream)
                        copy_stream.wait_stream(torch.cuda.current_stream())
                i = len(self.samples)
                t0 = time.perf_counter()
                if copy_stream is not None:
                    with torch.cuda.stream(copy_stream):
                        for k in keys:
                            self.bufs[k][i:i + 1].copy_(sample[k], non_blocking=True)
                else:
                    for k in keys:
                        self.bufs[k][i:i + 1].copy_(sample[k].to(dev_))
                if prof is not None:
                    prof["stage_host"] = prof.get("stage_host", 0.0) + time.perf_counter() - t0
                self.samples.append(sample)

        dev_ = self.device

        def stage_a(ch, n, staged=None):
            """Own frames up to the crop means: normalise, SP forward, uint8 quantisation, gaze point, crop means (n,512).
            ``staged``: the chunk's (image, flow, gt) already normalised on the device (the ``into=`` path's gather)."""
            t0 = time.perf_counter()
            if copy_stream is not None:
                torch.cuda.current_stream().wait_stream(copy_stream)
            input_s, input_t, target = staged or stage_batch({k: ch.bufs[k][:n] for k in keys}, self.device)
            t0 = mark("normalise", t0)
            del features_blobs[:]
            output = self.model(input_s, input_t)                     # (n,1,224,224)
            ch.sp = output
            feature_s = features_blobs[0]                             # (n,512,14,14)
            t0 = mark("sp_forward", t0)
            quant = (255 * output).to(torch.uint8)                    # np.uint8(255 * x): truncation, on the device
            # computeAAEAUC's third value is the GROUND-TRUTH arg-max, used as the "predicted" gaze point
            # (AT.py:221-224); evaluated on the quantised map like the reference, by the device kernel
            if self.device.type == 'cuda' and not self.align:
                # the same device kernel computeAAEAUC uses, its gaze point kept on the device (no read-back in the chunk)
                from . import hipops as H
                pred_gp = H.aae_auc(quant.float().squeeze(1), target.squeeze(1))[:, 2:4].to(torch.int32).contiguous()
            else:
                _, _, pred_gp = computeAAEAUC(quant.float().squeeze(1), target.squeeze(1))
            t0 = mark("metric", t0)
            if self.align:
                chn_weights = crop_align_mean(feature_s, pred_gp, self.crop_size)            # (n,512)
            else:
                chn_weights = crop_mean_weight(feature_s, pred_gp, self.crop_size)           # (n,512)
            mark("crop", t0)
            return quant, feature_s, chn_weights

        def chain(rows, flags):
            """The recurrent part of ONE chunk.  A fixation frame (fixsac == 1) keeps its crop mean and leaves the state alone;
            the saccade frames of the chunk, in order, are ONE lstmnet call over T' = their count steps at batch 1 (inputs
            known up front, state carried in and out): the same recurrence as the reference's frame-by-frame calls
            (AT.py:240-246).  ``rows`` (n,512) crop means, ``flags`` the frames' int(fixsac) -> (saccade indices, (T',512))
            or (None, None) when the chunk has no saccade frame (no call, the state stays)."""
            nonlocal hidden
            sacc = [i for i, f in enumerate(flags) if f != 1]
            if not sacc:
                return None, None
            idx = torch.tensor(sacc, device=rows.device)
            hidden = repackage_hidden(hidden)
            seq, hidden = self.lstm(rows.index_select(0, idx).unsqueeze(1), hidden)      # (T',1,512)
            return idx, seq.squeeze(1)

        def stage_b(ch, n, quant, feature_s, chn_weights):
            """Own frames from the final channel weights on: weighted maps, quantisation, asynchronous read-back."""
            t0 = time.perf_counter()
            feats = get_weighted_batch(chn_weights, feature_s)        # (n,14,14): one launch for the chunk (AT.py:58-66 per frame)
            featq = (255 * feats).to(torch.uint8)                     # np.uint8(255 * x) on the device
            if self.device.type == 'cuda':
                if ch.out is None or ch.out[0].shape[0] < n:
                    ch.out = (torch.empty(quant.shape, dtype=torch.uint8).pin_memory(),
                              torch.empty(featq.shape, dtype=torch.uint8).pin_memory())
                ch.out[0][:n].copy_(quant, non_blocking=True)          # two read-backs per chunk, asynchronous
                ch.out[1][:n].copy_(featq, non_blocking=True)
                ch.done = torch.cuda.Event()
                ch.done.record()
            else:
                ch.out, ch.done = (quant, featq), None
            mark("weighted_readback", t0)

        def launch(ch):
            """Queue the whole device side of a chunk; nothing here waits for the GPU."""
            n = len(ch.samples)
            quant, feature_s, chn_weights = stage_a(ch, n)
            t0 = time.perf_counter()
            idx, seq = chain(chn_weights, [int(sm['fixsac']) for sm in ch.samples])
            if idx is not None:
                chn_weights = chn_weights.index_copy(0, idx, seq)
            mark("lstm", t0)
            stage_b(ch, n, quant, feature_s, chn_weights)

        def launch_window(ch, w):
            """The sharded form of launch(): ``ch`` is this rank's chunk of the window (possibly empty).  The one point that
            waits is the gather: the fixation flags are host data every rank needs before it can shape the LSTM calls, and a
            backend without device collectives is fed the crop means from host memory."""
            n = len(ch.samples)
            if n:
                quant, feature_s, chn_weights = stage_a(ch, n)
            t0 = time.perf_counter()
            rows = torch.zeros((cap, 512), dtype=torch.float32, device=self.device)      # rows padded to the chunk size
            meta = torch.zeros(cap + 1, dtype=torch.int32)                                # row count, then int(fixsac) per row
            if n:
                rows[:n].copy_(chn_weights)
                meta[0] = n
                meta[1:n + 1] = torch.tensor([int(sm['fixsac']) for sm in ch.samples], dtype=torch.int32)
            all_meta = [m.tolist() for m in dp.all_gather(meta)]
            all_rows = dp.all_gather(rows)
            t0 = mark("gather", t0)
            for r in range(world_):
                n_r = all_meta[r][0]
                if n_r != len(plan.window(w, r)):
                    raise RuntimeError(f"sharded extract_late: rank {r} brought {n_r} frames to window {w}, "
                                       f"the plan gives it {len(plan.window(w, r))}")
                idx, seq = chain(all_rows[r][:n_r], all_meta[r][1:n_r + 1])
                if r == rank_ and idx is not None:
                    chn_weights = chn_weights.index_copy(0, idx, seq)
            mark("lstm", t0)
            if n:
                stage_b(ch, n, quant, feature_s, chn_weights)

        def finish(ch):
            """Hand the images of a queued chunk over (host I/O) once its results have landed."""
            if not ch.samples:
                return
            t0 = time.perf_counter()
            if ch.done is not None:
                ch.done.synchronize()
            n = len(ch.samples)
            outims, featims = ch.out[0][:n].numpy(), ch.out[1][:n].numpy()
            for i, sm in enumerate(ch.samples):
                currname = sm['imname'][0]
                imwrite(os.path.join(pred_folder, currname), outims[i].squeeze())
                imwrite(os.path.join(feat_folder, currname), resize(featims[i], (224, 224)))
            ch.samples = []
            if prof is not None:
                prof["finish_host"] = prof.get("finish_host", 0.0) + time.perf_counter() - t0

        def store_chunks():
            """The ``into=`` form: per chunk one gather launch over the ST pool, the forward and the LSTM call of launch(), and
            one late_store launch; nothing is read back before the last chunk has been queued."""
            N = len(st_set)
            order = torch.arange(N, dtype=torch.int64, device=self.device)
            rows = torch.full((N, 3), -1, dtype=torch.int64)          # a frame that `task` leaves out is forwarded, not stored
            rows[into.st_index] = into.plane_table                    # (host rows: late_store checks them without a read-back)
            pending, ch = [], _Chunk()
            for k0 in _progress(range(0, N, cap)):
                k1 = min(k0 + cap, N)
                n, idx, status = k1 - k0, order[k0:k1], {}
                t0 = time.perf_counter()
                staged = H.resident_gather(st_set.pool, st_set.table, idx, fields=keys, status_to=status)
                mark("gather", t0)
                quant, feature_s, chn_weights = stage_a(ch, n, staged)
                t0 = time.perf_counter()
                at_idx, seq = chain(chn_weights, [int(f) for f in st_set.fixsac[k0:k1]])
                if at_idx is not None:
                    chn_weights = chn_weights.index_copy(0, at_idx, seq)
                t0 = mark("lstm", t0)
                feats = get_weighted_batch(chn_weights, feature_s)    # (n,14,14), as stage_b
                H.late_store(ch.sp.reshape(n, *ch.sp.shape[-2:]), feats.contiguous(), into.pool, rows[k0:k1], gt_pool=st_set.pool,
                             gt_src=st_set.table[k0:k1, 21].contiguous(), status_to=status)
                mark("late_store", t0)
                pending.append((f"extract_late(into=): frames {k0} .. {k1 - 1}", status))
            # the one place that waits for the device (the warning of a clamped map points here)
            H.drain_status(pending, '_late_store_status', H.late_store_status,
                           functools.partial(H.check_late_store_status, stacklevel=3), H.judge_resident_status)

        if into is not None:
            # The file path creates one iterator over st_loader, and creating it draws the loader's base seed from torch's
            # global generator.  The same draw is made here (no sample is fetched), so that whatever is seeded after the
            # extraction -- LF's initial weights, its shuffles -- is what it is after the file path.
            if getattr(st_loader, 'num_workers', None) == 0:
                iter(st_loader)
            with torch.no_grad():
                store_chunks()
            H.lstm_persist_check()
            into.mark_filled()
            print('Finished extracting the LF planes into device memory!')
            return

        ring, cur, prev = [_Chunk(), _Chunk()], 0, None
        kept = getattr(self, "_extract_buffers", None)               # device / pinned buffers survive across calls
        if kept is not None:
            for ch, (bufs, sig, out) in zip(ring, kept):
                ch.bufs, ch.sig, ch.out = bufs, sig, out

        def step(queue, *at):
            """Queue the staged chunk, then hand over the one queued before it."""
            nonlocal cur, prev
            queue(ring[cur], *at)
            if prev is not None:
                finish(ring[prev])
            prev, cur = cur, 1 - cur

        with torch.no_grad():
            if plan is None:
                for i, sample in _progress(enumerate(st_loader)):
                    ring[cur].add(to_raw_u8(sample, self.device), cap)
                    if len(ring[cur].samples) >= cap:
                        step(launch)
                if ring[cur].samples:
                    step(launch)
            else:
                frames = iter(st_loader)
                for w in _progress(range(plan.windows)):
                    for _ in plan.window(w, rank_):
                        ring[cur].add(to_raw_u8(next(frames), self.device), cap)
                    step(launch_window, w)
            if prev is not None:
                finish(ring[prev])
        self._extract_buffers = [(ch.bufs, ch.sig, ch.out) for ch in ring]
        if self.device.type == 'cuda':
            H.lstm_persist_check()          # every chunk has been read back: a lost in-launch hand-off of the saccade-frame LSTM calls surfaces here
        print('Finished extracting files for LF module!')
