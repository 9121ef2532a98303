"""Mirror of the reference's ``LF.py``: driver of the late-fusion module (LF.py:16-161) -- file listing with
leave-one-subject-out split, Adam, train / validation loops with per-batch AAE / AUC, best-train and best-val
checkpoints.  Model, loss and optimizer are the HIP-backed mirrors.  ``LF(resident=True)`` keeps the three maps of every
frame in device memory and gathers each batch there (data/late_resident.py); the default reads the files as the reference."""
import os

import torch

from . import dp
from .data.lateDataset import lateDataset
from .models.late_fusion import late_fusion
from .optim import FusedAdam
from .trainloop import (EpochMeters, ReplayOrEager, make_criterion, progress as _progress, rank_loaders,
                        split_by as _split)
from .utils import aae_auc_from_rows, aae_auc_rows, computeAAEAUC, load_merged, owned_state_dict, plot_loss

LF_GRAPH = os.environ.get("EGAZE_LF_GRAPH", "1") != "0"      # A/B knob: 0 = issue every LF training step launch by launch


class GraphedLateIteration:
    """LF.trainLate's iteration (LF.py:90-100) -- late_fusion forward, loss, the batch's AAE / AUC (computeAAEAUC, LF.py:92-94),
    zero_grad, backward, Adam -- as ONE hipGraph replay (graphs.GraphedTrainStep), the metric kernel included.  The reference
    reads the loss and both maps back every iteration only to feed three running averages; here the loss and the metric's 6
    doubles per sample are copied into pinned host slots asynchronously and read RING iterations at a time (``drain``): the
    same values reach the same meters in the same order, but the host no longer waits for the device after every replay
    (the per-iteration read-back cost 0.22 ms of a 1.44 ms iteration, profiles/r04_lf_step.txt)."""
    RING = 16

    def __init__(self, model, criterion, optimizer, example):
        """``example``: (feat, im, gt), or (fused, gt) of a resident batch (data.late_resident: the two maps come out of the
        gather as the (B,2,H,W) tensor the fusion stack reads, so no cat2_planes launch is in the step)."""
        from .graphs import GraphedTrainStep

        def fwd_loss(*maps):
            o = _forward(model, maps)
            l = criterion(o, maps[-1])
            rows, _ = aae_auc_rows(o, maps[-1])               # device kernel, maps stay in HBM (LF.py:92-94)
            return l, o, rows
        self.step = GraphedTrainStep(fwd_loss, optimizer, example)
        self.shape = tuple(example[0].shape)
        self.h_rows = torch.empty((self.RING, self.shape[0], 6), dtype=torch.float64).pin_memory()
        self.h_loss = torch.empty((self.RING,), dtype=torch.float32).pin_memory()
        self.pending = 0

    def __call__(self, *maps):
        loss, out, rows = self.step(*maps)
        self.h_rows[self.pending].copy_(rows, non_blocking=True)
        self.h_loss[self.pending].copy_(loss, non_blocking=True)
        self.pending += 1
        return out

    @property
    def full(self):
        return self.pending >= self.RING

    def drain(self):
        """-> [(loss, aae, auc)] of the iterations since the last drain, oldest first (one synchronisation for all of them)."""
        if not self.pending:
            return []
        torch.cuda.current_stream().synchronize()
        done = []
        for k in range(self.pending):
            aae1, auc1, _ = aae_auc_from_rows(self.h_rows[k].numpy())
            done.append((float(self.h_loss[k]), aae1, auc1))
        self.pending = 0
        return done

    def close(self):
        self.step.close()


def _stage_late(sample, device):
    return tuple(sample[k].float().to(device, non_blocking=True) for k in ('im', 'gt', 'feat'))


def _stage_late_resident(sample, device):
    """(fused, gt) of a resident batch: one gather launch on the copy stream; staged_batches reads its status at hand-over."""
    return sample['resident'].gather(sample, device)


def _maps(staged):
    """A staged batch in the step's argument order: (feat, im, gt) of the file loader, (fused, gt) of the resident set."""
    if len(staged) == 2:
        return staged
    im, gt, feat = staged
    return feat, im, gt


def _forward(model, maps):
    if len(maps) == 2:                                        # the gather built late_fusion.forward's Cat2Planes tensor
        return model.fusion(maps[0], fuse_sigmoid=True)
    return model(maps[0], maps[1])                            # channel 0 = AT map, channel 1 = SP map (LF.py:90)


class LF():
    stage = staticmethod(_stage_late)           # staged_batches' stage function; resident=True replaces it on the instance

    def __init__(self, pretrained_model=None, save_path='save', late_save_img='loss_late.png',
                 save_name='best_late.pth.tar', device='0', late_pred_path='../new_pred', num_epoch=10,
                 late_feat_path='../new_feat', gt_path='../gtea_gts', val_name='Alireza', batch_size=32,
                 loss_function='f', lr=1e-7, task=None, resident=False, decode='host', resident_gb=None, datasets=None):
        """``resident``: both datasets are data.late_resident.ResidentLateDatasets, filled here (``decode``: how the one-time
        fill decodes; ``resident_gb``: the device memory both pools may take, default 0.8 x what is free); the loaders, their
        samplers and their RNG draws stay the file loader's, so a seeded run draws the same batches.  Under
        torch.distributed every rank fills its own full pool.  ``datasets=(train_set, val_set)``: two complete resident sets
        on this device (ResidentLateDataset.from_st sets that AT.extract_late(into=...) has written) are used as they are: no
        folder is listed, no file is read, and everything downstream is ``resident=True``'s."""
        self.model = late_fusion()
        self.device = torch.device('cuda:' + device)
        self.save_name, self.save_path = save_name, save_path
        if pretrained_model is not None:
            load_merged(self.model, torch.load(pretrained_model, map_location='cpu', weights_only=False)['state_dict'])
            print('loaded pretrained late fusion model from ' + pretrained_model)
        self.model.to(self.device)
        self.batch_size, self.num_epoch, self.epochnow, self.late_save_img = batch_size, num_epoch, 0, late_save_img
        if datasets is not None:
            train_set, val_set = self._given_sets(datasets)
        else:
            train_set, val_set = self._listed_sets(late_pred_path, late_feat_path, gt_path, val_name, task, resident, decode,
                                                   resident_gb)
        # (LF.py:69-72; no worker: lateDataset declares no loader_workers, the resident sets declare 0)
        self.train_loader, self.val_loader, self.train_sampler = rank_loaders(train_set, val_set, batch_size, 0)
        self.criterion = make_criterion(loss_function, self.device)
        self.optimizer = FusedAdam(self.model.parameters(), lr=lr)
        self.reducer = dp.attach(self.optimizer) if torch.distributed.is_initialized() else None
        from . import hipops
        print(hipops.precision_banner())

    def _given_sets(self, datasets):
        """``datasets=(train_set, val_set)``: two complete ResidentLateDatasets on this device, used as they are."""
        from .data.late_resident import ResidentLateDataset
        try:
            train_set, val_set = datasets
        except (TypeError, ValueError):
            raise ValueError("LF: datasets must be (train_set, val_set)") from None
        for name, ds in (("training", train_set), ("validation", val_set)):
            if not isinstance(ds, ResidentLateDataset):
                raise ValueError(f"LF: datasets: the {name} set must be a ResidentLateDataset, got {type(ds).__name__}")
            if not ds.filled:
                raise ValueError(f"LF: datasets: the {name} set is not complete (fill(), or AT.extract_late(into=...))")
            if ds.pool.device != self.device:
                raise ValueError(f"LF: datasets: the {name} set's pool is on {ds.pool.device}, LF runs on {self.device}")
        print('num of training LF samples: %d' % len(train_set))
        print('num of LF val samples: ', len(val_set))
        assert(len(train_set) > 0)
        self.stage = _stage_late_resident
        return train_set, val_set

    def _listed_sets(self, late_pred_path, late_feat_path, gt_path, val_name, task, resident, decode, resident_gb):
        """The two datasets over the hand-over folders, as the reference lists them (LF.py:44-68)."""
        listGtFiles, listValGtFiles = _split(gt_path, val_name, task)
        print('num of training LF samples: %d' % len(listGtFiles))
        print('Loading SP predictions from /%s' % late_pred_path)
        listTrainFiles, listValFiles = _split(late_pred_path, val_name, task)
        print('num of LF val samples: ', len(listValFiles))
        listTrainFeats, listValFeats = _split(late_feat_path, val_name, task)
        assert(len(listTrainFeats) == len(listTrainFiles) and len(listGtFiles) > 0)
        assert(len(listValGtFiles) == len(listValFiles))
        if resident:                           # the planes live on the device; batches are gathered there (data/late_resident.py)
            from .data.late_resident import ResidentLateDataset
            from .data.resident import fill_all
            train_set = ResidentLateDataset(late_pred_path, gt_path, late_feat_path, listTrainFiles, listGtFiles,
                                            listTrainFeats, decode=decode)
            val_set = ResidentLateDataset(late_pred_path, gt_path, late_feat_path, listValFiles, listValGtFiles, listValFeats,
                                          decode=decode)
            fill_all((train_set, val_set), self.device, resident_gb, flag="--late_resident")
            self.stage = _stage_late_resident
        else:
            train_set = lateDataset(late_pred_path, gt_path, late_feat_path, listTrainFiles, listGtFiles, listTrainFeats)
            val_set = lateDataset(late_pred_path, gt_path, late_feat_path, listValFiles, listValGtFiles, listValFeats)
        return train_set, val_set

    def _run(self, loader, train, every):
        from .data.STdatas import staged_batches
        meters = EpochMeters(timed=False)

        def update(done):
            for loss1, aae1, auc1 in done:
                meters.update(loss1, 1, auc1, aae1)
        # the three maps of batch k + 1 cross PCIe on a copy stream while step k computes (LF.py:85-89 copies in the step)
        # The training step (forward + loss + zero_grad + backward + Adam, ~110 launches for ~1.4 ms of kernels) is captured
        # once and replayed (graphs.GraphedTrainStep); single process only -- the gradient reducer's hooks are host code.
        # An exception / KeyboardInterrupt inside the loop must not leave the optimizer capturable with a stale host step count
        # (ADVICE r3): leaving the block closes the step, which syncs the count back from the device
        use_graph = train and LF_GRAPH and dp.world_size() == 1 and self.device.type == 'cuda'
        with ReplayOrEager(use_graph, lambda maps: GraphedLateIteration(self.model, self.criterion, self.optimizer,
                                                                        maps)) as replay:
            for i, (sample, staged) in _progress(enumerate(staged_batches(loader, self.device, self.stage))):
                maps = _maps(staged)                              # (feat, im, gt), or (fused, gt) of a resident batch
                graphed = replay.pick(tuple(maps[0].shape), maps)
                if graphed is not None:
                    graphed(*maps)                                # one replay = one LF.trainLate iteration (LF.py:90-100)
                    if graphed.full or (i + 1) % every == 0:
                        update(graphed.drain())
                else:
                    if replay.step is not None:
                        update(replay.step.drain())               # (a trailing partial batch: the meters stay in iteration order)
                    out = _forward(self.model, maps)
                    loss = self.criterion(out, maps[-1])
                    aae1, auc1, _ = computeAAEAUC(out.detach(), maps[-1])     # device kernel, maps stay in HBM (LF.py:92-94)
                    meters.update(loss.item(), 1, auc1, aae1)
                    if train:
                        self.optimizer.zero_grad()
                        loss.backward()
                        self.optimizer.step()
                if (i + 1) % every == 0:
                    print('Epoch: [{0}][{1}/{2}]\t''AUCAAE_late {auc.avg:.3f} ({aae.avg:.3f})\t'
                          'Loss {loss.val:.4f} ({loss.avg:.4f})\t'.format(self.epochnow, i + 1, len(loader) + 1, auc=meters.auc,
                                                                          loss=meters.loss, aae=meters.aae))
            if replay.step is not None:
                update(replay.step.drain())
            if train:
                self.optimizer.check_finite()        # (NaN / inf gradient elements are skipped by the Adam kernel and reported here)
        return meters.averages()                     # global, so that every rank agrees on the best epoch

    def trainLate(self):
        # like the reference, the model is never switched to eval(): BN uses batch statistics in both loops
        return self._run(self.train_loader, True, 3000)

    def testLate(self):
        dp.sync_buffers(self.model)                  # train-mode BN here too (never eval()), but checkpoints are rank 0's
        with torch.no_grad():
            return self._run(self.val_loader, False, 1000)

    def train(self):
        print('begin training LF module...')
        trainprev, valprev, loss_train, loss_val = 999, 999, [], []
        for epoch in range(self.num_epoch):
            self.epochnow = epoch
            if self.train_sampler is not None:
                self.train_sampler.set_epoch(epoch)
            loss, auc, aae = self.trainLate()
            loss_train.append(loss)
            print('training, auc is %5f, aae is %5f' % (auc, aae))
            if loss < trainprev:
                if dp.is_main():                      # rank 0 owns the files (LF.py:144-153)
                    torch.save({'state_dict': owned_state_dict(self.model), 'loss': loss, 'auc': auc, 'aae': aae},
                               os.path.join(self.save_path, self.save_name))
                trainprev = loss
            loss, auc, aae = self.testLate()
            loss_val.append(loss)
            if dp.is_main():
                plot_loss(loss_train, loss_val, os.path.join(self.save_path, self.late_save_img))
            if loss < valprev:
                if dp.is_main():
                    torch.save({'state_dict': owned_state_dict(self.model), 'loss': loss, 'auc': auc, 'aae': aae},
                               os.path.join(self.save_path, 'val' + self.save_name))
                valprev = loss
            dp.barrier()
            print('testing, auc is %5f, aae is %5f' % (auc, aae))
        print('LF module training finished!')

    def val(self):
        print('begin testing LF module...')
        loss, auc, aae = self.testLate()
        print('AUC is : %04f, AAE is: %04f' % (auc, aae))
        print('LF module testing finished!')
