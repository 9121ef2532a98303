"""What the training drivers (SP, LF, AT, streamtrain, gaze_full, extractLSTMw) share, each piece once:
the progress wrapper, the rank-sharded and the batch-1 loaders, the ST file lists and datasets, the epoch's meters with their
reduction over the ranks, the validation loop of SP and the stream scripts, and the life cycle of a captured training step.
All of it is host code; the step bodies, their launches and the order of those stay in the drivers."""
import os
import time

import torch
from torch.utils.data import DataLoader

from . import dp
from .utils import AverageMeter, computeAAEAUC


def progress(it):
    try:
        from tqdm import tqdm
        return tqdm(it)
    except Exception:
        return it


def make_criterion(loss_function, device):
    from .floss import BCELoss, floss
    return (floss() if loss_function == 'f' else BCELoss()).to(device)


def init_distributed(args, timeout=None):
    """One process per GPU under torch.distributed.run (LOCAL_RANK / WORLD_SIZE set): ``args.device`` becomes the local rank
    and the default process group is created (``timeout``: a datetime.timedelta for its collectives)."""
    if 'LOCAL_RANK' in os.environ and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        args.device = os.environ['LOCAL_RANK']
        torch.cuda.set_device(int(args.device))
        torch.distributed.init_process_group(os.environ.get('EGAZE_DIST_BACKEND', 'nccl'),
                                             **({} if timeout is None else {'timeout': timeout}))


# ------------------------------------------------------------------------------------------------------------- loaders
def rank_loaders(train_set, val_set, batch_size, default_workers):
    """-> (train_loader, val_loader, train_sampler).  One process per GPU: every rank draws a disjoint 1/world share of each
    epoch (dp.RankShardSampler, train_sampler.set_epoch per epoch); at world 1 the sampler is None and these are exactly the
    reference's loaders (SP.py:34-35, LF.py:69-72, spatialstream.py:60-63).  ``default_workers``: the worker count of a dataset
    that declares no ``loader_workers`` (the resident sets declare 0: a pool must not be pickled into a worker)."""
    train_sampler = dp.RankShardSampler(train_set, True, batch_size) if dp.world_size() > 1 else None
    val_sampler = dp.RankShardSampler(val_set, False, batch_size, pad=False) if dp.world_size() > 1 else None
    train_loader = DataLoader(dataset=train_set, batch_size=batch_size, shuffle=train_sampler is None, sampler=train_sampler,
                              num_workers=getattr(train_set, 'loader_workers', default_workers), pin_memory=True,
                              collate_fn=getattr(train_set, 'collate_fn', None))
    val_loader = DataLoader(dataset=val_set, batch_size=batch_size, shuffle=False, sampler=val_sampler,
                            num_workers=getattr(val_set, 'loader_workers', default_workers), pin_memory=True,
                            collate_fn=getattr(val_set, 'collate_fn', None))
    return train_loader, val_loader, train_sampler


def extraction_loader(data, workers=None):
    """The batch-1, in-order loader of an extraction pass over an ST dataset.  ``workers=None``: the file form (the dataset's
    ``loader_workers``, else 1; pinned).  ``workers=0``: the in-memory hand-over form (nothing to pin: the batch is an index)."""
    return DataLoader(dataset=data, batch_size=1, shuffle=False,
                      num_workers=getattr(data, 'loader_workers', 1) if workers is None else workers,
                      pin_memory=workers is None, collate_fn=getattr(data, 'collate_fn', None))


def split_by(folder, val_name, task=None):
    """-> (training names, validation names) of ``folder``, sorted: leave-one-subject-out by ``val_name`` (gaze_full.py:61-71,
    LF.py:44-63), both restricted to the names holding ``task`` where one is given."""
    names = os.listdir(folder)
    train = sorted(k for k in names if val_name not in k)
    val = sorted(k for k in names if val_name in k)
    if task is not None:
        train = [k for k in train if task in k]
        val = [k for k in val if task in k]
    return train, val


def st_datasets(args, key=None, flow_from=None):
    """-> (train_data, val_data): the reference's file lists and STDatasets (gaze_full.py:60-76, spatialstream.py:34-59) from the
    parsed paths, bytes over PCIe and normalised on the GPU.  ``--gpu_decode`` / ``--gpu_resident`` choose the decoder and the
    resident form (filled here, within ``--gpu_resident_gb``); ``key``: only that input and the ground truth are read by
    decode='gpu'; ``flow_from`` (data.resident.FlowFrom): the flow planes are computed from its frames, ``--flowPath`` is not
    opened."""
    from .data.STdatas import STDataset
    listFolders = sorted(os.listdir(args.framePath if flow_from is not None else args.flowPath))
    listGtFiles, listValGtFiles = split_by(args.gtPath, args.val_name)
    print('num of training samples: ', len(listGtFiles))
    listfixsacTrain, listfixsacVal = split_by(args.fixsacPath, args.val_name)
    listTrainFiles, listValFiles = split_by(args.imagePath, args.val_name)
    print('num of val samples: ', len(listValFiles))
    decode = 'gpu' if getattr(args, 'gpu_decode', False) else 'host'
    resident = getattr(args, 'gpu_resident', False)
    if resident:                            # the planes live on the device; batches are gathered there (data/resident.py)
        from .data.resident import ResidentSTDataset as STDataset, fill_all
    train_data = STDataset(args.flowPath, args.imagePath, args.gtPath, listFolders, listTrainFiles, listGtFiles,
                           listfixsacTrain, args.fixsacPath, raw_u8=True, decode=decode)
    val_data = STDataset(args.flowPath, args.imagePath, args.gtPath, listFolders, listValFiles, listValGtFiles,
                         listfixsacVal, args.fixsacPath, raw_u8=True, decode=decode)
    if key is not None:
        train_data.gpu_fields = val_data.gpu_fields = (key, 'gt')
    if resident:
        fill_all((train_data, val_data), torch.device('cuda:' + str(args.device)), getattr(args, 'gpu_resident_gb', None),
                 flow_from=flow_from)
    return train_data, val_data


# -------------------------------------------------------------------------------------------------------------- meters
class EpochMeters:
    """The loss / AUC / AAE running averages of one epoch (any subset may be fed) and, with ``timed``, the time per iteration
    (``batch_time``, taken at every update).  Host arithmetic only: nothing here touches the device."""

    def __init__(self, timed=True):
        self.loss, self.auc, self.aae, self.batch_time = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
        self.end = time.time() if timed else None

    def update(self, loss=None, n=1, auc=None, aae=None):
        """``n`` weights the loss only (the batch size in SP and the stream loops, 1 in LF); AUC and AAE count per batch."""
        if loss is not None:
            self.loss.update(loss, n)
        if auc is not None:
            self.auc.update(auc)
        if aae is not None:
            self.aae.update(aae)
        if self.end is not None:
            now = time.time()
            self.batch_time.update(now - self.end)
            self.end = now

    def averages(self):
        """-> (loss, auc, aae), global under torch.distributed so that every rank takes the same 'best epoch' decision.  At
        world 1 dp.reduce_meters is sum / max(count, 1e-30): AverageMeter.avg bit for bit, 0 for a meter never fed."""
        return tuple(dp.reduce_meters(*((m.sum, m.count) for m in (self.loss, self.auc, self.aae))))


def validation_epoch(batches, forward, criterion, print_when, total, squeeze=False):
    """The validation loop of SP.testSP (SP.py:150-186) and streamtrain.evaluate (spatialstream.py:154-184) -> (loss, auc, aae).
    ``batches``: the enumerate()d staged_batches of the loader (the caller wraps it in its progress bar, switches the model to
    eval() and syncs its buffers first); ``forward(staged) -> (output, target)``; ``print_when(i)``: the reference's print
    predicate; ``total``: len(loader), printed; ``squeeze``: the stream scripts hand computeAAEAUC squeezed maps."""
    meters = EpochMeters()
    with torch.no_grad():
        for i, (sample, staged) in batches:
            output, target = forward(staged)
            target = target.view(output.size())
            loss = criterion(output, target).item()
            aae1, auc1, _ = computeAAEAUC(output.squeeze(), target.squeeze()) if squeeze else computeAAEAUC(output, target)
            meters.update(loss, output.size(0), auc1, aae1)
            if print_when(i):
                print('Test: [{0}/{1}]\t''Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                      'Loss {loss.val:.4f} ({loss.avg:.4f})\t'.format(i, total, batch_time=meters.batch_time, loss=meters.loss))
    loss_avg, auc_avg, aae_avg = meters.averages()
    if dp.is_main():
        print('AUC: {0}\t AAE: {1}'.format(auc_avg, aae_avg))
    return loss_avg, auc_avg, aae_avg


# ------------------------------------------------------------------------------------------------------ captured steps
class ReplayOrEager:
    """The life cycle of a captured training step inside an epoch loop::

        with ReplayOrEager(wanted, lambda example: GraphedXStep(..., example)) as replay:
            for batch in loader:
                step = replay.pick(tuple(batch[0].shape), batch)
                if step is not None: step(*batch)        # replay
                else: ...                                # the loop's own eager body

    The step is built from the first batch when ``wanted`` and replayed while the shape is the one it captured; any other
    batch (the trailing partial one) is the loop's to run eagerly.  Leaving the block -- normally, by an exception or by a
    KeyboardInterrupt -- closes the step: the optimizer leaves capturable mode and its host step count follows the device's."""

    def __init__(self, wanted, build):
        self.wanted, self.build, self.step = wanted, build, None

    def __enter__(self):
        return self

    def pick(self, shape, example):
        if self.step is None:
            if not self.wanted:
                return None
            self.step = self.build(example)
        return self.step if shape == self.step.shape else None

    def __exit__(self, *exc):
        step, self.step, self.wanted = self.step, None, False
        if step is not None:
            step.close()
        return False
