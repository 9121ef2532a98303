"""Mirror of the reference's ``gaze_full.py`` CLI (gaze_full.py:10-118): the same 37 flags with the same defaults,
then SP -> AT -> (extraction) -> LF.  Run as ``python -m egaze_amd.gaze_full --train_sp --train_lstm --train_late ...``
(one process per GPU; under ``torch.distributed.run`` the SP / LF optimizers all-reduce their gradients over RCCL).
"""
import argparse
import os

import torch

from .trainloop import extraction_loader, init_distributed, st_datasets
from .trainloop import split_by as _split  # noqa: F401  (the tools and the tests list the folders with it)


# The three in-memory hand-overs: (flag, [(flag it needs, why)], why it runs in one process, the flag it implies).  The parser
# refuses each where a need is missing or WORLD_SIZE is above 1, in this order.
_POOL = "the frames and the ground truth are taken from the resident pool on the device"
_HANDOVERS = (
    ('lstm_handover', (('gpu_resident', _POOL),
                       ('extract_lstm', "the LSTM vectors exist only in the memory of the run that extracts them"),
                       ('train_lstm', "the vectors are not written anywhere, only this run's LSTM training can use them")),
     "a sharded extraction leaves every rank with its own vectors only", 'lstm_resident'),
    ('late_handover', (('gpu_resident', _POOL),
                       ('extract_late', "the late-fusion planes exist only in the memory of the run that extracts them"),
                       ('train_late', "the planes are not written anywhere, only this run's LF training can use them")),
     "a sharded extraction leaves every rank with its own chunks only", 'late_resident'),
    ('flow_handover', (('gpu_resident', "the flow images are written into the resident pool on the device"),
                       ('framePath', "the flow images are computed from the frames (one folder per video, img_%05d.jpg)")),
     "every rank would compute every flow", None),
)


def build_parser():
    from .streamtrain import _CheckedParser, add_augment_flags

    class _Parser(_CheckedParser):
        """Also refuses ``--late_handover``, ``--lstm_handover`` and ``--flow_handover`` where they cannot work, as any other
        bad command line."""

        def parse_known_args(self, args=None, namespace=None):
            ns, rest = super().parse_known_args(args, namespace)
            if getattr(ns, 'lstm_handover_chunk', None) is not None and not getattr(ns, 'lstm_handover', False):
                self.error("--lstm_handover_chunk needs --lstm_handover")
            world = os.environ.get('WORLD_SIZE', '1')
            for flag, needs, alone, implies in _HANDOVERS:
                if not getattr(ns, flag, False):
                    continue
                for need, why in needs:
                    if getattr(ns, need, None) in (None, False):
                        self.error(f"--{flag} needs --{need}: {why}")
                # (the two checks of --lstm_handover's own extras sit inside the loop only to keep the order of its refusals)
                if flag == 'lstm_handover' and ns.align:
                    self.error("--lstm_handover does not take --align: the aligned window is built on the host from the "
                               "full-resolution ground truth")
                if int(world) > 1:
                    self.error(f"--{flag} runs in one process: {alone} (WORLD_SIZE is {world})")
                if flag == 'lstm_handover' and getattr(ns, 'lstm_handover_chunk', 1) < 1:
                    self.error("--lstm_handover_chunk must be at least 1")
                if implies is not None:
                    setattr(ns, implies, True)
            for flag in ('framePath', 'flow_quality', 'flow_bound'):
                if getattr(ns, flag, None) is not None and not getattr(ns, 'flow_handover', False):
                    self.error(f"--{flag} needs --flow_handover")
            if getattr(ns, 'flow_handover', False):
                if not 0 <= getattr(ns, 'flow_quality', 95) <= 100:
                    self.error("--flow_quality must be 0 .. 100 (0: no JPEG round trip)")
                if not getattr(ns, 'flow_bound', 20.0) > 0:
                    self.error("--flow_bound must be positive")
            return ns, rest

    p = _Parser()
    a = p.add_argument
    a('--lr_late', type=float, default=1e-4, required=False, help='lr for LF Adam')
    a('--lr', type=float, default=1e-7, required=False, help='lr for SP Adam')
    a('--sp_resume', default='0', required=False, help='2 from fusion, 0 from vgg, 1 from separately trained models.')
    a('--sp_save_img', default='loss_SP.png', required=False)
    a('--late_save_img', default='loss_late.png', required=False)
    a('--pretrained_spatial', default='save/04_spatial.pth.tar', required=False)
    a('--pretrained_temporal', default='save/03_temporal.pth.tar', required=False)
    a('--pretrained_model', default=None, required=False, help='pretrained SP module')
    a('--pretrained_lstm', default=None, required=False, help='pretrained LSTM in AT module')
    a('--pretrained_late', default=None, required=False, help='pretrained LF module')
    a('--lstm_save_img', default='loss_lstm.png', required=False)
    a('--save_sp', default='best_SP.pth.tar', required=False)
    a('--save_lstm', default='best_lstm.pth.tar', required=False)
    a('--save_late', default='best_late.pth.tar', required=False)
    a('--save_path', default='save', required=False)
    a('--loss_function', default='f', required=False, help='if is not set as f, use bce loss')
    a('--num_epoch', type=int, default=10, required=False)
    a('--num_epoch_lstm', type=int, default=120, required=False)
    a('--extract_lstm', action='store_true')
    a('--extract_lstm_path', default='../512w', required=False)
    a('--train_sp', action='store_true')
    a('--train_lstm', action='store_true')
    a('--train_late', action='store_true')
    a('--extract_late', action='store_true')
    a('--extract_late_pred_folder', default='../new_pred/', required=False)
    a('--extract_late_feat_folder', default='../new_feat/', required=False)
    a('--device', default='0', help='GPU index of this process (one process per GPU)')
    a('--val_name', default='Alireza', required=False, help='cross subject validation')
    a('--task', default=None, required=False, help='cross task validation')
    a('--flowPath', default='../gtea_imgflow', required=False)
    a('--imagePath', default='../gtea_images', required=False)
    a('--fixsacPath', default='fixsac', required=False)
    a('--gtPath', default='../gtea_gts', required=False)
    a('--batch_size', type=int, default=64, help='batch size of LF')
    a('--batch_size_sp', type=int, default=8, help='batch size of SP')
    a('--crop_size', type=int, default=3, help='crop size of vgg conv5_3 feature')
    a('--align', action='store_true')
    # not a reference flag: absent from the namespace unless given, so the parsed defaults stay the reference's 37
    a('--gpu_decode', action='store_true', default=argparse.SUPPRESS,
      help="decode the dataset's JPEGs on the GPU (STDataset(decode='gpu')); default: host decode as the reference")
    a('--gpu_resident', action='store_true', default=argparse.SUPPRESS,
      help="decode every file once and keep the planes in device memory (data.resident); batches are gathered on the GPU. "
           "With --gpu_decode the one-time fill decodes on the GPU")
    a('--gpu_resident_gb', type=float, default=argparse.SUPPRESS,
      help='device memory the resident dataset may take, in GB, shared by the training and validation sets '
           '(default: 0.8 x what is free)')
    a('--late_resident', action='store_true', default=argparse.SUPPRESS,
      help="LF stage: decode the extracted SP / AT maps and the ground truth once and keep the planes in device memory "
           "(data.late_resident); batches are gathered on the GPU.  Honours --gpu_decode and --gpu_resident_gb")
    a('--lstm_resident', action='store_true', default=argparse.SUPPRESS,
      help="AT stage: read the extracted LSTM vectors once and keep them in device memory (data.lstm_resident); every step of "
           "the LSTM training and validation fetches its input and target on the GPU.  Honours --gpu_resident_gb")
    a('--late_handover', action='store_true', default=argparse.SUPPRESS,
      help="with --gpu_resident --extract_late --train_late: the extraction writes the SP / AT planes and the ground truth "
           "straight into the late-fusion pools on the device (no pred / feat file is written or read) and LF trains from "
           "them.  Implies --late_resident; one process only.  Honours --gpu_resident_gb")
    a('--lstm_handover', action='store_true', default=argparse.SUPPRESS,
      help="with --gpu_resident --extract_lstm --train_lstm: the extraction writes the LSTM vectors straight into the vector "
           "pools on the device (no fix_*.pth.tar file is written or read, --extract_lstm_path is not touched) and the LSTM "
           "trains from them.  Implies --lstm_resident; one process only; not with --align.  Honours --gpu_resident_gb")
    a('--lstm_handover_chunk', type=int, default=argparse.SUPPRESS,
      help="frames per encoder forward of the --lstm_handover extraction (default 1: the file path's schedule, bit for bit; "
           "a larger chunk is faster and is another batched forward, not bit-identical with the files)")
    a('--flow_handover', action='store_true', default=argparse.SUPPRESS,
      help="with --gpu_resident --framePath P: the TV-L1 flow images are computed from the frames and written straight into "
           "the flow planes of the resident pool (data.extract_flow.flows_into); no flow file is written or read and "
           "--flowPath is not opened.  The planes are those extract_flow's files decode to.  One process only")
    a('--framePath', default=argparse.SUPPRESS,
      help="--flow_handover: folder of per-video folders holding img_%%05d.jpg frames (extract_flow's --framePath)")
    a('--flow_quality', type=int, default=argparse.SUPPRESS,
      help="--flow_handover: JPEG quality the flow images go through (default 95, extract_flow's; 0: none)")
    a('--flow_bound', type=float, default=argparse.SUPPRESS,
      help="--flow_handover: flow of +-bound pixels maps to 255 / 0 (default 20, extract_flow's)")
    add_augment_flags(p)                  # the SP stage's training loop only: validation, AT and LF never see an augmented batch
    return p


def _at_kwargs(args, STTrainData, STValData):
    """AT's arguments from the command line, but for ``shard``, ``resident`` and the hand-over pair, which the two stages set."""
    return dict(pretrained_model=args.pretrained_model, pretrained_lstm=args.pretrained_lstm,
                extract_lstm=args.extract_lstm, crop_size=args.crop_size, num_epoch_lstm=args.num_epoch_lstm,
                lstm_save_img=args.lstm_save_img, save_path=args.save_path, save_name=args.save_lstm,
                device=args.device, lstm_data_path=args.extract_lstm_path, traindata=STTrainData, valdata=STValData,
                task=args.task, align=args.align, resident_gb=getattr(args, 'gpu_resident_gb', None))


def _at_stage(args, STTrainData, STValData):
    from .AT import AT
    att = AT(resident=getattr(args, 'lstm_resident', False) and args.train_lstm,
             lstm_handover=getattr(args, 'lstm_handover', False), lstm_handover_chunk=getattr(args, 'lstm_handover_chunk', 1),
             **_at_kwargs(args, STTrainData, STValData))
    if args.train_lstm:
        att.train()
    if args.extract_late and getattr(args, 'late_handover', False):
        # both late pools are planned and allocated, under what the ST pools left of --gpu_resident_gb, before the extraction
        # starts: a pool that does not fit refuses here, not after the first pass
        from .data.late_resident import ResidentLateDataset
        late = [ResidentLateDataset.from_st(data, task=args.task) for data in (STTrainData, STValData)]
        from .data.resident import resident_budget, under_budget
        under_budget(late, resident_budget(att.device, getattr(args, 'gpu_resident_gb', None),
                                           sum(d.needed_bytes for d in (STTrainData, STValData))),
                     lambda needed, budget: f"--late_handover: the late-fusion planes need {needed} bytes, {budget} bytes are "
                                            f"left of the budget beside the resident dataset: run without --late_handover "
                                            f"(there is no partial cache)",
                     lambda d, left: d.allocate(att.device, left))
        if not args.train_lstm:
            att.reload_LSTM(os.path.join(args.save_path, args.save_lstm))
        for data, into in ((STValData, late[1]), (STTrainData, late[0])):
            att.extract_late(extraction_loader(data, workers=0), into=into)
        return tuple(late)
    if args.extract_late:
        if not args.train_lstm:
            att.reload_LSTM(os.path.join(args.save_path, args.save_lstm))
        for data in (STValData, STTrainData):
            att.extract_late(extraction_loader(data), args.extract_late_pred_folder, args.extract_late_feat_folder)


def _at_stage_sharded(args, STTrainData, STValData):
    """The AT stage under torch.distributed.  The two extraction passes are per-frame work and run on every rank
    (extractLSTMw.extractw and AT.extract_late with ``shard=``); ``AT.train`` is a per-sample optimiser chain whose state and
    weights are carried from sample to sample across the whole dataset, so it stays on rank 0 while the others wait on
    the host (_wait_for_rank0)."""
    from . import dp
    from .AT import AT
    shard = (dp.rank(), dp.world_size())
    att = AT(shard=shard, resident=getattr(args, 'lstm_resident', False) and args.train_lstm and dp.is_main(),   # where AT.train runs
             **_at_kwargs(args, STTrainData, STValData))
    if args.train_lstm:
        if dp.is_main():
            try:
                att.train()
            except BaseException:         # let the waiting ranks go down with this one instead of polling for ever
                torch.distributed.distributed_c10d._get_default_store().set("at_lstm_trained/failed", "1")
                raise
        _wait_for_rank0("at_lstm_trained")
    if args.extract_late:
        # every rank runs the whole recurrence of extract_late: all of them take the weights from the one saved file
        att.reload_LSTM(os.path.join(args.save_path, args.save_lstm))
        for data in (STValData, STTrainData):
            att.extract_late(extraction_loader(data), args.extract_late_pred_folder, args.extract_late_feat_folder, shard=shard)
    dp.barrier()                          # LF lists the folders: not before every rank has written its files


def _wait_for_rank0(key, poll_s=5.0):
    """Host-side rendezvous after a rank-0-only stage: rank 0 sets ``key`` in the default process group's store when it is
    done (or ``key + '/failed'`` on its way out of an exception), the others poll with sleep.  No device collective runs
    while waiting, and a failure of rank 0 ends the other ranks instead of leaving them in a barrier."""
    import time
    from . import dp
    if dp.world_size() == 1:
        return
    store = torch.distributed.distributed_c10d._get_default_store()
    if dp.is_main():
        store.set(key, "1")
        return
    while True:
        if store.check([key + "/failed"]):
            raise RuntimeError("rank 0 failed in its sequential stage (%s)" % key)
        if store.check([key]):
            return
        time.sleep(poll_s)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .AT import AT
    from .LF import LF
    from .SP import SP
    from .streamtrain import augment_spec
    from . import dp
    import datetime
    # the LSTM training of the AT stage is sequential (rank 0 only) and takes hours: the other ranks wait for it on the HOST
    # (_wait_for_rank0: a key in the process group's store, polled with sleep) -- not inside a device collective, which
    # would spin for hours and need a multi-day collective timeout that also hides real hangs of the SP / LF all-reduces
    init_distributed(args, timeout=datetime.timedelta(minutes=30))
    flow_from = None
    if getattr(args, 'flow_handover', False):   # the flow paths are keys into the pool; --flowPath is never opened
        from .data.resident import FlowFrom
        flow_from = FlowFrom(args.framePath, bound=getattr(args, 'flow_bound', 20.0),
                             quality=getattr(args, 'flow_quality', 95))
    STTrainData, STValData = st_datasets(args, flow_from=flow_from)
    os.makedirs(args.save_path, exist_ok=True)
    if args.train_sp:
        sp = SP(lr=args.lr, loss_save=args.sp_save_img, save_name=args.save_sp, save_path=args.save_path,
                loss_function=args.loss_function, num_epoch=args.num_epoch, batch_size=args.batch_size_sp,
                device=args.device, resume=args.sp_resume, pretrained_spatial=args.pretrained_spatial,
                pretrained_temporal=args.pretrained_temporal, traindata=STTrainData, valdata=STValData,
                augment=augment_spec(args))
        sp.train()
        args.pretrained_model = os.path.join(args.save_path, args.save_sp)
    # Under torch.distributed the AT stage's two extraction passes are sharded over the ranks, chunk by chunk, without changing
    # a byte of what they write; only the LSTM training -- a batch-1, sequence-1 optimiser chain carried from sample to sample
    # across the whole dataset (AT.py:127-145) -- runs on rank 0 alone (_at_stage_sharded).  One rank: the calls as ever.
    late_sets = None
    if dp.world_size() == 1:
        late_sets = _at_stage(args, STTrainData, STValData)
    else:
        _at_stage_sharded(args, STTrainData, STValData)
    _lf_stage(args, (STTrainData, STValData), late_sets)


def _lf_stage(args, st_data=(), late_sets=None):
    """The LF stage.  ``--late_resident``: its two datasets are decoded once into device memory (data/late_resident.py), on the
    GPU with ``--gpu_decode``, within ``--gpu_resident_gb``; the pools of ``--gpu_resident`` (``st_data``) are released first.
    ``late_sets``: the (training, validation) sets ``--late_handover``'s extraction has written, handed to LF as they are."""
    from .LF import LF
    late_resident = getattr(args, 'late_resident', False)
    decode = 'gpu' if getattr(args, 'gpu_decode', False) else 'host'
    if late_resident:                       # nothing after the AT stage reads the ST pools: their memory goes to the LF pools
        for data in st_data:
            if getattr(data, 'pool', None) is not None:
                data.pool = data.table = None
        torch.cuda.empty_cache()
    lf = LF(pretrained_model=args.pretrained_late, save_path=args.save_path, late_save_img=args.late_save_img,
            save_name=args.save_late, device=args.device, late_pred_path=args.extract_late_pred_folder,
            num_epoch=args.num_epoch, late_feat_path=args.extract_late_feat_folder, gt_path=args.gtPath,
            val_name=args.val_name, batch_size=args.batch_size, loss_function=args.loss_function, lr=args.lr_late,
            task=args.task, resident=late_resident, decode=decode, resident_gb=getattr(args, 'gpu_resident_gb', None),
            datasets=late_sets)
    if args.train_late:
        lf.train()
    else:
        lf.val()


if __name__ == '__main__':
    main()
