"""Shared implementation of the reference's stream pre-training scripts ``spatialstream.py`` / ``temporalstream.py``: the
first step of its recipe ("first train the spatial and temporal stream separately, and then train the full SP module").

The two scripts differ only in the input (the RGB frame / the 20-channel flow stack), the freezing of the encoder, the file
names and one print condition (``STREAMS`` below); everything else is here:

  ``StreamVGG``   the reference's ``VGG`` (spatialstream.py:65-116): VGG16-BN encoder + the 14-conv decoder of
                  run_spatialstream.py (three 512->512 convs before the first upsample) + Sigmoid, forward -> the map only.
  ``train_epoch`` the reference's ``train`` (:121-151).  Both scripts optimise ``model.decoder.parameters()`` only (:216), so the
                  encoder's train-mode forward (batch statistics, running-statistic updates) runs under ``torch.no_grad()``
                  and only the decoder builds an autograd graph.  ``--hipgraph`` replays the whole step as one hipGraph.
  ``validate``    the reference's ``validate`` (:154-184): eval mode, loss + computeAAEAUC per batch, returns the mean loss.
  ``main``        flags, model building for ``--resume 0 / 1``, Adam, the epoch loop and best-val checkpoints (:189-236).

Nothing runs at import: the reference parses argv, lists the data folders and downloads VGG16-BN there.
"""
import argparse
import functools
import os

import torch
import torch.nn as nn

from . import dp
from .trainloop import (EpochMeters, ReplayOrEager, init_distributed, make_criterion, progress as _progress, rank_loaders,
                        st_datasets, validation_epoch)
from .utils import (FusedSequential, cfg, change_key_names, init_like_reference, load_merged, make_layers, owned_state_dict,
                    plot_loss, save_checkpoint)

# run_spatialstream.py:17-53 / spatialstream.py:72-91 as (Cin, Cout) 3x3+ReLU blocks and 'U' = nearest x2 upsample; a 1x1 head
# follows
DECODER_PLAN = [(512, 512), (512, 512), (512, 512), 'U', (512, 512), (512, 512), (512, 512), 'U', (512, 256),
                (256, 256), (256, 256), 'U', (256, 128), (128, 128), 'U', (128, 64), (64, 64)]

# what the two reference scripts do differently (diff spatialstream.py temporalstream.py)
STREAMS = {
    'spatial': dict(in_channels=3, key='image', freeze=True, arch='rgb', loss_save='loss_spatial.png',
                    save_name='_spatial.pth.tar', val_print=lambda i: (i + 1) % 1000 == 0),
    'temporal': dict(in_channels=20, key='flow', freeze=False, arch='flow', loss_save='loss_temporal.png',
                     save_name='best_temporal.pth.tar', val_print=lambda i: i % 1000 == 0),
}


class StreamVGG(nn.Module):
    """The reference's ``VGG`` of both stream scripts.  State-dict keys: ``features.*`` + ``decoder.{0,2,...,30}.*`` -- the
    layout of run_spatialstream.VGG, so each loads the other's checkpoints strictly.  ``freeze_features``: the spatial script
    sets ``requires_grad = False`` on the encoder (spatialstream.py:70-71), the temporal one does not."""

    def __init__(self, features, freeze_features=True):
        super(StreamVGG, self).__init__()
        self.features = features
        if freeze_features:
            for param in self.features.parameters():
                param.requires_grad = False
        layers = []
        for item in DECODER_PLAN:
            if item == 'U':
                layers.append(nn.Upsample(scale_factor=2))
            else:
                layers += [nn.Conv2d(item[0], item[1], kernel_size=3, padding=1), nn.ReLU(inplace=True)]
        layers.append(nn.Conv2d(64, 1, kernel_size=1, padding=0))
        self.decoder = FusedSequential(*layers)              # 31 children, indices as the reference's
        self.final = nn.Sigmoid()
        init_like_reference(self)

    def forward(self, x):
        """Full autograd semantics (an unfrozen, optimised encoder gets its gradients); the decoder's head runs fused with
        ``final`` (functions.HeadSigmoid)."""
        return self.decoder(self.features(x), fuse_sigmoid=True)


def _optimised(model, optimizer):
    """True when the optimizer holds a parameter of the encoder (not the reference's setup: it optimises the decoder only)."""
    ids = {id(p) for p in (optimizer.params if hasattr(optimizer, 'params')
                           else [q for g in optimizer.param_groups for q in g['params']])}
    return any(id(p) in ids for p in model.features.parameters())


def step_forward(model, x, encoder_grad=False):
    """The training step's forward: the encoder's train-mode pass (batch statistics, running statistics updated) without an
    autograd graph -- the reference back-propagates into it and then never applies the result -- and the decoder with one.
    ``decoder.0`` therefore takes no data gradient (functions.ConvReLU skips it: ``needs_input_grad``)."""
    if encoder_grad:
        return model(x)
    with torch.no_grad():
        feat = model.features(x)
    return model.decoder(feat, fuse_sigmoid=True)


def stage_stream(sample, device, key, prepare=True):
    """``staged_batches`` stage of a stream script: only the stream's input (``'image'`` or ``'flow'``) and the ground truth
    cross PCIe; bytes of a ``raw_u8`` dataset are normalised on the device (hipops.u8_normalize).  ``prepare``: the flow stack's
    NHWC-32 re-layout is issued behind the copy (hipops.prepare_network_input), as data.STdatas.stage_batch does for SP."""
    from . import hipops as H
    from .data.STdatas import FLOW_MEAN, FLOW_STD, IMAGE_MEAN, IMAGE_STD
    if 'resident' in sample:                   # data.resident: gathered from the pool on the device, NHWC-32 form included
        got = sample['resident'].gather(sample, device, fields=(key, 'gt'), prepare=prepare)
        return got[0 if key == 'image' else 1], got[2]
    if 'jpeg_blob' in sample:                  # decode='gpu': decoded on the device into the raw_u8 layout
        from .data.STdatas import decode_to_u8
        image, flow, gt = decode_to_u8(sample, device)
        sample = {'image': image, 'flow': flow, 'gt': gt}
    x, gt = sample[key], sample['gt']
    if device.type != 'cuda':
        return x.float().to(device), gt.float().to(device)
    if x.dtype == torch.uint8:
        mean, std = (IMAGE_MEAN, IMAGE_STD) if key == 'image' else (FLOW_MEAN, FLOW_STD)
        x = H.u8_normalize(x.contiguous().to(device, non_blocking=True), mean, std)
        gt = H.u8_normalize(gt.contiguous().to(device, non_blocking=True), (0.0,), (1.0,))
    else:
        x = x.float().to(device, non_blocking=True)
        gt = gt.float().to(device, non_blocking=True)
    if prepare and key == 'flow':
        H.prepare_network_input(x)
    return x, gt


class GraphedStreamStep:
    """One training iteration of a stream script -- the encoder's train-mode forward with its running-statistic updates, the
    decoder's forward and backward, the loss and FusedAdam (device step counter) -- as one hipGraph replay
    (graphs.GraphedTrainStep).  The frozen encoder's packed weights are baked into the graph: they are passed as
    ``extra_params``, so a ``load_state_dict`` into the encoder between two replays is repacked before the next one."""

    def __init__(self, model, criterion, optimizer, example, encoder_grad=False):
        from .graphs import GraphedTrainStep

        def fwd_loss(x_, gt_):
            o = step_forward(model, x_, encoder_grad)
            return criterion(o, gt_.view(o.size())), o
        self.step = GraphedTrainStep(fwd_loss, optimizer, example, extra_params=list(model.features.parameters()))
        self.shape = tuple(example[0].shape)

    def __call__(self, x, gt):
        return self.step(x, gt)

    def close(self):
        self.step.close()


def train_epoch(train_loader, model, criterion, optimizer, epoch, device, stream='spatial', hipgraph=False, every=5000,
                augment=None):
    """spatialstream.py:121-151.  Returns the epoch's mean loss (averaged over the ranks under torch.distributed).
    ``hipgraph``: full batches run as one captured step (GraphedStreamStep), a trailing partial batch eagerly; single process
    only (the gradient all-reduce hooks are host code).  ``augment``: a hipops.AugSpec; the batches of a resident dataset are
    augmented in the gather under (its seed, ``epoch``, sample number).  The gather runs on the staging stream outside the
    captured step, so seed and epoch passed by value never end up inside a graph."""
    spec = STREAMS[stream]
    device = torch.device(device)
    meters = EpochMeters()
    model.train()
    optimizer.zero_grad()
    encoder_grad = _optimised(model, optimizer)
    use_graph = hipgraph and dp.world_size() == 1 and device.type == 'cuda'
    stage = functools.partial(stage_stream, key=spec['key'], prepare=not use_graph)
    from .data.STdatas import augmenting, staged_batches
    # both are left on every way out; leaving the replay closes the captured step: the optimizer leaves capturable mode, its
    # host step count follows the device counter
    with augmenting(getattr(train_loader, 'dataset', None), augment, epoch), \
            ReplayOrEager(use_graph, lambda example: GraphedStreamStep(model, criterion, optimizer, example,
                                                                       encoder_grad)) as replay:
        for i, (sample, (inp, target)) in _progress(enumerate(staged_batches(train_loader, device, stage))):
            graphed = replay.pick(tuple(inp.shape), (inp, target))
            if graphed is not None:
                loss, output = graphed(inp, target)
            else:
                if replay.step is not None:
                    optimizer.zero_grad()      # (a replay leaves its gradient in the buffers: the captured step zeroes first)
                output = step_forward(model, inp, encoder_grad)
                target = target.view(output.size())
                loss = criterion(output, target)
                loss.backward()
                optimizer.step()
                optimizer.zero_grad()
            meters.update(loss.item(), inp.size(0))
            if (i + 1) % every == 0:
                print('Epoch: [{0}][{1}/{2}]\t''Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                      'Loss {loss.val:.4f} ({loss.avg:.4f})\t'.format(epoch, i + 1, len(train_loader) + 1,
                                                                      batch_time=meters.batch_time, loss=meters.loss))
    if hasattr(optimizer, 'check_finite'):
        optimizer.check_finite()        # raises if a step of the epoch met NaN / inf gradients (the kernel skipped those elements)
    return meters.averages()[0]


def validate(val_loader, model, criterion, epoch, device, stream='spatial'):
    """spatialstream.py:154-184: returns the mean loss (``evaluate`` has the AUC / AAE averages too)."""
    return evaluate(val_loader, model, criterion, epoch, device, stream)[0]


def evaluate(val_loader, model, criterion, epoch, device, stream='spatial'):
    """The body of the reference's ``validate``: eval mode, no_grad, loss and computeAAEAUC(output.squeeze(), target.squeeze())
    per batch (the per-sample branch for a 3-D batch, the 2-D one for a batch of 1), prints AUC / AAE.  Returns (loss, auc,
    aae) averages.  Under torch.distributed every rank first takes rank 0's BatchNorm running statistics (the encoder's differ
    per rank after training) and the averages are global."""
    spec = STREAMS[stream]
    device = torch.device(device)
    dp.sync_buffers(model)
    model.eval()
    from .data.STdatas import staged_batches
    batches = _progress(enumerate(staged_batches(val_loader, device, functools.partial(stage_stream, key=spec['key']))))
    return validation_epoch(batches, lambda staged: (model(staged[0]), staged[1]), criterion, spec['val_print'],
                            len(val_loader), squeeze=True)


def build_parser(stream):
    """The reference's flags and defaults (spatialstream.py:15-30 / temporalstream.py:14-29), plus ``--hipgraph``."""
    spec = STREAMS[stream]
    p = _CheckedParser()
    p.add_argument('--lr', type=float, default=1e-7, required=False)
    p.add_argument('--loss_save', default=spec['loss_save'], required=False)
    p.add_argument('--save_name', default=spec['save_name'], required=False)
    p.add_argument('--save_path', default='save', required=False)
    p.add_argument('--loss_function', default='f', required=False)
    p.add_argument('--num_epoch', type=int, default=10, required=False)
    p.add_argument('--device', default='0')
    p.add_argument('--resume', type=int, default=0, help='0 from vgg, 1 from pretrained model.')
    p.add_argument('--pretrained_model', default='save/best_spatial.pth.tar', help='path to pretrained model')
    p.add_argument('--batch_size', type=int, default=16, required=False)
    p.add_argument('--flowPath', default='../gtea_imgflow', required=False)
    p.add_argument('--imagePath', default='../gtea_images', required=False)
    p.add_argument('--fixsacPath', default='../fixsac', required=False)
    p.add_argument('--gtPath', default='../gtea_gts', required=False)
    p.add_argument('--val_name', default='Alireza', required=False)
    p.add_argument('--hipgraph', action='store_true',
                   help='replay every full training batch as one captured hipGraph (default: eager)')
    # absent from the namespace unless given: the parsed defaults stay the reference's
    p.add_argument('--gpu_decode', action='store_true', default=argparse.SUPPRESS,
                   help="decode the dataset's JPEGs on the GPU (STDataset(decode='gpu')); default: host decode as the reference")
    p.add_argument('--gpu_resident', action='store_true', default=argparse.SUPPRESS,
                   help="decode every file once and keep the planes in device memory (data.resident); batches are gathered on "
                        "the GPU.  With --gpu_decode the one-time fill decodes on the GPU")
    p.add_argument('--gpu_resident_gb', type=float, default=argparse.SUPPRESS,
                   help='device memory the resident dataset may take, in GB, shared by the training and validation sets '
                        '(default: 0.8 x what is free)')
    add_augment_flags(p)
    return p


class _CheckedParser(argparse.ArgumentParser):
    """An ArgumentParser that refuses ``--augment`` / ``--augment_seed`` without ``--gpu_resident``, and a spec that does not
    parse, as it refuses any other bad command line."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if (hasattr(ns, 'augment') or hasattr(ns, 'augment_seed')) and not getattr(ns, 'gpu_resident', False):
            self.error("--augment / --augment_seed need --gpu_resident: augmentation happens in the gather over the resident "
                       "pool, the host loading path has none")
        if hasattr(ns, 'augment_seed') and not hasattr(ns, 'augment'):
            self.error("--augment_seed without --augment")
        if hasattr(ns, 'augment'):
            try:
                augment_spec(ns)
            except ValueError as e:
                self.error(f"--augment: {e}")
        return ns, rest


def add_augment_flags(parser):
    """``--augment SPEC`` / ``--augment_seed N`` (absent from the namespace unless given); ``parser`` is a _CheckedParser."""
    parser.add_argument('--augment', metavar='SPEC', default=argparse.SUPPRESS,
                        help="augment the training batches in the resident gather: 'flip=0.5,shift=16,contrast=0.2,"
                             "brightness=0.1,scale=0.15,rotate=10' (any subset; a bare 'flip' means 0.5; scale is the "
                             "amplitude of a magnification 1 +- scale, at most 0.5, rotate that of a rotation in degrees, at "
                             "most 45).  Needs --gpu_resident")
    parser.add_argument('--augment_seed', type=int, metavar='N', default=argparse.SUPPRESS,
                        help='seed of the augmentation draw (default 0); the draw depends on (seed, epoch, sample number) only')


def augment_spec(args):
    """The hipops.AugSpec of a parsed command line, None without ``--augment``."""
    if not hasattr(args, 'augment'):
        return None
    from .hipops import AugSpec
    return AugSpec.parse(args.augment, seed=getattr(args, 'augment_seed', None))


def build_model(stream, resume=0, pretrained_model=None):
    """spatialstream.py:189-210: resume 1 merges the whole state dict of ``--pretrained_model`` (no optimizer state, the epoch
    counter restarts), resume 0 takes the encoder from ImageNet VGG16-BN (the temporal stream through change_key_names(., 20))."""
    from .SP import _load_vgg16_bn
    spec = STREAMS[stream]
    model = StreamVGG(make_layers(cfg['D'], spec['in_channels']), freeze_features=spec['freeze'])
    if resume == 1:
        print('building model and loading from pretrained model...')
        load_merged(model, torch.load(pretrained_model, map_location='cpu', weights_only=False)['state_dict'])
    else:
        print('building model and loading pretrained_dict from vgg...')
        pretrained_dict = _load_vgg16_bn()
        if spec['in_channels'] != 3:
            pretrained_dict = change_key_names(pretrained_dict, spec['in_channels'])
        load_merged(model, pretrained_dict, known_only=True)
    return model


def make_loaders(args, key=None):
    """The reference's file lists and loaders (spatialstream.py:34-63); shuffled / sharded per rank under torch.distributed."""
    train_data, val_data = st_datasets(args, key)
    return rank_loaders(train_data, val_data, args.batch_size, 0)


def checkpoint_state(stream, epoch, model, optimizer):
    """The reference's checkpoint dict (spatialstream.py:235): storage-independent tensors (utils.owned_state_dict)."""
    return {'epoch': epoch, 'arch': STREAMS[stream]['arch'], 'state_dict': owned_state_dict(model),
            'optimizer': optimizer.state_dict()}


def main(stream, argv=None):
    """spatialstream.py / temporalstream.py as a function.  One process per GPU under torch.distributed.run (LOCAL_RANK /
    WORLD_SIZE set): gradients all-reduced (dp.attach), rank 0 writes the plot and the checkpoints.  Returns the model."""
    from .optim import FusedAdam
    spec = STREAMS[stream]
    args = build_parser(stream).parse_args(argv)
    if not torch.distributed.is_initialized():
        init_distributed(args)
    device = torch.device('cuda:' + args.device)
    train_loader, val_loader, train_sampler = make_loaders(args, spec['key'])
    model = build_model(stream, args.resume, args.pretrained_model)
    model.to(device)
    print('done!')
    criterion = make_criterion(args.loss_function, device)
    optimizer = FusedAdam(model.decoder.parameters(), lr=args.lr)           # spatialstream.py:216
    if torch.distributed.is_initialized():
        dp.attach(optimizer)
    os.makedirs(args.save_path, exist_ok=True)
    train_loss, val_loss, best_loss = [], [], 100
    for epoch in range(args.num_epoch):
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        train_loss.append(train_epoch(train_loader, model, criterion, optimizer, epoch, device, stream, args.hipgraph,
                                      augment=augment_spec(args)))
        loss1 = validate(val_loader, model, criterion, epoch, device, stream)
        val_loss.append(loss1)
        if dp.is_main():
            plot_loss(train_loss, val_loss, os.path.join(args.save_path, args.loss_save))
            print('epoch%05d, val loss is: %05f' % (epoch, loss1))
        if loss1 < best_loss:
            best_loss = loss1
            if dp.is_main():
                save_checkpoint(checkpoint_state(stream, epoch, model, optimizer), '%05d' % epoch + args.save_name,
                                args.save_path)
        dp.barrier()
    return model
