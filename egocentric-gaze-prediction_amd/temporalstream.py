"""Mirror of the reference's ``temporalstream.py``: pre-training of the temporal (optical-flow) stream -- the ``VGG`` model on the
20-channel flow stack, ``train`` / ``validate`` and the CLI (temporalstream.py:14-232).  Implementation: streamtrain.py.  Run as
``python -m egaze_amd.temporalstream --flowPath ... --gtPath ...`` (nothing happens at import)."""
import torch

from . import streamtrain as _st
from .streamtrain import StreamVGG

STREAM = 'temporal'


class VGG(StreamVGG):
    """temporalstream.py:63-111: ``VGG(make_layers(cfg['D'], 20))``, encoder NOT frozen (the reference still optimises the
    decoder only), forward -> the gaze map."""

    def __init__(self, features):
        super(VGG, self).__init__(features, freeze_features=False)


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def train(train_loader, model, criterion, optimizer, epoch, device=None, hipgraph=False):
    return _st.train_epoch(train_loader, model, criterion, optimizer, epoch, device or _device(), STREAM, hipgraph)


def validate(val_loader, model, criterion, epoch, device=None):
    return _st.validate(val_loader, model, criterion, epoch, device or _device(), STREAM)


def build_parser():
    return _st.build_parser(STREAM)


def main(argv=None):
    return _st.main(STREAM, argv)


if __name__ == '__main__':
    main()
