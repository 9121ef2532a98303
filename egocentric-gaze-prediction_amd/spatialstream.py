"""Mirror of the reference's ``spatialstream.py``: pre-training of the spatial (RGB) stream -- the ``VGG`` model with a frozen
VGG16-BN encoder, ``train`` / ``validate`` and the CLI (spatialstream.py:15-236).  Implementation: streamtrain.py.  Run as
``python -m egaze_amd.spatialstream --imagePath ... --gtPath ...`` (nothing happens at import)."""
import torch

from . import streamtrain as _st
from .streamtrain import StreamVGG

STREAM = 'spatial'


class VGG(StreamVGG):
    """spatialstream.py:65-116: ``VGG(make_layers(cfg['D'], 3))``, encoder frozen, forward -> the gaze map."""

    def __init__(self, features):
        super(VGG, self).__init__(features, freeze_features=True)


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
