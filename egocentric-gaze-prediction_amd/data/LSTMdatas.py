"""Mirror of the reference's ``data/LSTMdatas.py``: consecutive files of extracted 512-vectors; sample i =
(file[i], file[i+1], same-video flag) (data/LSTMdatas.py:44-59)."""
import os

import torch
from torch.utils.data import Dataset


class lstmDataset(Dataset):
    def __init__(self, Path='../512w/test', name=None):
        self.Path = Path
        files = os.listdir(Path)
        self.listFiles = sorted(files if name is None else [k for k in files if name in k])

    def __len__(self):
        return len(self.listFiles) - 1

    def __getitem__(self, index):
        a, b = self.listFiles[index], self.listFiles[index + 1]
        return {'input': torch.load(os.path.join(self.Path, a)), 'gt': torch.load(os.path.join(self.Path, b)),
                'same': b[:-14] == a[:-14]}


def deferred_steps(samples):
    """The step schedule of AT's LSTM loops: ``samples`` yields (input, target, same) in loader order -> one
    (input of the previous sample, target of this one, reset) per scored step.  The reference scores the prediction made from
    sample i - 1 against the target of sample i (AT.py:127-145), so the forward pass of sample i - 1 is deferred until target i
    is known: the first sample yields nothing.  ``reset``: the state is zeroed before that forward pass -- on the first step,
    and wherever the deferred sample was flagged ``same`` false (AT.py:129-130).  The flag compares a file with its successor,
    so the reset falls on the forward pass of the last frame of a video: the reference's quirk, kept.
    Lazy: k steps have pulled k + 1 samples (the file loop reads nothing ahead); no device, no file is touched here."""
    samples = iter(samples)
    for prev_inp, _, _ in samples:           # the first sample only defers its input; its flag guards a forward pass that
        break                                # resets anyway (nothing ran before)
    else:
        return
    reset = True
    for inp, target, same in samples:
        yield prev_inp, target, reset
        prev_inp, reset = inp, not same
