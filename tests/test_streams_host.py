"""Host-side tests of the stream pre-training scripts (egaze_amd.spatialstream / temporalstream, implementation in
streamtrain.py): model layout against the reference's own ``VGG`` (key list stored by tests/golden/make_golden_streams.py),
the CLI flags and defaults, import without side effects, weight loading for ``--resume 0 / 1`` and the checkpoint format."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _models():
    import egaze_amd  # noqa: F401
    from egaze_amd import spatialstream, temporalstream
    from egaze_amd.utils import cfg, make_layers
    return (spatialstream.VGG(make_layers(cfg['D'], 3)), temporalstream.VGG(make_layers(cfg['D'], 20)))


@pytest.mark.parametrize("tag", ["spatial_stream_s32", "temporal_stream_s32", "spatial_stream_s224"])
def test_state_dict_layout_matches_reference(tag):
    from oracle import egaze_oracle as O
    sp, tp = _models()
    model = sp if tag.startswith("spatial") else tp
    keys = [str(k) for k in np.load(os.path.join(GOLDEN, tag + ".npz"))["keys"]]
    assert list(model.state_dict().keys()) == keys
    want = O.spatial_vgg_shapes()
    if tag.startswith("temporal"):
        want["features.0.weight"] = (64, 20, 3, 3)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == {k: tuple(v) for k, v in want.items()}
    decoder_idx = sorted({int(k.split('.')[1]) for k in keys if k.startswith("decoder.")})
    assert decoder_idx == [0, 2, 4, 7, 9, 11, 14, 16, 18, 21, 23, 26, 28, 30]


def test_freezing_and_strict_cross_loading():
    from egaze_amd.run_spatialstream import VGG as DemoVGG
    from egaze_amd.utils import cfg, make_layers
    sp, tp = _models()
    assert not any(p.requires_grad for p in sp.features.parameters())          # spatialstream.py:70-71
    assert all(p.requires_grad for p in tp.features.parameters())              # temporalstream.py: not frozen
    assert all(p.requires_grad for p in sp.decoder.parameters())
    demo = DemoVGG(make_layers(cfg['D'], 3))
    demo.load_state_dict(sp.state_dict(), strict=True)
    sp.load_state_dict(demo.state_dict(), strict=True)


SPATIAL_DEFAULTS = dict(lr=1e-7, loss_save='loss_spatial.png', save_name='_spatial.pth.tar', save_path='save',
                        loss_function='f', num_epoch=10, device='0', resume=0,
                        pretrained_model='save/best_spatial.pth.tar', batch_size=16, flowPath='../gtea_imgflow',
                        imagePath='../gtea_images', fixsacPath='../fixsac', gtPath='../gtea_gts', val_name='Alireza',
                        hipgraph=False)


@pytest.mark.parametrize("stream", ["spatial", "temporal"])
def test_parser_flags_and_defaults(stream):
    import egaze_amd  # noqa: F401
    import importlib
    mod = importlib.import_module(f"egaze_amd.{stream}stream")
    want = dict(SPATIAL_DEFAULTS)
    if stream == "temporal":
        want.update(loss_save='loss_temporal.png', save_name='best_temporal.pth.tar')
    args = mod.build_parser().parse_args([])
    assert vars(args) == want
    a = mod.build_parser().parse_args(['--lr', '1e-4', '--resume', '1', '--batch_size', '4', '--num_epoch', '2'])
    assert (a.lr, a.resume, a.batch_size, a.num_epoch) == (1e-4, 1, 4, 2)


def test_import_has_no_side_effects(tmp_path):
    """The reference scripts parse argv, list the data folders and download VGG16-BN at import; the mirrors do nothing."""
    code = ("import os, sys, torch.utils.model_zoo as mz\n"
            "sys.argv = ['x', '--not-a-flag']\n"
            "def boom(*a, **k): raise AssertionError('side effect at import')\n"
            "os.listdir = boom; mz.load_url = boom\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import egaze_amd.spatialstream, egaze_amd.temporalstream, egaze_amd.streamtrain\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "ok"
    assert os.listdir(str(tmp_path)) == []


def _fake_vgg(path):
    from egaze_amd.utils import cfg, make_layers
    torch.manual_seed(3)
    enc = make_layers(cfg['D'], 3)
    sd = collections.OrderedDict(('features.' + k, v.clone().normal_(0, 0.05) if v.is_floating_point() else v.clone())
                                 for k, v in enc.state_dict().items())
    sd['classifier.0.weight'] = torch.zeros(4, 4)
    torch.save(sd, path)
    return sd


def test_build_model_resume0_and_resume1(tmp_path, monkeypatch):
    import egaze_amd  # noqa: F401
    from egaze_amd import streamtrain
    vgg = _fake_vgg(str(tmp_path / "vgg.pth"))
    monkeypatch.setenv("EGAZE_VGG16_BN", str(tmp_path / "vgg.pth"))
    sp = streamtrain.build_model('spatial', 0)
    assert torch.equal(sp.features[0].weight.detach(), vgg['features.0.weight'])
    assert torch.equal(sp.features[40].weight.detach(), vgg['features.40.weight'])
    tp = streamtrain.build_model('temporal', 0)
    rgb = vgg['features.0.weight']
    assert torch.allclose(tp.features[0].weight.detach(), rgb.mean(1, keepdim=True).repeat(1, 20, 1, 1))
    assert torch.equal(tp.features[1].weight.detach(), vgg['features.1.weight'])
    # change_key_names keeps the first 25 entries only (utils.py:78-94): the deeper layers keep their init
    assert not torch.equal(tp.features[40].weight.detach(), vgg['features.40.weight'])
    # resume 1: the whole state dict is merged from --pretrained_model
    torch.save({'epoch': 3, 'state_dict': tp.state_dict()}, str(tmp_path / "t.pth"))
    tp2 = streamtrain.build_model('temporal', 1, str(tmp_path / "t.pth"))
    for k, v in tp.state_dict().items():
        assert torch.equal(tp2.state_dict()[k], v), k


@pytest.mark.parametrize("stream,arch", [("spatial", "rgb"), ("temporal", "flow")])
def test_checkpoint_format(stream, arch, tmp_path):
    import egaze_amd  # noqa: F401
    from egaze_amd import streamtrain
    from egaze_amd.utils import save_checkpoint
    sp, tp = _models()
    model = sp if stream == "spatial" else tp
    opt = torch.optim.Adam(model.decoder.parameters(), lr=1e-7)
    state = streamtrain.checkpoint_state(stream, 4, model, opt)
    assert set(state) == {'epoch', 'arch', 'state_dict', 'optimizer'}
    assert state['epoch'] == 4 and state['arch'] == arch
    name = '%05d' % 4 + streamtrain.STREAMS[stream]['save_name']
    save_checkpoint(state, name, str(tmp_path))
    ck = torch.load(str(tmp_path / name), map_location='cpu', weights_only=False)
    assert list(ck['state_dict']) == list(model.state_dict())
    assert len({v.untyped_storage().data_ptr() for v in ck['state_dict'].values()}) == len(ck['state_dict'])
    assert len(ck['optimizer']['param_groups'][0]['params']) == 28              # the decoder's 14 convs
    assert name == ('00004_spatial.pth.tar' if stream == 'spatial' else '00004best_temporal.pth.tar')
