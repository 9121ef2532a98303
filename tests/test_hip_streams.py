"""GPU tests of the stream pre-training scripts (egaze_amd.spatialstream / temporalstream, implementation streamtrain.py):
literal reference training steps and ``validate`` against tests/golden/{spatial,temporal}_stream_*.npz (made by
tests/golden/make_golden_streams.py from the reference's own ``VGG`` / ``train`` / ``validate``), the captured step against
the eager one, the checkpoint hand-off to run_spatialstream and SP, the native-kernel path and the 2-rank data-parallel
path."""
import collections
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = {"spatial": 5, "temporal": 6}         # make_golden_streams.py
FIXTURES = [("spatial", 32, "s32"), ("temporal", 32, "s32"), ("spatial", 224, "s224")]


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def robust_close(a, b, max_tol=0.15, norm_tol=3e-2):
    """As in test_hip_model_sp.py: relative L2 within 3e-2 and max-rel within 0.15 (a ReLU decision flipped by rounding moves
    single entries; an indexing / formula bug fails both by far)."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    mx = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    l2 = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    return mx < max_tol and l2 < norm_tol, (mx, l2)


def _module(stream):
    import importlib
    import egaze_amd  # noqa: F401
    return importlib.import_module(f"egaze_amd.{stream}stream")


def build(stream, seed=None):
    from egaze_amd.utils import cfg, make_layers
    mod = _module(stream)
    model = mod.VGG(make_layers(cfg['D'], 3 if stream == "spatial" else 20))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.synth_state_dict(shapes, seed=SEEDS[stream] if seed is None else seed, head_gain=0.25))
    return model.to(DEV), mod


def gmap(gold, k):
    """A stored map, decoded: maps above 64 x 64 are kept as round(v * 65535) in uint16 (make_golden_streams.compact_map)."""
    a = gold[k]
    return a.astype(np.float64) / 65535.0 if a.dtype == np.uint16 else a


def key_of(stream):
    return "image" if stream == "spatial" else "flow"


@pytest.mark.parametrize("stream,size,tag", FIXTURES)
def test_golden_train_steps(stream, size, tag):
    """Two literal reference iterations (spatialstream.py:130-141) through the port's ``train``: train-mode encoder under
    no_grad, decoder forward / backward, floss, FusedAdam over the decoder.  Bounds as test_model_sp_train_step."""
    from egaze_amd import streams
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    gold = np.load(os.path.join(GOLDEN, f"{stream}_stream_{tag}.npz"))
    model, mod = build(stream)
    lr = float(gold["lr"])
    model.eval()
    x_s, x_t, gt, _ = synth.synth_sp_batch(2, size, seed=0)
    x = x_s if stream == "spatial" else x_t
    with torch.no_grad():
        out_eval = model(x.to(DEV))
    assert rel(out_eval.cpu().numpy(), gmap(gold, "eval_out")) < 1e-4
    enc0 = {k: p.detach().clone() for k, p in model.features.named_parameters()}
    dec0 = {k: p.detach().cpu().clone() for k, p in model.decoder.named_parameters()}
    optimizer = FusedAdam(model.decoder.parameters(), lr=lr)
    outs, losses, grads = [], [], []
    h = model.decoder.register_forward_hook(lambda m, i, o: outs.append(o.detach().cpu().clone()))
    crit = floss().to(DEV)

    def criterion(o, t):
        loss = crit(o, t)
        losses.append(loss.item())
        return loss

    def grab():
        streams.join_all_into_current()
        grads.append({k: p.grad.detach().cpu().clone() for k, p in model.decoder.named_parameters()})
    optimizer.pre_step_hooks.append(grab)
    loader = [{key_of(stream): x, "gt": gt}, {key_of(stream): x, "gt": gt}]
    mod.train(loader, model, criterion, optimizer, 0, DEV)
    h.remove()
    assert len(outs) == 2 and len(losses) == 2
    for s in (0, 1):
        r = rel(outs[s].numpy(), gmap(gold, f"train_out{s + 1}"))
        assert r < 1e-4, (s, r)
        want = float(gold[f"train_loss{s + 1}"])
        assert abs(losses[s] - want) < 1e-4 * abs(want), (s, losses[s], want)
    g1 = {"decoder." + k: v for k, v in grads[0].items()}
    keys = [k[5:] for k in gold.files if k.startswith("gsum/")]
    assert set(keys) == set(g1)
    floor = 1e-5 * max(gold["gsum/" + k][0] for k in keys)
    for k in keys:
        want, got = gold["gsum/" + k][0], g1[k].double().norm().item()
        assert abs(got - want) <= 5e-3 * want + floor, (k, got, want)
    for k in [f[5:] for f in gold.files if f.startswith("grad/")]:
        if gold["gsum/" + k][0] > 100 * floor:
            good, info = robust_close(g1[k].numpy(), gold["grad/" + k])
            assert good, (k, info)
    sd = model.state_dict()
    for f in gold.files:
        if f.startswith("after/"):
            assert rel(sd[f[6:]].cpu().numpy(), gold[f]) < 1e-4, f
        elif f.startswith("after_sum/"):
            v = sd[f[10:]].double().cpu()           # (a sum can cancel: held to 1e-4 of the norm)
            assert abs(v.norm().item() - gold[f][1]) <= 1e-4 * gold[f][1], f
            assert abs(v.sum().item() - gold[f][0]) <= 1e-4 * gold[f][1], f
        elif f.startswith("delta/") and gold["gsum/" + f[6:]][0] > 100 * floor:
            d = (sd[f[6:]].cpu() - dec0[f[14:]]).double()
            assert abs(d.abs().max().item() - gold[f][1]) < 2e-2 * lr + 1e-9, f
    for k, v in sd.items():
        if k.startswith("features.") and k.endswith("num_batches_tracked"):
            assert int(v) == 2, k
    for k, p in model.features.named_parameters():        # never updated, never given a gradient
        assert torch.equal(p.detach(), enc0[k]), k
        assert p.grad is None, k
    assert optimizer.step_count == 2


@pytest.mark.parametrize("stream,size,tag", FIXTURES)
def test_validate_matches_reference(stream, size, tag):
    """spatialstream.py:154-184 on a loader of a batch of 2 and a batch of 1 (the per-sample and the 2-D branch of
    computeAAEAUC): mean loss, AUC and AAE.  The maps differ from the reference's by ~1e-5 relative, so the AAE (a centre of
    mass) is held to 1e-4 degrees; the AUC proxy counts pixels and matches exactly."""
    from egaze_amd import streamtrain
    from egaze_amd.floss import floss
    gold = np.load(os.path.join(GOLDEN, f"{stream}_stream_{tag}.npz"))
    model, mod = build(stream)
    v_s, v_t, v_gt, _ = synth.synth_sp_batch(3, size, seed=7)
    v = v_s if stream == "spatial" else v_t
    loader = [{key_of(stream): v[:2], "gt": v_gt[:2]}, {key_of(stream): v[2:], "gt": v_gt[2:]}]
    crit = floss().to(DEV)
    loss, auc, aae = streamtrain.evaluate(loader, model, crit, 0, DEV, stream)
    assert abs(loss - float(gold["val_loss"])) < 1e-4 * abs(float(gold["val_loss"]))
    assert abs(aae - gold["val_aae"].mean()) < 1e-4, (aae, gold["val_aae"])
    assert abs(auc - gold["val_auc"].mean()) < 1e-12, (auc, gold["val_auc"])
    assert mod.validate(loader, model, crit, 0, DEV) == loss
    assert not model.training


def _eager_steps(model, crit, opt, batches):
    from egaze_amd import streamtrain
    outs, losses = [], []
    for x, g in batches:
        o = streamtrain.step_forward(model, x)
        loss = crit(o, g.view(o.size()))
        loss.backward()
        opt.step()
        opt.zero_grad()
        outs.append(o.detach().clone())
        losses.append(loss.item())
    return outs, losses


def _state(model, opt):
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return sd, opt.flat_m.clone(), opt.flat_v.clone(), opt.step_count


@pytest.mark.parametrize("stream", ["spatial", "temporal"])
def test_graphed_step_bit_identical_and_follows_encoder_loads(stream):
    """7 full batches through the captured step (2 warm-up steps, the capture, replays) + a trailing partial batch (eager, as
    train_epoch runs it) == the eager loop, bit for bit: outputs, losses, decoder parameters, Adam moments and step count,
    encoder running statistics.  Before the 7th step an outside ``features.load_state_dict`` lands in both models: the replay
    must see it (the frozen encoder's packed weights are rebuilt before the next replay)."""
    from egaze_amd import streamtrain
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    x_s, x_t, gt, _ = synth.synth_sp_batch(15, 32, seed=11)
    x = (x_s if stream == "spatial" else x_t).to(DEV)
    gt = gt.to(DEV)
    batches = [(x[2 * i:2 * i + 2], gt[2 * i:2 * i + 2]) for i in range(7)] + [(x[14:], gt[14:])]
    runs = []
    for graphed in (False, True):
        model, _ = build(stream)
        model.train()
        new = synth.synth_state_dict({k: tuple(v.shape) for k, v in model.features.state_dict().items()}, seed=21)
        opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
        crit = floss().to(DEV)
        opt.zero_grad()
        step = streamtrain.GraphedStreamStep(model, crit, opt, batches[0]) if graphed else None
        outs, losses = [], []
        for i, (xb, gb) in enumerate(batches):
            if i == 6:
                model.features.load_state_dict(new)
            if step is not None and i < 7:
                loss, o = step(xb, gb)
                outs.append(o.clone())
                losses.append(loss.item())
            else:
                if step is not None:
                    opt.zero_grad()                # as train_epoch does after replays
                o, l_ = _eager_steps(model, crit, opt, [(xb, gb)])
                outs += o
                losses += l_
        if step is not None:
            assert step.step.graph is not None and step.step.calls == 7
            step.close()
        runs.append((outs, losses, _state(model, opt)))
    (oe, le, se), (og, lg, sg) = runs
    assert le == lg
    for i, (a, b) in enumerate(zip(oe, og)):
        assert torch.equal(a, b), i
    for k in se[0]:
        assert torch.equal(se[0][k], sg[0][k]), k
    assert torch.equal(se[1], sg[1]) and torch.equal(se[2], sg[2]) and se[3] == sg[3] == 8
    assert int(sg[0]["features.1.num_batches_tracked"]) == 2      # reset to 0 by the load before step 7, then 7 and 8


def test_train_epoch_interrupted_with_the_step_open():
    """train_epoch(hipgraph=True) over four batches of 2 at 32 x 32 whose third batch raises (GraphedStreamStep is built at the
    first batch and puts the optimizer into capturable mode; its first two calls are its eager warm-up steps): the step is
    closed on the way out -- the optimizer has left capturable mode and its host step count is the number of completed steps,
    the device counter's -- and an eager epoch on the same objects runs.  (test_hip_lf.py holds LF._run to the same.)"""
    import math
    from egaze_amd import streamtrain
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    x_s, _, gt, _ = synth.synth_sp_batch(8, 32, seed=13)
    batches = [{"image": x_s[2 * i:2 * i + 2], "gt": gt[2 * i:2 * i + 2]} for i in range(4)]
    model, _ = build("spatial")
    opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
    crit = floss().to(DEV)

    class Broken:
        def __len__(self):
            return len(batches)

        def __iter__(self):
            yield batches[0]
            yield batches[1]
            raise RuntimeError("third batch")
    with pytest.raises(RuntimeError, match="third batch"):
        streamtrain.train_epoch(Broken(), model, crit, opt, 0, DEV, "spatial", hipgraph=True)
    torch.cuda.synchronize()
    # (the loader runs one batch ahead of the step: the error arrives while step 1 or 2 is the last one issued)
    assert not opt.capturable and opt.step_count in (1, 2)
    assert int(opt.step_dev[0].item()) == opt.step_count
    done = opt.step_count
    loss = streamtrain.train_epoch(batches, model, crit, opt, 1, DEV, "spatial", hipgraph=False)
    assert math.isfinite(loss) and loss > 0
    assert not opt.capturable and opt.step_count == done + 4


def _write_dataset(root, size=32):
    """The reference's on-disk layout (data/STdatas.py): flow/<video>/flow_{x,y}_NNNNN.jpg, images, gt maps named
    <video>_000000_NNNNN.png, fixation files; 3 training frames (batches of 2 + 1) and 2 validation frames ('Alireza')."""
    from PIL import Image
    rs = np.random.RandomState(0)
    for d in ("flow", "img", "gt", "fs"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for video, frames in (("Ahmad_American", (10, 11, 12)), ("Alireza_American", (11, 12))):
        os.makedirs(os.path.join(root, "flow", video), exist_ok=True)
        for n in range(1, 13):
            for ax in "xy":
                Image.fromarray(rs.randint(0, 256, (size, size)).astype(np.uint8)).save(
                    os.path.join(root, "flow", video, f"flow_{ax}_{n:05d}.jpg"))
        for n in frames:
            Image.fromarray(rs.randint(0, 256, (size, size, 3)).astype(np.uint8)).save(
                os.path.join(root, "img", f"{video}_img_{n:05d}.png"))
            yy, xx = np.mgrid[0:size, 0:size]
            cy, cx = rs.uniform(4, size - 4, 2)
            g = np.round(255 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 20.0)).astype(np.uint8)
            Image.fromarray(g).save(os.path.join(root, "gt", f"{video}_000000_{n:05d}.png"))
        np.savetxt(os.path.join(root, "fs", video + ".txt"), np.ones(len(frames)))
    return ["--flowPath", os.path.join(root, "flow"), "--imagePath", os.path.join(root, "img"), "--gtPath",
            os.path.join(root, "gt"), "--fixsacPath", os.path.join(root, "fs")]


def _fake_vgg(path):
    from egaze_amd.utils import cfg, make_layers
    torch.manual_seed(3)
    enc = make_layers(cfg['D'], 3)
    sd = collections.OrderedDict(('features.' + k, v.clone().normal_(0, 0.05) if v.is_floating_point() else v.clone())
                                 for k, v in enc.state_dict().items())
    for k in list(sd):
        if k.endswith('running_var'):
            sd[k] = sd[k].abs() + 0.5
    sd['classifier.0.weight'] = torch.zeros(4, 4)
    torch.save(sd, path)
    return sd


class _SPData(torch.utils.data.Dataset):
    def __init__(self, n, size, seed):
        self.im, self.fl, self.gt, self.fs = synth.synth_sp_batch(n, size, seed=seed)

    def __len__(self):
        return self.im.shape[0]

    def __getitem__(self, i):
        return {'image': self.im[i], 'flow': self.fl[i], 'gt': self.gt[i], 'fixsac': self.fs[i],
                'imname': 'frame_%05d.jpg' % i}


def test_checkpoint_hand_off(tmp_path, monkeypatch):
    """spatialstream.main / temporalstream.main for one epoch on files (resume 0 from a VGG16-BN file), then: resume 1 restores
    the weights, the spatial checkpoint loads strictly into run_spatialstream.VGG and SpatialPipeline runs on it, and SP's
    resume-1 path still loads nothing into its encoders from either checkpoint."""
    from egaze_amd import spatialstream, temporalstream
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.run_spatialstream import VGG as DemoVGG, SpatialPipeline
    from egaze_amd.SP import SP
    from egaze_amd.utils import cfg, make_layers
    vgg = _fake_vgg(str(tmp_path / "vgg.pth"))
    monkeypatch.setenv("EGAZE_VGG16_BN", str(tmp_path / "vgg.pth"))
    data = _write_dataset(str(tmp_path / "data"))
    save = str(tmp_path / "save")
    common = data + ["--save_path", save, "--num_epoch", "1", "--batch_size", "2", "--lr", "1e-4"]
    ck_path = {}
    for stream, mod, arch, name in (("spatial", spatialstream, "rgb", "00000_spatial.pth.tar"),
                                    ("temporal", temporalstream, "flow", "00000best_temporal.pth.tar")):
        model = mod.main(common)
        ck_path[stream] = os.path.join(save, name)
        ck = torch.load(ck_path[stream], map_location='cpu', weights_only=False)
        assert set(ck) == {'epoch', 'arch', 'state_dict', 'optimizer'} and ck['arch'] == arch and ck['epoch'] == 0
        keys = [str(k) for k in np.load(os.path.join(GOLDEN, f"{stream}_stream_s32.npz"))["keys"]]
        assert list(ck['state_dict']) == keys                  # the reference VGG's key list
        assert ck['optimizer']['state'][0]['step'] == 2         # 3 frames, batches of 2 + 1
        w0 = vgg['features.0.weight']
        want0 = w0 if stream == "spatial" else w0.mean(1, keepdim=True).repeat(1, 20, 1, 1)
        assert torch.allclose(ck['state_dict']['features.0.weight'], want0)        # encoder: loaded, never updated
        assert int(ck['state_dict']['features.1.num_batches_tracked']) == 2
        again = mod.main(data + ["--save_path", save, "--num_epoch", "0", "--resume", "1", "--pretrained_model",
                                 ck_path[stream]])
        for k, v in ck['state_dict'].items():
            assert torch.equal(again.state_dict()[k].cpu(), v), k
    # run_spatialstream (BASELINE config 1) takes the spatial checkpoint strictly
    demo = DemoVGG(make_layers(cfg['D'], 3))
    demo.load_state_dict(torch.load(ck_path["spatial"], map_location='cpu', weights_only=False)['state_dict'])
    demo.to(DEV).eval()
    pipe = SpatialPipeline(demo, late_fusion().to(DEV).eval()).eval()
    with torch.no_grad():
        out, feat, com, vec, weighted, fin = pipe(torch.randn(1, 3, 224, 224, device=DEV))
    assert tuple(fin.shape) == (1, 1, 224, 224) and bool(torch.isfinite(fin).all())
    # SP(resume=1) filters the checkpoints with un-stripped keys: nothing reaches its encoders
    sp = SP(lr=1e-4, save_path=save, save_name='sp.pth.tar', num_epoch=1, batch_size=2, device='0', resume=1,
            pretrained_spatial=ck_path["spatial"], pretrained_temporal=ck_path["temporal"],
            traindata=_SPData(2, 32, 0), valdata=_SPData(2, 32, 1))
    for stream, enc in (("spatial", sp.model.features_s), ("temporal", sp.model.features_t)):
        sd = torch.load(ck_path[stream], map_location='cpu', weights_only=False)['state_dict']
        for k, v in enc.state_dict().items():
            if v.dim() == 4:                                # conv weights: random init vs loaded / trained values
                assert not torch.equal(v.cpu(), sd['features.' + k]), (stream, k)


FORBIDDEN = re.compile(r"miopen|rocblas|hipblaslt|Cijk_|at::native.*(conv|gemm|batch_norm|norm_|loss|bce|binary_cross|"
                       r"im2col|col2im|upsample|sigmoid)", re.IGNORECASE)


@pytest.mark.parametrize("stream", ["spatial", "temporal"])
def test_native_kernels_only(stream):
    """One eager training step under torch.profiler: every convolution, batch-norm, upsample, sigmoid and loss kernel is this
    package's own -- nothing from MIOpen, rocBLAS / hipBLASLt or an at::native convolution / GEMM / norm / loss."""
    from torch.profiler import ProfilerActivity, profile
    from egaze_amd import streamtrain
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    model, _ = build(stream)
    model.train()
    opt = FusedAdam(model.decoder.parameters(), lr=1e-4)
    crit = floss().to(DEV)
    x_s, x_t, gt, _ = synth.synth_sp_batch(2, 64, seed=1)
    x, gt = (x_s if stream == "spatial" else x_t).to(DEV), gt.to(DEV)
    _eager_steps(model, crit, opt, [(x, gt)])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _eager_steps(model, crit, opt, [(x, gt)])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 30, names
    bad = sorted({n for n in names if FORBIDDEN.search(n)})
    assert not bad, bad


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("stream", ["spatial", "temporal"])
def test_two_ranks_one_gpu(stream, tmp_path):
    """2 ranks on the one GPU over gloo (tests/stream_dp_worker.py): the reduced decoder gradient is the sum of the two local
    gradients bit for bit, the replicas are bit-identical after two steps, and the encoders are untouched."""
    prefix = str(tmp_path / "obs")
    env = dict(os.environ)
    env.update(EGAZE_SINGLE_DEVICE="1", EGAZE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("EGAZE_PRECISION", None)
    env.pop("EGAZE_STREAMS", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "stream_dp_worker.py"), prefix, stream]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    obs = [torch.load(f"{prefix}.{k}") for k in range(2)]
    g0, g1 = obs[0]["g_local"]
    assert not torch.equal(g0, g1) and g0.abs().max() > 0 and g1.abs().max() > 0
    for o in obs:
        assert o["n_buckets"] >= 2 and o["grad_scale"] == 0.5
        assert torch.equal(o["g_sum"], g0 + g1), (o["g_sum"] - (g0 + g1)).abs().max()
        assert torch.equal(o["enc"], o["enc0"])
        assert o["enc_grads_none"]
    assert torch.equal(obs[0]["flat_p"], obs[1]["flat_p"])
    assert torch.equal(obs[0]["enc"], obs[1]["enc"])
    assert all(l == l for o in obs for l in o["losses"]) and obs[0]["losses"] != obs[1]["losses"]
