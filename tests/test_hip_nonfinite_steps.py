"""Non-finite propagation through literal trainer steps: a poisoned step reads back a NaN loss (as the fp64 / fp32 oracle's does),
raises FusedAdam's flag and leaves every parameter and both Adam moments bit for bit where they were (AT: all of them; SP: all
whose gradient is not exactly zero in torch too, see the test).

Every scenario makes ONE CLEAN STEP FIRST: with fresh (all-zero) moments a gradient that was wrongly turned into 0 would move
nothing either (m = v = 0 -> update 0) and the test would prove nothing; after a real step the moments are non-zero and a g = 0
"step" decays them and moves the weight.

SP: three plants (tests/nonfinite_ref.py: one NaN pixel of the flow input, one +inf in a mid-encoder conv weight, one NaN in a
decoder bias), each checked on the CPU to give the oracle a NaN loss (tests/test_nonfinite_ref_host.py).
AT: one NaN in h0, or in the input vector -- the stand-in for what a lost hand-off of the persistent launches writes (no hand-off
is lost here) -- at batch 1 (fused single-step kernels, wavefront, persistent) and at T, B = 3, 16 (wavefront, persistent), eager,
and at batch 1 through the graphed sample step with its loss ring.  A clean step made afterwards from reset state equals bit for
bit the same clean step of a twin run in which the poisoned step is replaced by an optimizer step whose every gradient is NaN (what
the contract says a poisoned step amounts to: everything skipped, the step counter advanced)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import nonfinite_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(t):
    return t.detach().clone().view(torch.int32)


def snapshot(opt):
    torch.cuda.synchronize()
    return bits(opt.flat_p), bits(opt.flat_m), bits(opt.flat_v)


def changed(opt, snap, names=None):
    """Per parameter: how many elements of (p, m, v) differ from the snapshot."""
    out = {}
    now = snapshot(opt)
    for i, (p, o) in enumerate(zip(opt.params, opt.offsets)):
        n = p.numel()
        d = tuple(int((now[j][o:o + n] != snap[j][o:o + n]).sum()) for j in range(3))
        if any(d):
            out[names[i] if names else i] = d
    return out


# ----------------------------------------------------------------------------- SP
@pytest.mark.parametrize("name", R.SP_PLANTS)
def test_sp_poisoned_step_does_not_reach_the_weights(name):
    import egaze_amd.hipops as H
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    from oracle import egaze_oracle as O
    from oracle import synth
    from test_hip_model_sp import build_model
    oloss, osd = R.sp_oracle_poisoned(name)
    assert torch.isnan(oloss)
    model, _ = build_model()
    model.train()
    crit = floss().to(DEV)
    opt = FusedAdam(model.parameters(), lr=R.SP_LR)
    names = [k for k, _ in model.named_parameters()]
    assert [p.data_ptr() for p in opt.params] == [p.data_ptr() for _, p in model.named_parameters()]

    def step(x_s, x_t, gt):
        opt.zero_grad()
        out = model(x_s.to(DEV), x_t.to(DEV))
        loss = crit(out, gt.to(DEV).view(out.size()))
        loss.backward()
        opt.step()
        return loss.item()

    x_s, x_t, gt, _ = synth.synth_sp_batch(R.SP_B, R.SP_SIZE, seed=40)
    assert torch.isfinite(torch.tensor(step(x_s, x_t, gt)))
    opt.check_finite()
    assert float(opt.flat_m.abs().max()) > 0 and float(opt.flat_v.abs().max()) > 0
    x_s, x_t, gt, _ = synth.synth_sp_batch(R.SP_B, R.SP_SIZE, seed=41)
    key, idx, kind = R.sp_plant_target(O.sp_shapes(), name)
    if key == "x_t":
        x_t[idx] = R.KINDS[kind]
    else:
        p = dict(model.named_parameters())[key]
        p.data[idx] = R.KINDS[kind]
        H.touch_params([p])                          # a write behind torch's back: its packings are stale
    snap = snapshot(opt)
    loss = step(x_s, x_t, gt)
    print(f"SP {name}: loss read back {loss}, oracle {oloss.item()}")
    assert loss != loss, f"the loss read back is {loss}, the oracle's is NaN"
    with pytest.raises(FloatingPointError):
        opt.check_finite()
    # Which elements may move.  torch itself gives some parameters of a poisoned step a gradient of exactly ZERO: the encoder whose
    # features lose the fusion maximum everywhere (the NaN stream wins it), and every filter below the plant whose ReLU is closed
    # on the whole batch (threshold_backward writes 0 there whatever the incoming gradient is).  Those elements take the g = 0 Adam
    # step torch takes; FusedAdam skips the elements whose gradient is NaN / inf.  So: an element with a non-finite gradient is
    # bit for bit where it was; an element that moved had a gradient of exactly zero; and the parameter tensors that hold non-finite
    # gradients are the oracle's.
    torch.cuda.synchronize()
    now, g = snapshot(opt), opt.flat_g.detach().clone()
    moved_el = (now[0] != snap[0]) | (now[1] != snap[1]) | (now[2] != snap[2])
    bad_g = ~torch.isfinite(g)
    print(f"SP {name}: {int(bad_g.sum())} of {g.numel()} gradient elements non-finite, {int(moved_el.sum())} elements moved, "
          f"{int((moved_el & bad_g).sum())} of them with a non-finite gradient, {int((moved_el & (g != 0)).sum())} with a non-zero one")
    assert int((moved_el & bad_g).sum()) == 0, "elements with a NaN / inf gradient took a step"
    assert int((moved_el & (g != 0)).sum()) == 0, "elements took a step on a finite non-zero gradient of a poisoned step"
    _, _, ograds = R.sp_oracle_poisoned(name, grads=True)
    want = {k for k, v in ograds.items() if not torch.isfinite(v).all()}
    got = {k for k, p, o in zip(names, opt.params, opt.offsets) if bad_g[o:o + p.numel()].any()}
    clean_stream = {k for k, v in ograds.items() if float(v.abs().max()) == 0.0}
    print(f"SP {name}: {len(got)} of {len(names)} parameter tensors hold non-finite gradients (oracle {len(want)}); all-zero in the "
          f"oracle: {len(clean_stream)}")
    # (the bias of a convolution under a train-mode BatchNorm: its gradient is identically zero, the HIP path writes that zero
    # instead of summing round-off -- functions._zero_bias_grad -- so its moments are zero and it never moves)
    pre_bn = {k for k in names if k.endswith(".bias") and k.split(".")[0] in ("features_s", "features_t", "fusion")
              and ograds[k[:-5] + ".weight"].dim() >= 4}
    assert len(pre_bn) == 27
    for k, p, o in zip(names, opt.params, opt.offsets):
        if k in pre_bn:
            assert float(g[o:o + p.numel()].abs().max()) == 0.0 and not moved_el[o:o + p.numel()].any(), k
    assert got == want - pre_bn, (sorted(got ^ (want - pre_bn)))
    assert len(want) >= len(names) // 3
    for k, p, o in zip(names, opt.params, opt.offsets):
        if k in clean_stream:
            assert float(g[o:o + p.numel()].abs().max()) == 0.0, k
    sd = model.state_dict()
    for k, v in osd.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert torch.equal(torch.isfinite(sd[k].cpu()), torch.isfinite(v)), k


# ----------------------------------------------------------------------------- LF
@pytest.mark.parametrize("name", sorted(R.LF_PLANTS))
def test_lf_poisoned_step_does_not_reach_the_weights(name):
    """The late-fusion step (deferred BatchNorm, the BN + ReLU operand prologues, the one-pass first-block backward): every
    gradient of a poisoned step is NaN here, so ALL of flat_p / flat_m / flat_v stay bit for bit (the biases under a train-mode
    BatchNorm have zero gradients and zero moments: they do not move either)."""
    import egaze_amd.hipops as H
    from egaze_amd.floss import floss
    from egaze_amd.models.late_fusion import late_fusion
    from egaze_amd.optim import FusedAdam
    from oracle import egaze_oracle as O
    from oracle import synth
    oloss, osd = R.lf_oracle_poisoned(name)
    assert torch.isnan(oloss)
    net = late_fusion()
    net.load_state_dict(synth.synth_state_dict(O.lf_shapes(), seed=3, head_gain=0.5))
    net = net.to(DEV).train()
    crit = floss()
    opt = FusedAdam(net.parameters(), lr=1e-4)

    def step(im, feat, gt):
        opt.zero_grad()
        out = net(feat.to(DEV), im.to(DEV))                  # LF.py:90 argument order
        loss = crit(out, gt.to(DEV))
        loss.backward()
        opt.step()
        return loss.item()

    assert torch.isfinite(torch.tensor(step(*synth.synth_lf_batch(R.LF_B, R.LF_SIZE, seed=7))))
    opt.check_finite()
    assert float(opt.flat_m.abs().max()) > 0
    im, feat, gt = synth.synth_lf_batch(R.LF_B, R.LF_SIZE, seed=8)
    key, idx, kind = R.LF_PLANTS[name]
    if key == "feat":
        feat[idx] = R.KINDS[kind]
    else:
        p = dict(net.named_parameters())[key]
        p.data[idx] = R.KINDS[kind]
        H.touch_params([p])
    snap = snapshot(opt)
    loss = step(im, feat, gt)
    print(f"LF {name}: loss read back {loss}, oracle {oloss.item()}")
    assert loss != loss, f"the loss read back is {loss}, the oracle's is NaN"
    with pytest.raises(FloatingPointError):
        opt.check_finite()
    moved = changed(opt, snap, [k for k, _ in net.named_parameters()])
    assert not moved, f"parameters that took a step (elements of p, m, v that moved): {moved}"
    sd = net.state_dict()
    for k, v in osd.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert torch.equal(torch.isfinite(sd[k].cpu()), torch.isfinite(v)), k


# ----------------------------------------------------------------------------- AT
def _net():
    from egaze_amd.models.LSTMnet import lstmnet
    from oracle import egaze_oracle as O
    from oracle import synth
    net = lstmnet()
    net.load_state_dict(synth.synth_state_dict(O.lstm_shapes(), seed=2))
    return net.to(DEV)


def _form(monkeypatch, form):
    import egaze_amd.hipops as H
    import egaze_amd.models.LSTMnet as M
    monkeypatch.setattr(M, "B1_FUSED", form == "fused")
    monkeypatch.setattr(H, "LSTM_PERSIST", form == "persist")


def _all_nan_step(opt):
    """An optimizer step whose every gradient is NaN: every element skipped, the flag raised, the counter advanced."""
    opt.zero_grad()
    opt.flat_g.fill_(float("nan"))
    opt.step()
    with pytest.raises(FloatingPointError):
        opt.check_finite()


@pytest.mark.parametrize("plant", sorted(R.AT_PLANTS))
@pytest.mark.parametrize("T,B,form", [(1, 1, "fused"), (1, 1, "wave"), (1, 1, "persist"), (3, 16, "wave"), (3, 16, "persist")])
def test_at_poisoned_step_eager(T, B, form, plant, monkeypatch):
    import egaze_amd.hipops as H
    from egaze_amd.functions import MSELoss
    from egaze_amd.optim import FusedAdam
    _form(monkeypatch, form)
    if form == "persist":
        assert H.lstm_persist_ok(2, B, 512)
    oloss = R.at_oracle_loss(*R.at_poisoned_inputs(T, B, 2, plant))
    assert torch.isnan(oloss)

    def run(poisoned):
        net = _net()
        opt = FusedAdam(net.parameters(), lr=1e-4)

        def step(x, tgt, h0, c0):
            opt.zero_grad()
            pred, _ = net(x.to(DEV), (h0.to(DEV), c0.to(DEV)))
            loss = MSELoss.apply(pred, tgt.to(DEV), True)          # criterion(pred, tanh(target)), AT.py:138
            loss.backward()
            opt.step()
            return loss.item()

        assert torch.isfinite(torch.tensor(step(*R.at_inputs(T, B, 1))))
        opt.check_finite()
        snap = snapshot(opt)
        assert int((snap[1] != 0).sum()) > 0
        if poisoned:
            loss = step(*R.at_poisoned_inputs(T, B, 2, plant))
            print(f"AT {T}x{B} {form} {plant}: loss read back {loss}, oracle {oloss.item()}")
            assert loss != loss, f"the loss read back is {loss}, the oracle's is NaN"
            with pytest.raises(FloatingPointError):
                opt.check_finite()
            moved = changed(opt, snap, [k for k, _ in net.named_parameters()])
            assert not moved, f"parameters that took a step (elements of p, m, v that moved): {moved}"
        else:
            _all_nan_step(opt)
            assert not changed(opt, snap)
        after = step(*R.at_inputs(T, B, 3))                          # a clean step from reset (clean) state
        opt.check_finite()
        assert H.lstm_persist_status() == 0
        return after, snapshot(opt)

    got, twin = run(True), run(False)
    assert got[0] == twin[0], (got[0], twin[0])
    for a, b, what in zip(got[1], twin[1], ("p", "m", "v")):
        assert torch.equal(a, b), f"flat_{what} after the clean step differs from the twin run in {int((a != b).sum())} elements"


@pytest.mark.parametrize("plant", sorted(R.AT_PLANTS))
def test_at_poisoned_step_graphed(plant, monkeypatch):
    """The batch-1 sample step replayed from its hipGraph, losses parked in the ring: the poisoned replay parks a NaN, the drain
    raises, nothing moved; after reset_state() the next replay equals the twin run's."""
    import egaze_amd.hipops as H
    from egaze_amd.AT import RING, _GraphedSampleStep, _LossRing
    from egaze_amd.optim import FusedAdam
    _form(monkeypatch, "fused")
    xp, tp, hp, _ = R.at_poisoned_inputs(1, 1, 2, plant)
    assert torch.isnan(R.at_oracle_loss(xp, tp, hp if plant == "h0" else torch.zeros(2, 1, 512), torch.zeros(2, 1, 512)))

    def run(poisoned):
        net = _net()
        opt = FusedAdam(net.parameters(), lr=1e-4)
        ring = torch.zeros(RING // 2, device=DEV)
        runner = _GraphedSampleStep(net, opt, torch.device(DEV), 512, ring)
        parked = _LossRing(ring, opt)
        stage = torch.empty((8, 2, 512), dtype=torch.float32).pin_memory()
        try:
            n = _GraphedSampleStep.WARM + 2                           # eager warm-up steps, the capture's first replay, one more
            for i in range(n):
                x, tgt, _, _ = R.at_inputs(1, 1, 10 + i)
                stage[i][0].copy_(x.view(-1)); stage[i][1].copy_(tgt.view(-1))
                runner.step(stage[i])
                parked.stepped()
            assert runner.graph is not None
            clean = parked.drain()
            assert len(clean) == n and all(v == v and abs(v) < float("inf") for v in clean)
            snap = snapshot(opt)
            if poisoned:
                x, tgt, h0, _ = R.at_poisoned_inputs(1, 1, 2, plant)
                if plant == "h0":
                    runner.state[0].copy_(h0.to(DEV))                # the carried h with one NaN element
                stage[n][0].copy_(x.view(-1)); stage[n][1].copy_(tgt.view(-1))
                slot = int(opt.step_dev[0].item()) % ring.numel()
                runner.step(stage[n])
                parked.stepped()
                torch.cuda.synchronize()
                loss = float(ring[slot])
                print(f"AT graphed {plant}: loss parked {loss}")
                assert loss != loss, f"the loss parked by the poisoned replay is {loss}, the oracle's is NaN"
                with pytest.raises(FloatingPointError):
                    parked.drain()
                moved = changed(opt, snap, [k for k, _ in net.named_parameters()])
                assert not moved, f"parameters that took a step (elements of p, m, v that moved): {moved}"
            else:
                _all_nan_step(opt)
                assert not changed(opt, snap)
            runner.reset_state()
            x, tgt, _, _ = R.at_inputs(1, 1, 30)
            stage[n + 1][0].copy_(x.view(-1)); stage[n + 1][1].copy_(tgt.view(-1))
            slot = int(opt.step_dev[0].item()) % ring.numel()
            runner.step(stage[n + 1])
            torch.cuda.synchronize()
            after = float(ring[slot])
            opt.check_finite()
            assert H.lstm_persist_status() == 0
            return after, snapshot(opt)
        finally:
            runner.close()

    got, twin = run(True), run(False)
    assert got[0] == got[0] and got[0] == twin[0], (got[0], twin[0])
    for a, b, what in zip(got[1], twin[1], ("p", "m", "v")):
        assert torch.equal(a, b), f"flat_{what} after the clean replay differs from the twin run in {int((a != b).sum())} elements"
