"""What the weight caches rely on in torch, pinned on the CPU (no GPU): hipops.packing._tag keys every packed weight, BatchNorm
fold and eval row by (global epoch, per-tensor epoch, torch version counter, address) and _uid gives the tensor an identity
that dies with it.  A torch upgrade that changes how a route moves the version counter fails here first; the GPU side of every
route is tests/test_hip_cache_coherence.py.  The two routes torch cannot see (``.data`` writes, raw pointers) are pinned as
invisible: they are what INTEGRATION.md ("Writes behind torch's back") asks the caller to declare with touch_params."""
import gc

import pytest
import torch
import torch.nn as nn


def P():
    from egaze_amd.hipops import packing
    return packing


def _conv():
    torch.manual_seed(0)
    return nn.Conv2d(4, 4, 3, padding=1)


def _new(p):
    return torch.randn(p.shape, generator=torch.Generator().manual_seed(7))


def _no_grad_add(m):
    with torch.no_grad():
        m.weight.add_(1.0)


def _no_grad_copy(m):
    with torch.no_grad():
        m.weight.copy_(_new(m.weight))


def _detach_add(m):
    m.weight.detach().add_(1.0)


def _load_state_dict(m):
    m.load_state_dict({"weight": _new(m.weight), "bias": _new(m.bias)})


def _state_dict_write(m):
    m.state_dict()["weight"].copy_(_new(m.weight))


def _init_normal(m):
    torch.nn.init.normal_(m.weight)


def _sgd_step(m):
    m.weight.grad = torch.ones_like(m.weight)
    torch.optim.SGD([m.weight], lr=0.5).step()


def _foreach_on_param(m):
    with torch.no_grad():
        torch._foreach_add_([m.weight], 1.0)


def _data_add(m):
    m.weight.data.add_(1.0)


def _data_copy(m):
    m.weight.data.copy_(_new(m.weight))


def _foreach_on_data(m):
    torch._foreach_add_([m.weight.data], 1.0)


def _data_assign(m):
    m.weight.data = _new(m.weight)


def _init_like_reference(m):
    from egaze_amd.utils import init_like_reference
    init_like_reference(m)


# route -> (write, delta of p._version, does _tag(p) change, do the values change)
ROUTES = {
    "no_grad-add_": (_no_grad_add, 1, True),
    "no_grad-copy_": (_no_grad_copy, 1, True),
    "detach-add_": (_detach_add, 1, True),
    "load_state_dict": (_load_state_dict, 1, True),
    "state_dict-write": (_state_dict_write, 1, True),
    "nn.init.normal_": (_init_normal, 1, True),
    "SGD.step": (_sgd_step, 1, True),
    "_foreach_add_-param": (_foreach_on_param, 1, True),
    "init_like_reference": (_init_like_reference, 1, True),
    # invisible to torch: same address, same version -- the caller declares them (touch_params / bump_weight_epoch)
    "data-add_": (_data_add, 0, False),
    "data-copy_": (_data_copy, 0, False),
    "_foreach_add_-data": (_foreach_on_data, 0, False),
    # a re-allocation: the version stays, the address moves
    "data-assign": (_data_assign, 0, True),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_version_counter_and_tag_per_route(route):
    p = P()
    write, dv, tag_moves = ROUTES[route]
    m = _conv()
    w = m.weight
    uid, tag, ver, before = p._uid(w), p._tag(w), w._version, w.detach().clone()
    write(m)
    assert m.weight is w and p._uid(w) == uid                   # the same live object keeps its identity
    assert not torch.equal(w.detach(), before)                  # (every route really changes the values)
    assert w._version - ver == dv
    assert (p._tag(w) != tag) == tag_moves
    if not tag_moves:
        # ... and the declared form of the same write is seen: per tensor, or wholesale
        p.touch_params([w])
        t1 = p._tag(w)
        assert t1 != tag
        epoch = p._WEIGHT_EPOCH[0]
        try:
            p.bump_weight_epoch()
            assert p._tag(w) != t1
        finally:
            p._WEIGHT_EPOCH[0] = epoch


def test_init_like_reference_moves_every_counter_it_writes_and_draws_as_before():
    """utils.init_like_reference on a module that already exists: every conv / BatchNorm / Linear parameter it rewrites gets a
    new tag, and the draws are the ones ``.data.normal_`` made (same generator state, same values)."""
    from egaze_amd.utils import init_like_reference
    p = P()
    m = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Flatten(), nn.Linear(8, 2))
    tags = {k: p._tag(v) for k, v in m.named_parameters()}
    torch.manual_seed(3)
    init_like_reference(m)
    for k, v in m.named_parameters():
        assert p._tag(v) != tags[k], k
    torch.manual_seed(3)
    want_conv = torch.empty(8, 3, 3, 3).normal_(0, (2.0 / (9 * 8)) ** 0.5)
    want_lin = torch.empty(2, 8).normal_(0, 0.01)
    assert torch.equal(m[0].weight.detach(), want_conv) and torch.equal(m[4].weight.detach(), want_lin)
    assert not m[0].bias.detach().any() and not m[4].bias.detach().any() and not m[1].bias.detach().any()
    assert torch.equal(m[1].weight.detach(), torch.ones(8))


def test_assign_gives_a_new_identity_and_the_old_entries_die_with_the_old_tensor():
    """load_state_dict(assign=True) replaces the Parameter object: a new uid (so no entry of the old one can be returned for
    it), and the finalizer of the old object drops its entries from _PACKED."""
    p = P()
    m = _conv()
    old = m.weight
    uid = p._uid(old)
    keys = [(uid, "fwd", 0), (uid, "dgrad_frag", 2)]
    other = (-7, "fwd", 0)
    saved = dict(p._PACKED)
    try:
        for k in keys + [other]:
            p._PACKED[k] = ("tag", None, None)
        m.load_state_dict({"weight": _new(old), "bias": _new(m.bias)}, assign=True)
        assert m.weight is not old
        assert p._uid(m.weight) != uid and p._uid(old) == uid
        assert all(k in p._PACKED for k in keys)                # the old tensor is alive: so are its entries
        del old
        gc.collect()
        assert not any(k[0] == uid for k in p._PACKED)
        assert other in p._PACKED                               # nobody else's
    finally:
        p._PACKED.clear()
        p._PACKED.update(saved)


def test_uids_are_never_reused():
    p = P()
    a = torch.zeros(4)
    ua = p._uid(a)
    del a
    gc.collect()
    b = torch.zeros(4)                                          # (may well get the freed address)
    assert p._uid(b) != ua and p._uid(b) == p._uid(b)
