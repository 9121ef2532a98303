"""The decoder's fused backward in the launch geometry bench.py times, against torch-CPU float64.

In the backward pass 11 of the 12 decoder convs of model_SP do not run the plain data gradient test_hip_ops.py pins: they run
hipops.conv3x3_dgrad_masked (the EPI_MASK_SUMS epilogue of csrc/conv3x3_igemm_x3s.hip), which applies the ReLU mask of the
block below, writes that block's bias-gradient partial rows (fp64, one per 128 pixels) and commits max |dx| to the abs-max
buffer that scales the next launch's f16 split; functions.ConvReLU.backward hands the three on as ``_egz_premasked``.  The
whole-model A/B (test_relu_backward_folded_into_dgrad_above) compares that path with the unfused one at batch 2, 64 x 64; here

  1. every distinct masked launch of the step (nine, derived from models/model_SP._DECODER_PLAN) runs at B = 32 on the route
     ConvReLU.backward takes, element-wise against fp64, with the mask, the stat rows, the abs-max and the unwritten-row
     hazard of the ``torch.empty`` stat buffer each pinned on its own;
  2. a three-block slice of the decoder runs through autograd at B = 32 with every switch at its default (streams, bias sums on
     the helper stream, split-K) against torch fp64 autograd;
  3. a gradient written in place between two blocks (a tensor hook) must drop the hand-over.

References are computed in float64 from the exact fp32 operands the kernels received.  Element-wise errors are
max |got - ref| / max |ref|.  The bias-gradient bar is held against the error of the smallest realistic defect, one dropped
128-pixel stat row, measured from the same fp64 data (chunk_defect): the defect must be at least 10x the bar."""
import gc
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 32

# (upsample-fused, dy channels K, dy size H, dx / mask_src channels C, dx size H'): the distinct masked data-gradient launches
# of the SP step at 224 x 224 (decoder.2 | .7 .9 | .14 .16 | .21 | .26 | .5 | .12 | .19 | .24)
MASKED_GEOMS = [(False, 512, 14, 512, 14), (False, 512, 28, 512, 28), (False, 256, 56, 256, 56), (False, 128, 112, 128, 112),
                (False, 64, 224, 64, 224), (True, 512, 28, 512, 14), (True, 256, 56, 512, 28), (True, 128, 112, 256, 56),
                (True, 64, 224, 128, 112)]

# element-wise bars of the data / weight gradients at this geometry (test_conv_ops_elementwise_at_the_headline_geometry)
DX_BAR3, DX_BAR2, DX_L2_BAR2 = 2e-5, 2e-3, 1e-3
# colsum_f64 of the stat rows against the fp64 column sums of the kernel's OWN fp32 dx: the reduction alone
# (test_hip_headline_ops.py: 3e-7, observed 4.9e-8 there; observed here <= 4.4e-8)
COLSUM_BAR = 3e-7
# ... and against the bias gradient of the fp64 reference, per backward arithmetic (products per MAC), from the nine geometries
# observed on MI355X (the figures are in test_masked_dgrad_at_batch_32).  Three products: 3.2e-6 .. 1.2e-5, bar 5x the worst.
# Two products: 1.9e-4 .. 2.4e-4 (the rounding noise of the 11-bit operand, the same at every size); 5x the worst would be
# 1.2e-3, which one dropped stat row of the 1.6 M-pixel launch (7.8e-3) does not exceed tenfold -- the bar is set TIGHTER, at a
# tenth of that defect (3.1x the worst observation), so that the test's own condition defect >= 10 bar holds for both.
DB_BAR = {3: 6e-5, 2: 7.5e-4}


def H():
    import egaze_amd.hipops as h
    return h


@pytest.fixture(autouse=True)
def cpu_threads():
    """fp64 references on at most 16 host threads; each geometry's tensors are freed before the next one."""
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        torch.set_num_threads(keep)
        gc.collect()
        torch.cuda.empty_cache()


def rel(got, ref):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def rel_l2(got, ref):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def chunk_defect(contrib, unit, ref):
    """Error max |d| / max |ref| that dropping ONE chunk of ``unit`` consecutive rows of the per-row contributions ``contrib``
    (rows, K) fp64 would cause -- the smallest over the first, a middle and the last chunk."""
    n = contrib.shape[0]
    starts = {0, (n // 2) // unit * unit, (n - unit) // unit * unit}
    scale = ref.abs().max().item()
    return min(contrib[s:s + unit].sum(0).abs().max().item() for s in starts) / scale


def dev_gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def decoder_masked_launches():
    """(ups, K, H, C, H') of the masked data-gradient launch of every decoder conv that sits on another ConvReLU block
    (utils.FusedSequential: ``relu_below``), from models/model_SP._DECODER_PLAN at 224 x 224."""
    from egaze_amd.models.model_SP import _DECODER_PLAN
    from egaze_amd.utils import cfg
    hh = 224 >> cfg['D'].count('M')                  # the encoders' output size
    out, ups, below = [], False, False
    for item in _DECODER_PLAN:
        if item == 'U':
            ups = True
            continue
        cin, cout = item
        hin, hh = hh, (2 * hh if ups else hh)
        if below:
            out.append((ups, cout, hh, cin, hin))
        ups, below = False, True
    return out


# ------------------------------------------------------------------------------------------------ 1. the masked data gradient
@pytest.mark.parametrize("ups,K,Hh,C,Hp", MASKED_GEOMS)
def test_masked_dgrad_at_batch_32(ups, K, Hh, C, Hp, monkeypatch):
    """hipops.conv3x3_dgrad_masked at B = 32 for each distinct launch of the step (plain, and upsample-fused where dx and
    mask_src are the LOW-res image), default SPLITK decision, three and two products per MAC.  mask_src is post-ReLU-like with
    one all-zero channel, one strictly positive channel, a few hundred -0.0 entries (masked, as torch's ``>`` does) and a few
    hundred 1e-40 subnormals (NOT masked); the truth of ``mask_src > 0`` is evaluated on the host copy.
      a. dx against fp64 conv2d_input (+ the 2 x 2 sum that is the backward of nearest upsampling) times the mask;
      b. the mask is exact: no non-zero dx where mask_src <= 0, dead channel all zero with a bias gradient of exactly 0.0,
         the subnormal positions pass;
      c. dx is bit-identical to the unfused launch (conv3x3_dgrad / conv3x3_ups_dgrad) times the mask wherever that launch
         is not split-K (conv3x3_ups_dgrad never is: the clause runs for every upsample-fused geometry);
      d. stat rows (ceil(M / 128), 2, C): colsum_f64 of plane 0 against the fp64 column sums of the kernel's own dx (the
         reduction alone) and against the reference's bias gradient, the latter held against one dropped stat row;
      e. no unwritten stat row: the launch runs once on a ``torch.empty`` buffer right after a NaN-filled block of the same
         size was freed, and once (the same C-ABI call) on test-owned NaN-filled dx / stat buffers -- both finite, identical;
      f. the committed abs-max equals max |dx| exactly.
    Observed on MI355X (three | two products; every geometry: clause c ran -- no unfused launch is split-K at B = 32 --, the
    poisoned block was reused, abs-max exact, colsum_f64 vs own dx 2.2e-8 .. 4.4e-8):
      plain 512@14 -> 512@14    (49 rows): dx 2.0e-6 | 1.9e-4 (L2 2.1e-4)  bias gradient 3.2e-6 | 1.9e-4  one stat row 1.3e-1
      plain 512@28 -> 512@28   (196 rows): dx 2.0e-6 | 2.1e-4 (L2 2.1e-4)  bias gradient 8.3e-6 | 2.0e-4  one stat row 7.2e-2
      plain 256@56 -> 256@56   (784 rows): dx 1.5e-6 | 2.4e-4 (L2 2.1e-4)  bias gradient 7.2e-6 | 2.0e-4  one stat row 3.3e-2
      plain 128@112 -> 128@112 (3136 rows): dx 1.0e-6 | 2.2e-4 (L2 2.1e-4)  bias gradient 9.8e-6 | 2.3e-4  one stat row 1.5e-2
      plain 64@224 -> 64@224  (12544 rows): dx 7.9e-7 | 2.2e-4 (L2 2.1e-4)  bias gradient 1.2e-5 | 2.4e-4  one stat row 7.8e-3
      ups 512@28 -> 512@14      (49 rows): dx 2.3e-6 | 2.1e-4 (L2 2.1e-4)  bias gradient 7.1e-6 | 2.4e-4  one stat row 1.3e-1
      ups 256@56 -> 512@28     (196 rows): dx 1.8e-6 | 2.3e-4 (L2 2.1e-4)  bias gradient 6.4e-6 | 2.1e-4  one stat row 6.9e-2
      ups 128@112 -> 256@56    (784 rows): dx 1.5e-6 | 2.2e-4 (L2 2.1e-4)  bias gradient 7.0e-6 | 1.9e-4  one stat row 2.8e-2
      ups 64@224 -> 128@112   (3136 rows): dx 1.3e-6 | 2.2e-4 (L2 2.1e-4)  bias gradient 6.9e-6 | 2.0e-4  one stat row 1.2e-2
    The three-product bias gradient is 3 - 15x further from fp64 than a sum of independent element errors of dx's size would be
    and grows with the pixel count: the element errors of the split-half data gradient share a small common-mode part.  It is
    the arithmetic of the unfused launch too (clause c: bit-identical)."""
    h = H()
    launches = decoder_masked_launches()
    assert len(launches) == 11 and len(MASKED_GEOMS) == 9 and sorted(set(launches)) == sorted(MASKED_GEOMS), launches
    g = dev_gen(1100 + 2 * Hh + K + ups)
    dead, alive = 3, 5
    mask = torch.randn(B, Hp, Hp, C, generator=g, device=DEV).clamp_(min=0)
    mask[..., dead] = 0.0
    mask[..., alive] = torch.rand(B, Hp, Hp, generator=g, device=DEV) + 0.5
    idx = torch.randint(0, mask.numel(), (800,), generator=g, device=DEV).unique()
    idx = idx[(idx % C != dead) & (idx % C != alive)]
    nz, sub = idx[0::2][:300], idx[1::2][:300]
    assert len(nz) >= 200 and len(sub) >= 200
    sub_bits = torch.tensor([1e-40], dtype=torch.float32).view(torch.int32).item()
    mask.view(-1).view(torch.int32)[nz] = -2 ** 31                 # -0.0 and the subnormal as bit patterns: no float pass
    mask.view(-1).view(torch.int32)[sub] = sub_bits                # on the way can round or flush them
    w = torch.randn(K, C, 3, 3, generator=g, device=DEV) * (2.0 / (9 * C)) ** 0.5
    dy = 1e-3 * torch.randn(B, Hh, Hh, K, generator=g, device=DEV)
    M = B * Hp * Hp
    rows = (M + 127) // 128

    # the truth of the mask, on the host copy of the fp32 values (no device flush-to-zero mode enters it)
    m_host = mask.cpu()
    gt0 = m_host > 0
    assert sub_bits != 0 and bool((m_host.view(-1)[sub.cpu()].view(torch.int32) == sub_bits).all())
    assert bool(gt0.view(-1)[sub.cpu()].all()) and not bool(gt0.view(-1)[nz.cpu()].any())
    assert bool(torch.signbit(m_host.view(-1)[nz.cpu()]).all())
    assert not bool(gt0[..., dead].any()) and bool(gt0[..., alive].all())
    gt0_d, le0_d = gt0.to(DEV), (m_host <= 0).to(DEV)

    ref = torch.nn.grad.conv2d_input((B, C, Hh, Hh), w.cpu().double(), dy.cpu().double().permute(0, 3, 1, 2), padding=1)
    if ups:
        ref = ref.view(B, C, Hp, 2, Hp, 2).sum((3, 5))
    masked_ref = (ref.permute(0, 2, 3, 1) * gt0).contiguous().view(M, C)
    del ref
    ref_sums = masked_ref.sum(0)
    defect = chunk_defect(masked_ref, 128, ref_sums)
    assert bool((masked_ref.view(-1)[sub.cpu()] != 0).all())

    dt = h.conv_dtype("dgrad", C, K, dy)
    wp, st = h.conv_weight(w, "ups_dgrad" if ups else "dgrad", dt, dy, C)
    assert dt == h.F16X3 and st
    ns = int(h.LIB.egz_conv3x3_streamed_splits(B, Hh, Hh, K, C))
    clause_c = bool(ups or not (h.SPLITK and ns > 1))

    fig, ok = {}, {}
    for products in (3, 2):
        monkeypatch.setattr(h, "BWD_PRODUCTS", products)
        # e. make garbage visible: the block the launch's torch.empty stat buffer is about to get holds NaN
        poison = torch.full((rows, 2, C), float("nan"), dtype=torch.float64, device=DEV)
        pptr = poison.data_ptr()
        del poison
        dx, stat, am = h.conv3x3_dgrad_masked(dy, wp, C, dt, mask, ups)
        reused = stat.data_ptr() == pptr
        assert tuple(stat.shape) == (rows, 2, C) and stat.dtype == torch.float64 and tuple(dx.shape) == (B, Hp, Hp, C)
        ok["stat finite"] = bool(torch.isfinite(stat[:, 0]).all())
        # ... and the same launch, with the arguments conv3x3_dgrad_masked passes, on NaN-filled buffers the test owns
        dx2, stat2 = torch.full_like(dx, float("nan")), torch.full_like(stat, float("nan"))
        am2 = h._new_absmax(dy.device)
        h.check(h.LIB.egz_conv3x3_fwd_streamed(dy.data_ptr(), wp.data_ptr(), None, dx2.data_ptr(), stat2.data_ptr(), B, Hh, Hh,
                                               K, C, h.EPI_MASK_SUMS, h._p2(dt), 1 if ups else 0, h.absmax_of(dy).data_ptr(),
                                               mask.data_ptr(), am2.data_ptr(), None, None, h._stream()), "masked dgrad")
        ok["stat finite (own buffer)"] = bool(torch.isfinite(stat2[:, 0]).all())
        ok["same launch"] = torch.equal(stat2[:, 0], stat[:, 0]) and torch.equal(dx2, dx) and float(h.absmax_value(am2)) == float(h.absmax_value(am))
        del dx2, stat2
        # a.
        dx64 = dx.cpu().double().view(M, C)
        e_dx, l2_dx = rel(dx64, masked_ref), rel_l2(dx64, masked_ref)
        # b.
        ok["masked entries zero"] = int(((dx != 0) & le0_d).sum()) == 0
        ok["dead channel zero"] = int((dx[..., dead] != 0).sum()) == 0
        db = h.colsum_f64(stat, C)
        ok["dead bias gradient 0.0"] = float(db[dead]) == 0.0
        ok["subnormals pass"] = bool((dx.view(-1)[sub] != 0).all())
        # c.
        if clause_c:
            plain = (h.conv3x3_ups_dgrad(dy, wp, C, dtype=dt, streamed=st) if ups
                     else h.conv3x3_dgrad(dy, wp, C, dtype=dt, streamed=st))
            ok["bit-identical to unfused * mask"] = torch.equal(dx, torch.where(gt0_d, plain, torch.zeros_like(plain)))
            del plain
        # d.
        e_red, e_db = rel(db, dx64.sum(0)), rel(db, ref_sums)
        # f.
        amv, dmax = float(h.absmax_value(am)), float(dx.abs().max())
        ok["abs-max exact"] = amv == dmax
        fig[products] = (e_dx, l2_dx, e_red, e_db)
        print(f"B=32 {'ups' if ups else 'plain'} dy {K}@{Hh} -> dx {C}@{Hp} ({rows} stat rows, {products} products): dx {e_dx:.1e} "
              f"(L2 {l2_dx:.1e})  colsum vs own dx {e_red:.1e}  bias gradient vs fp64 {e_db:.1e}  abs-max {amv:.6e} / {dmax:.6e}  | "
              f"clause c {'ran' if clause_c else f'skipped (unfused launch is split-K x{ns})'}, poisoned block "
              f"{'reused' if reused else 'not reused'}, one stat row {defect:.1e}  " + ("" if all(ok.values()) else f"FAILED {ok}"))
        del dx, stat, dx64
        assert all(ok.values()), (products, ok)
    (e3, _, r3, b3), (e2, l2, r2, b2) = fig[3], fig[2]
    assert e3 < DX_BAR3, e3
    assert e2 < DX_BAR2 and l2 < DX_L2_BAR2, (e2, l2)
    assert r3 < COLSUM_BAR and r2 < COLSUM_BAR, (r3, r2)
    assert b3 < DB_BAR[3] and b2 < DB_BAR[2], (b3, b2)
    assert defect >= 10 * DB_BAR[3] and defect >= 10 * DB_BAR[2], defect


# ------------------------------------------------------------------------------------------------ 2. the hand-over
def dyadic(shape, lo, hi, scale, g):
    """Integers lo .. hi times a power of two."""
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float() * scale


def test_decoder_slice_hand_over_at_batch_32():
    """decoder.9 (512 -> 512 @ 28) -> decoder.12 (upsample-fused 512 -> 256 @ 56) -> decoder.14 (256 -> 256 @ 56) through
    functions.ConvReLU.apply at B = 32, everything at its default (streams, BIAS_ON_HELPER, MASK_FUSE, SPLITK), loss =
    (out * g).sum() for a fixed random g; all three dW, all three db and dx against torch fp64 autograd (F.conv2d, F.relu,
    F.interpolate(nearest)) on the same operands.  The top block takes relu_bwd_bias, its data gradient and the middle block's
    produce the masked form, the middle and bottom blocks consume it: MASK_FUSE_STATS moves by 2 / 2.
    A ReLU decision that differs between the fp32-class forward pass and the fp64 one moves single entries of every gradient
    below it by O(1e-3) (one term of a 2304-term sum), and with 64 M activations and forward errors of 1e-7 some would.  The
    inputs, weights and biases therefore sit on a dyadic grid (small integers times a power of two): every forward sum is
    exact in both arithmetics (at most 2^20 grid steps, fp32 holds 2^24), so the test requires ZERO differing decisions; the
    gradient g and with it every backward operand is generic.
    Observed on MI355X: moved by 2 / 2, differing ReLU decisions 0 / 0 / 0 (forward error 0.0), dx 1.1e-6, dW 1.1e-6 / 1.0e-6 /
    1.2e-6, db 2.0e-6 / 8.5e-7 / 1.2e-7 (decoder.9 / .12 / .14)."""
    h = H()
    from egaze_amd.functions import ConvReLU
    g = dev_gen(1200)
    x = dyadic((B, 28, 28, 512), -2, 3, 1.0, g).clamp_(min=0).permute(0, 3, 1, 2).requires_grad_(True)
    ws = [dyadic((512, 512, 3, 3), -1, 1, 1.0 / 64, g), dyadic((256, 512, 3, 3), -1, 1, 1.0 / 64, g),
          dyadic((256, 256, 3, 3), -1, 1, 1.0 / 64, g)]
    bs = [dyadic((512,), -4, 4, 1.0 / 16, g), dyadic((256,), -4, 4, 1.0 / 16, g), dyadic((256,), -4, 4, 1.0 / 16, g)]
    for t in ws + bs:
        t.requires_grad_(True)
    gout = torch.randn(B, 56, 56, 256, generator=g, device=DEV).permute(0, 3, 1, 2)
    before = dict(h.MASK_FUSE_STATS)
    a1 = ConvReLU.apply(x, ws[0], bs[0], False, False)           # the first block of a chain: its input is not a ReLU output
    a2 = ConvReLU.apply(a1, ws[1], bs[1], True, True)
    a3 = ConvReLU.apply(a2, ws[2], bs[2], False, True)
    (a3 * gout).sum().backward()
    torch.cuda.synchronize()
    moved = {k: h.MASK_FUSE_STATS[k] - before[k] for k in before}

    xr = x.detach().cpu().double().requires_grad_(True)
    wr = [t.detach().cpu().double().requires_grad_(True) for t in ws]
    br = [t.detach().cpu().double().requires_grad_(True) for t in bs]
    r1 = F.relu(F.conv2d(xr, wr[0], br[0], padding=1))
    r2 = F.relu(F.conv2d(F.interpolate(r1, scale_factor=2, mode="nearest"), wr[1], br[1], padding=1))
    r3 = F.relu(F.conv2d(r2, wr[2], br[2], padding=1))
    (r3 * gout.cpu().double()).sum().backward()
    flips = [int(((a.detach().cpu() > 0) != (r.detach() > 0)).sum()) for a, r in ((a1, r1), (a2, r2), (a3, r3))]
    e = {"out": rel(a3, r3), "dx": rel(x.grad, xr.grad)}
    for i, name in enumerate(("9", "12", "14")):
        e[f"dW.{name}"], e[f"db.{name}"] = rel(ws[i].grad, wr[i].grad), rel(bs[i].grad, br[i].grad)
    print(f"B=32 decoder.9 -> .12 -> .14: MASK_FUSE_STATS moved by {moved}, differing ReLU decisions {flips}  "
          + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert moved == {"produced": 2, "consumed": 2}, moved
    assert flips == [0, 0, 0], flips
    for name, err in e.items():
        assert err < (DB_BAR[3] if name.startswith("db") else DX_BAR3), (name, err)


# ------------------------------------------------------------------------------------------------ 3. a stale hand-over
@pytest.mark.parametrize("hook", [None, "mul_", "add_"])
def test_premasked_gradient_written_in_place_is_dropped(hook):
    """Two chained ConvReLU blocks (B = 2, 16 x 16, 64 channels).  The upper block's data gradient carries the lower block's
    ReLU mask, bias-gradient stat rows and abs-max (``_egz_premasked``).  A tensor hook on the activation between them that
    writes the gradient in place (scaled by 2, or 1e-4 added: 10 % of its size) makes all three stale: the bias gradient
    would come from the old stat rows, the f16 split would be scaled with the old maximum, and the added constant would
    never be masked.  The lower block must then take its own ReLU-backward pass (MASK_FUSE_STATS['consumed'] does not move)
    and its weight, bias and input gradients match torch fp64 autograd with the same hook; without a hook the fused
    hand-over must still be taken.
    Observed on MI355X before functions.py stored the gradient's version beside the stat rows: consumed moved by 1 with either
    hook; mul_: db off by 5.0e-1; add_: dW 3.7e-1, db 7.4e-1, dx 1.0e-1.  With it: consumed moved
    by 0 with either hook and by 1 without; dW 4.4e-7 .. 5.4e-7, db 2.8e-7, dx 5.5e-7 in all three runs."""
    h = H()
    from egaze_amd.functions import ConvReLU
    g = dev_gen(1300)
    x = torch.randn(2, 16, 16, 64, generator=g, device=DEV).clamp_(min=0).permute(0, 3, 1, 2).requires_grad_(True)
    ws = [(torch.randn(64, 64, 3, 3, generator=g, device=DEV) * (2.0 / (9 * 64)) ** 0.5).requires_grad_(True) for _ in range(2)]
    bs = [(0.1 * torch.randn(64, generator=g, device=DEV)).requires_grad_(True) for _ in range(2)]
    gout = 1e-3 * torch.randn(2, 16, 16, 64, generator=g, device=DEV).permute(0, 3, 1, 2)

    def in_place(grad):
        if hook == "mul_":
            grad.mul_(2.0)
        elif hook == "add_":
            grad.add_(1e-4)

    before = dict(h.MASK_FUSE_STATS)
    a1 = ConvReLU.apply(x, ws[0], bs[0], False, False)
    if hook:
        a1.register_hook(in_place)
    a2 = ConvReLU.apply(a1, ws[1], bs[1], False, True)
    (a2 * gout).sum().backward()
    torch.cuda.synchronize()
    moved = {k: h.MASK_FUSE_STATS[k] - before[k] for k in before}

    xr = x.detach().cpu().double().requires_grad_(True)
    wr = [t.detach().cpu().double().requires_grad_(True) for t in ws]
    br = [t.detach().cpu().double().requires_grad_(True) for t in bs]
    r1 = F.relu(F.conv2d(xr, wr[0], br[0], padding=1))
    if hook:
        r1.register_hook(in_place)
    r2 = F.relu(F.conv2d(r1, wr[1], br[1], padding=1))
    (r2 * gout.cpu().double()).sum().backward()
    e = {"dW": rel(ws[0].grad, wr[0].grad), "db": rel(bs[0].grad, br[0].grad), "dx": rel(x.grad, xr.grad),
         "dW above": rel(ws[1].grad, wr[1].grad), "db above": rel(bs[1].grad, br[1].grad)}
    print(f"hook {hook}: MASK_FUSE_STATS moved by {moved}  " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert moved == {"produced": 1, "consumed": 0 if hook else 1}, moved
    for name, err in e.items():
        assert err < DX_BAR3, (name, err)
