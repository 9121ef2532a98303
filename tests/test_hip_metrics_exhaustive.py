"""The AAE / AUC metric kernel (csrc/metrics.hip, egz_aae_auc) at EVERY one of the 224 x 224 centroids against scipy, at the
batch sizes and input forms the drivers use, across every level of its first-arg-max reduction, and on the predictions the
reference itself rejects.

The kernel never builds the filtered map: it argues that a delta through scipy's separable 'reflect' filter leaves at most
three non-zero terms per sample, replaces the count #{z > z[gp]} by a sort and 224 binary searches, and promises scipy's own
integer.  test_hip_metrics.py pins that on 14 maps; this module pins it on all 50,176 centres.

Top level imports numpy only: the scipy reference runs in spawned worker processes, which import this module to find their
function and must never import torch or the package (they would open the GPU).  Everything else is imported inside the tests.
"""
import math
import multiprocessing
import os
import sys
import time
import types

import numpy as np
import pytest

N = 224
NPIX = N * N
RADIUS = 56                       # int(4 * 14 + 0.5): scipy's truncate = 4 sigma
DIST = 112 / math.tan(math.pi / 6)
DEV = "cuda:0"
MAX_WORKERS = 16
CHUNK = 1024                      # maps per launch of the sweep (2 x 205 MB of device maps, built on the device)

# Worst |device AAE - host fp64 AAE| over the 250,880 maps of the sweep (exact centroids: only the atan2 / sqrt of the device
# maths library remain against the host's), measured on an MI355X:
# see profiles/metrics_exhaustive.txt.  The bar is 8 x that, for libm variation between ROCm versions.
AAE_WORST_MEASURED = 1.4210854715202004e-14
AAE_BAR = 8 * AAE_WORST_MEASURED


# ----------------------------------------------------------------------------- 1. the scipy reference table (host, workers)
def _ref_chunk(args):
    """Worker: numpy + scipy only.  The map exactly as oracle.egaze_oracle.compute_aae_auc builds it (utils.py:108-113)."""
    centres, gps = args
    from scipy import ndimage
    cnt = np.empty(gps.shape[:2], np.int64)
    zgp = np.empty(gps.shape[:2], np.float64)
    for n in range(len(centres)):
        z = np.zeros((224, 224))
        z[int(centres[n, 0])][int(centres[n, 1])] = 1
        z = ndimage.gaussian_filter(z, 14)
        z = z - z.min()
        z = z / z.max()
        for g in range(gps.shape[1]):
            i, j = int(gps[n, g, 0]), int(gps[n, g, 1])
            cnt[n, g] = (z > z[i][j]).sum()
            zgp[n, g] = z[i][j]
    return cnt, zgp, "torch" in sys.modules


def scipy_fp_counts(centres, gps, workers=MAX_WORKERS):
    """centres (M, 2) int, gps (M, G, 2) int -> (counts (M, G) int64, z[gp] (M, G) float64): for every centre the scipy map
    of a delta there, and #{z > z[gp]} for each of its gaze points.  At most 16 spawned workers, none of which sees torch."""
    centres = np.ascontiguousarray(centres, dtype=np.int64).reshape(-1, 2)
    gps = np.ascontiguousarray(gps, dtype=np.int64).reshape(len(centres), -1, 2)
    workers = max(1, min(MAX_WORKERS, workers, os.cpu_count() or 1, len(centres)))
    if workers == 1:
        cnt, zgp, _ = _ref_chunk((centres, gps))
        return cnt, zgp
    parts = np.array_split(np.arange(len(centres)), min(len(centres), workers * 8))
    # a spawned child re-imports the parent's __main__ (whatever started pytest, which may import torch): hand it an empty one,
    # so that a worker holds this module, numpy and scipy and nothing else
    main = sys.modules["__main__"]
    sys.modules["__main__"] = types.ModuleType("__main__")
    try:
        with multiprocessing.get_context("spawn").Pool(workers) as pool:
            out = pool.map(_ref_chunk, [(centres[p], gps[p]) for p in parts], chunksize=1)
    finally:
        sys.modules["__main__"] = main
    assert not any(o[2] for o in out), "a reference worker imported torch"
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _scipy_weights():
    x = np.arange(-RADIUS, RADIUS + 1)
    phi = np.exp(-0.5 / (14.0 * 14.0) * x ** 2)
    return phi / phi.sum()


def _line(c, v, gw):
    """The kernel's term order for a line that is v at index c and zero elsewhere (centre tap, then |k| = 56 .. 1, mirror
    multiplicity x value x weight), in numpy."""
    refl = lambda q: np.where(q < 0, -q - 1, np.where(q >= N, 2 * N - 1 - q, q))
    p = np.arange(N)
    tmp = ((p == c) * v) * gw[RADIUS]
    for ll in range(RADIUS, 0, -1):
        m = (refl(p + ll) == c).astype(np.float64) + (refl(p - ll) == c)
        tmp = tmp + (m * v) * gw[RADIUS + ll]
    return tmp


def test_reference_table_vs_oracle_host():
    """Host only: the worker function equals O.compute_aae_auc (count and gaze point) on centres at the corners and on both
    sides of every change of the mirror logic, the pool path equals the in-process path, and the numpy restatement of the
    kernel's term order equals scipy's filtered delta bit for bit there (a cross-check of the design, not the reference)."""
    from oracle import egaze_oracle as O
    rs = np.random.RandomState(5)
    cs = [(0, 0), (223, 223), (0, 223), (27, 28), (55, 56), (56, 55), (111, 112), (167, 168), (168, 167), (195, 196), (100, 3)]
    cs += [tuple(rs.randint(0, N, 2)) for _ in range(5)]
    centres = np.array(cs)
    gps = rs.randint(0, N, (len(cs), 3, 2))
    gps[:, 0] = centres                                             # the centre itself: count 0
    gps[:, 1] = np.clip(centres + rs.randint(-56, 57, centres.shape), 0, N - 1)
    cnt, zgp = scipy_fp_counts(centres, gps, workers=1)
    cnt2, zgp2 = scipy_fp_counts(centres, gps, workers=4)
    assert np.array_equal(cnt, cnt2) and np.array_equal(zgp, zgp2)
    inner = ((centres >= RADIUS) & (centres < N - RADIUS)).all(1)    # no mirror term reaches the centre: it is the maximum
    assert (cnt[inner, 0] == 0).all() and (zgp[inner, 0] == 1.0).all() and (zgp[:, 1] > 0).all()
    assert cnt[cs.index((100, 3)), 0] > 0      # near a border the direct and the mirrored tap add up to more NEXT to the centre
    from scipy import ndimage
    gw = _scipy_weights()
    for n, (ci, cj) in enumerate(cs):
        pred = np.zeros((N, N), np.float32)
        pred[ci, cj] = 1.0
        for g in range(3):
            tgt = np.zeros((N, N), np.float32)
            tgt[gps[n, g, 0], gps[n, g, 1]] = 1.0
            _, auc, gp = O.compute_aae_auc(pred, tgt)
            assert gp[0] == list(gps[n, g])
            assert cnt[n, g] == round((1 - auc) * NPIX), (ci, cj, g)
        z = np.zeros((N, N))
        z[ci][cj] = 1
        z = ndimage.gaussian_filter(z, 14)
        vrow = _line(ci, 1.0, gw)                                   # first pass, along axis 0
        mine = np.stack([_line(cj, vrow[i], gw) for i in range(N)])    # second pass, along axis 1
        assert np.array_equal(mine, z), (ci, cj)


# ----------------------------------------------------------------------------- 2. every centre, five gaze points
KINDS = ("centre", "uniform", "in-support", "57-away", "border")


def _sweep_cases():
    """For every centre (ci, cj): the two prediction pixels (mass 0.5 each; the same pixel twice = a single 1.0), the exact
    centroid, and five gaze points.  Fixed seed."""
    rs = np.random.RandomState(20240224)
    ci, cj = np.divmod(np.arange(NPIX), N)
    single = (ci + cj) % 2 == 0                                    # half the centres: one 1.0, integer centroid
    # the other half: 0.5 + 0.5 with the neighbour below, to the right or diagonal -- whichever fits, drawn where several do
    shape = rs.randint(0, 3, NPIX)                                 # 0 below, 1 right, 2 diagonal
    shape = np.where(ci == N - 1, 1, np.where(cj == N - 1, 0, shape))
    di = np.where(single, 0, (shape != 1).astype(np.int64))
    dj = np.where(single, 0, (shape != 0).astype(np.int64))
    assert ((ci + di < N) & (cj + dj < N)).all() and single.sum() == NPIX // 2
    cent = np.stack([ci + 0.5 * di, cj + 0.5 * dj], 1)             # exact in fp64 and in numpy's float32 sum
    gps = np.empty((NPIX, 5, 2), np.int64)
    gps[:, 0] = np.stack([ci, cj], 1)                              # (a) the centre
    gps[:, 1] = rs.randint(0, N, (NPIX, 2))                        # (b) uniform
    gps[:, 2, 0] = np.clip(ci + rs.randint(-56, 57, NPIX), 0, N - 1)   # (c) inside the support: z[gp] > 0
    gps[:, 2, 1] = np.clip(cj + rs.randint(-56, 57, NPIX), 0, N - 1)
    # (d) 57 away along one axis: z[gp] == 0.0.  224 > 2 * 57, so at least one of the four always fits.
    cand = np.stack([np.stack([ci + 57, cj], 1), np.stack([ci - 57, cj], 1), np.stack([ci, cj + 57], 1),
                     np.stack([ci, cj - 57], 1)], 1)               # (NPIX, 4, 2)
    ok = ((cand >= 0) & (cand < N)).all(2)
    assert ok.any(1).all()
    pick = np.argmax(ok * rs.uniform(0.5, 1.0, ok.shape), 1)       # a random one of those that fit
    gps[:, 3] = cand[np.arange(NPIX), pick]
    # (e) the nearest image-border pixel in the centre's row or column (ties: top, bottom, left, right)
    bcand = np.stack([np.stack([0 * ci, cj], 1), np.stack([0 * ci + N - 1, cj], 1), np.stack([ci, 0 * cj], 1),
                      np.stack([ci, 0 * cj + N - 1], 1)], 1)
    bpick = np.argmin(np.stack([ci, N - 1 - ci, cj, N - 1 - cj], 1), 1)
    gps[:, 4] = bcand[np.arange(NPIX), bpick]
    p1 = ci * N + cj
    p2 = (ci + di) * N + (cj + dj)
    return np.stack([ci, cj], 1), p1, p2, cent, single, gps


def _host_aae(cent, gp):
    """The reference's formula (utils.py:104-107) in fp64 on exact centroids; atan2 from the C library, one call per sample."""
    d = np.full(len(cent), DIST)
    r1 = np.stack([cent[:, 0] - 112, cent[:, 1] - 112, d], 1)
    r2 = np.stack([gp[:, 0] - 112.0, gp[:, 1] - 112.0, d], 1)
    cn = np.linalg.norm(np.cross(r1, r2), axis=1)
    dt = (r1 * r2).sum(1)
    return np.array([math.degrees(math.atan2(a, b)) for a, b in zip(cn.tolist(), dt.tolist())])


def _first(bad, centres, kind, *cols):
    idx = np.flatnonzero(bad)[:8]
    return [(tuple(centres[i]), KINDS[kind[i]]) + tuple(c[i].tolist() for c in cols) for i in idx]


@pytest.mark.gpu
def test_every_centre_five_gaze_points_vs_scipy(capsys):
    """All 50,176 centres x 5 gaze points = 250,880 maps.  fp count == scipy's integer, gaze point and centroid exact, AAE within
    AAE_BAR of the fp64 host formula, and exactly 0.0 where the gaze point is an integer centroid.

    Measured on an MI355X: worst |device AAE - host fp64 AAE| = 1.42e-14 deg (bar 8 x = 1.14e-13 deg); the host reference
    (50,176 scipy filters, 16 spawned workers) and the GPU part are timed in profiles/metrics_exhaustive.txt."""
    import torch
    import egaze_amd.hipops as H
    centres, p1, p2, cent, single, gps = _sweep_cases()
    assert len(np.unique(centres[:, 0] * N + centres[:, 1])) == NPIX           # every centre, once
    t0 = time.time()
    ref_cnt, ref_zgp = scipy_fp_counts(centres, gps)
    t_ref = time.time() - t0
    assert ref_cnt.shape == (NPIX, 5)
    # the cases are what they claim to be, by the reference's own map
    inner = ((centres >= RADIUS) & (centres < N - RADIUS)).all(1)
    assert (ref_zgp[inner, 0] == 1.0).all() and (ref_cnt[inner, 0] == 0).all()
    assert (ref_zgp[:, 2] > 0).all() and (ref_zgp[:, 3] == 0.0).all()
    # flat list of maps: sample s = 5 * centre + kind
    kind = np.tile(np.arange(5), NPIX)
    cidx = np.repeat(np.arange(NPIX), 5)
    gp_flat = gps.reshape(-1, 2)
    S = len(kind)
    assert S == 5 * NPIX and S % CHUNK == 0
    P1 = torch.from_numpy(p1[cidx]).to(DEV)
    P2 = torch.from_numpy(p2[cidx]).to(DEV)
    G = torch.from_numpy(gp_flat[:, 0] * N + gp_flat[:, 1]).to(DEV)
    rows = torch.arange(CHUNK, device=DEV)
    pred = torch.zeros(CHUNK, NPIX, device=DEV)
    tgt = torch.zeros(CHUNK, NPIX, device=DEV)
    res = torch.empty(S, 6, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    t0 = time.time()
    for s in range(0, S, CHUNK):
        pred.zero_(); tgt.zero_()
        pred[rows, P1[s:s + CHUNK]] = 0.5
        pred[rows, P2[s:s + CHUNK]] += 0.5                          # the same pixel again for the single-peak half: 1.0
        tgt[rows, G[s:s + CHUNK]] = 1.0
        res[s:s + CHUNK] = H.aae_auc(pred.view(CHUNK, N, N), tgt.view(CHUNK, N, N))
    res = res.cpu().numpy()
    t_gpu = time.time() - t0
    c_flat, cent_flat = centres[cidx], cent[cidx]

    bad = (res[:, 2] != gp_flat[:, 0]) | (res[:, 3] != gp_flat[:, 1])
    assert not bad.any(), ("gaze point", int(bad.sum()), _first(bad, c_flat, kind, res[:, 2:4], gp_flat))
    bad = (res[:, 4] != cent_flat[:, 0]) | (res[:, 5] != cent_flat[:, 1])
    assert not bad.any(), ("centroid", int(bad.sum()), _first(bad, c_flat, kind, res[:, 4:6], cent_flat))
    want = ref_cnt.reshape(-1)
    bad = res[:, 1] != want
    assert not bad.any(), ("fp count", int(bad.sum()), _first(bad, c_flat, kind, res[:, 1], want, gp_flat))
    host = _host_aae(cent_flat, gp_flat)
    diff = np.abs(res[:, 0] - host)
    worst = float(diff.max())
    with capsys.disabled():
        print(f"\n[metrics sweep] {S} maps, {NPIX} centres: worst |AAE device - host fp64| = {worst!r} deg at "
              f"{_first(diff == worst, c_flat, kind)[:1]}, bar {AAE_BAR!r}; host reference {t_ref:.1f} s "
              f"({min(MAX_WORKERS, os.cpu_count() or 1)} workers), GPU part {t_gpu:.1f} s")
    zero = single[cidx] & (kind == 0)
    assert zero.sum() == NPIX // 2
    bad = zero & (res[:, 0] != 0.0)
    assert not bad.any(), ("AAE at gp == integer centroid", int(bad.sum()), _first(bad, c_flat, kind, res[:, 0]))
    bad = ~(diff <= AAE_BAR)
    assert not bad.any(), ("AAE", int(bad.sum()), worst, _first(bad, c_flat, kind, res[:, 0], host))


# ----------------------------------------------------------------------------- 3. realistic maps, driver batch sizes and forms
BATCHES = (1, 32, 33, 64, 257)
CENTROID_BAR = 2 * NPIX * 2.0 ** -53 * 223        # two sums of <= 50176 non-negative fp64 terms each: 2.5e-9 px


def _realistic(B):
    """Sigmoid-like maps as test_hip_metrics.py builds them: a synth blob x 0.8 plus uniform noise; uint8 / 255 targets."""
    from oracle import synth
    rs = np.random.RandomState(1000 + B)
    gt = synth.synth_gt(B, N, rs)[:, 0]
    pred = synth.synth_gt(B, N, rs)[:, 0] * 0.8 + rs.uniform(0, 0.05, (B, N, N)).astype(np.float32)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)


def _exact_centroid(p):
    """math.fsum of the fp64 products i * p[i, j] (exact: a float32 times an integer below 2**8 has at most 32 bits)."""
    v = p.astype(np.float64)
    ii = np.arange(N, dtype=np.float64)
    t0 = math.fsum(v.ravel().tolist())
    t1 = math.fsum((v * ii[:, None]).ravel().tolist())
    t2 = math.fsum((v * ii[None, :]).ravel().tolist())
    return t1 / t0, t2 / t0


def _near_integer(c):
    return min(abs(c[0] - round(c[0])), abs(c[1] - round(c[1]))) < 1e-4


def test_realistic_seeds_have_no_ambiguous_centroid_host():
    """Host only: none of the 387 realistic samples has its exact centroid within 1e-4 px of an integer, where the reference's
    own int(com) (behind a float32 sum) would be ambiguous -- so the GPU test below excludes nothing from its count check."""
    for B in BATCHES:
        pred, _ = _realistic(B)
        assert not any(_near_integer(_exact_centroid(pred[b])) for b in range(B)), B


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_realistic_maps_three_input_forms_vs_oracle(B):
    """computeAAEAUC on (224,224), (B,224,224) and (B,1,224,224) device tensors against O.compute_aae_auc per sample: fp count,
    gaze point, AAE (1e-5 deg: the reference divides by its own float32 sum, see test_hip_metrics.py); the centroid against the
    exact sums within the derived 2.5e-9 px."""
    import torch
    import egaze_amd.hipops as H
    from egaze_amd.utils import computeAAEAUC
    from oracle import egaze_oracle as O
    pred, gt = _realistic(B)
    dp, dg = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    rows = H.aae_auc(dp, dg).cpu().numpy()
    excluded = 0
    aae_s, auc_s, gp_s = [], [], []
    for b in range(B):
        a_ref, auc_ref, gp_ref = O.compute_aae_auc(pred[b], gt[b])
        fp_ref = round((1 - auc_ref) * NPIX)
        a, auc, gp = computeAAEAUC(dp[b], dg[b])                    # the 2-D form, one sample at a time
        assert isinstance(a, float) and gp == [[int(gp_ref[0][0]), int(gp_ref[0][1])]], (b, gp, gp_ref)
        assert abs(a - a_ref) < 1e-5, (b, a, a_ref)
        exact = _exact_centroid(pred[b])
        assert abs(rows[b, 4] - exact[0]) <= CENTROID_BAR and abs(rows[b, 5] - exact[1]) <= CENTROID_BAR, (b, rows[b], exact)
        if _near_integer(exact):
            excluded += 1
        else:
            assert auc == 1 - float(fp_ref) / NPIX and rows[b, 1] == fp_ref, (b, rows[b], fp_ref)
        assert a == rows[b, 0] and gp[0] == [int(rows[b, 2]), int(rows[b, 3])]    # the batch launch computes the same sample
        aae_s.append(a); auc_s.append(auc); gp_s.append(gp[0])
    assert excluded == 0                                            # the seeds were chosen so; at most 1 % would be allowed
    m_ref = O.compute_aae_auc(pred, gt) if B > 1 else O.compute_aae_auc(pred[0], gt[0])
    for form in (dp, dp[:, None]):                                  # (B,224,224) and the drivers' (B,1,224,224)
        a, auc, gp = computeAAEAUC(form, dg if form.ndim == 3 else dg[:, None])
        assert gp == gp_s
        if B == 1:                                                  # squeezes to the single-image branch
            assert a == aae_s[0] and auc == auc_s[0]
        else:
            assert a == np.mean(aae_s) and auc == np.mean([1 - float(r[1]) / N / N for r in rows])
        assert abs(a - m_ref[0]) < 1e-5 and abs(auc - m_ref[1]) < 1e-12


@pytest.mark.gpu
def test_batch_permutation_and_repeat_bit_identical():
    """Samples do not see each other: permuting the batch permutes the rows bit for bit; two runs are bit-identical."""
    import torch
    import egaze_amd.hipops as H
    pred, gt = _realistic(257)
    dp, dg = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    r1 = H.aae_auc(dp, dg)
    r2 = H.aae_auc(dp, dg)
    assert torch.equal(r1, r2) and bool(torch.isfinite(r1).all())
    perm = torch.from_numpy(np.random.RandomState(8).permutation(257)).to(DEV)
    rp = H.aae_auc(dp[perm].contiguous(), dg[perm].contiguous())
    assert torch.equal(rp, r1[perm])
    assert torch.equal(H.aae_auc(dp[:64].contiguous(), dg[:64].contiguous()), r1[:64])
    assert torch.equal(H.aae_auc(dp[200:201].contiguous(), dg[200:201].contiguous()), r1[200:201])


# ----------------------------------------------------------------------------- 4. first arg-max across every reduction level
def _argmax_targets():
    """Targets whose maximum occurs twice or more.  The kernel gives quad q = idx // 4 to thread q % 1024 at loop step
    q // 1024, so pixel idx sits in thread (idx // 4) % 1024 (lane t % 64, wave t // 64) at step idx // 4096: an earlier pixel is
    never at a LATER step than a later pixel, but it can be in a higher lane or a later wave of an earlier or equal step."""
    rs = np.random.RandomState(77)
    sets = [(4095, 4096), (255, 256), (256, 4351), (255, 4351), (255, 4096), (255, 256, 4351), (0, NPIX - 1), (NPIX - 1,), (0,),
            (NPIX - 2, NPIX - 1), (4096 * 3 + 20, 4096 * 4 + 8), (4096 + 4, 8192), (7, 4096 * 11 + 7)]
    sets += [(4000 + a, 4000 + b) for a in range(4) for b in range(a + 1, 4)] + [(4000, 4001, 4002, 4003)]
    sets += [(4 * m + e, 4096 + e2) for m in (1, 2, 4, 8, 16, 32) for e, e2 in ((0, 0), (3, 1))]       # higher lane, each xor level
    sets += [(4 * 64 * w, 4096 + 4 * (64 * w - 1) + 3) for w in range(1, 16)]                          # later wave, each wave
    sets += [(4 * (64 * w + 63) + 3, 4096 * 5 + 4 * 64 * v) for w, v in ((15, 0), (9, 3), (1, 0))]
    sets += [tuple(sorted(rs.choice(NPIX, rs.randint(2, 6), replace=False))) for _ in range(150)]
    out = []
    for k, s in enumerate(sets):
        for bg in (0, 1):
            t = np.zeros(NPIX, np.float32) if bg == 0 else (rs.randint(0, 230, NPIX) / 255.0).astype(np.float32)
            t[list(s)] = 1.0 if k % 2 == 0 else np.float32(240 / 255.0)
            out.append(t)
    t = np.full(NPIX, 0.25, np.float32); out.append(t)                                   # all equal
    t = np.full(NPIX, -3.0, np.float32); out.append(t)                                   # all equal, negative
    t = -rs.uniform(1, 2, NPIX).astype(np.float32); t[[30000, 4095, 41000]] = -0.5; out.append(t)     # all negative, tied maximum
    t = -rs.uniform(1, 2, NPIX).astype(np.float32); out.append(t)                        # all negative, unique maximum
    t = np.full(NPIX, -0.0, np.float32); t[1000] = 0.0; out.append(t)                    # -0.0 == +0.0: the first of them
    t = np.full(NPIX, 0.0, np.float32); t[0] = -0.0; out.append(t)
    t = np.full(NPIX, -1.0, np.float32); t[9000] = 0.0; t[5000] = -0.0; out.append(t)
    t = np.full(NPIX, -1.0, np.float32); t[9000] = -0.0; t[5000] = 0.0; t[4096] = -2.0; out.append(t)
    t = rs.uniform(0, 1, NPIX).astype(np.float32); t[31337] = np.inf; out.append(t)      # +inf peak
    t = rs.uniform(0, 1, NPIX).astype(np.float32); t[[4351, 256]] = np.inf; out.append(t)
    return np.stack(out).reshape(-1, N, N)


@pytest.mark.gpu
def test_first_argmax_across_thread_lane_and_wave_levels():
    """gaze point == np.unravel_index(t.argmax(), t.shape) for tied maxima placed across the per-thread stride, every level of
    the shuffle tree and every pair of neighbouring waves; all-equal, all-negative, signed-zero and +inf targets."""
    import torch
    import egaze_amd.hipops as H
    tg = _argmax_targets()
    want = np.array([np.unravel_index(t.argmax(), t.shape) for t in tg])
    from oracle import synth
    pred = synth.synth_gt(1, N, np.random.RandomState(2))[0, 0] * 0.8 + 0.01
    dp = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pred.astype(np.float32), tg.shape))).to(DEV)
    res = H.aae_auc(dp, torch.from_numpy(tg).to(DEV)).cpu().numpy()
    bad = (res[:, 2] != want[:, 0]) | (res[:, 3] != want[:, 1])
    assert not bad.any(), [(int(i), res[i, 2:4].tolist(), want[i].tolist()) for i in np.flatnonzero(bad)[:8]]
    assert np.isfinite(res[:, :2]).all() and (res[:, 1] == np.round(res[:, 1])).all()


# ----------------------------------------------------------------------------- 5. predictions the reference itself rejects
@pytest.mark.gpu
def test_degenerate_predictions_are_refused_like_the_reference():
    """An all-zero prediction has a NaN centre of mass: the reference raises at int(nan).  A map with negative values can put the
    centroid outside the image: numpy then wraps a negative index or raises IndexError.  The kernel only ever compares the
    centroid (it addresses nothing with it), so it returns rows; the host half refuses them with a ValueError that names the
    sample, in every input form."""
    import torch
    from egaze_amd.utils import aae_auc_from_rows, aae_auc_rows, computeAAEAUC
    from oracle import egaze_oracle as O
    pred, gt = _realistic(3)
    zero = pred.copy(); zero[1] = 0.0
    with pytest.raises(ValueError):
        O.compute_aae_auc(zero[1], gt[1])                            # the reference: cannot convert float NaN to integer
    dz, dg = torch.from_numpy(zero).to(DEV), torch.from_numpy(gt).to(DEV)
    for o, t in ((dz, dg), (dz[:, None], dg[:, None])):
        with pytest.raises(ValueError, match="sample 1"):
            computeAAEAUC(o, t)
    with pytest.raises(ValueError, match="sample 0"):
        computeAAEAUC(dz[1], dg[1])
    rows, single = aae_auc_rows(dz, dg)
    rows = rows.cpu().numpy()
    assert not single and np.isnan(rows[1, 4:6]).all() and np.isfinite(rows[[0, 2]]).all()
    with pytest.raises(ValueError, match="sample 1"):
        aae_auc_from_rows(rows)
    assert aae_auc_from_rows(rows[[0, 2]])[2] == computeAAEAUC(dz[[0, 2]], dg[[0, 2]])[2]     # the others are still served
    # centroid row -180 (numpy would wrap it to row 44) and row 390 (numpy raises IndexError)
    low = np.zeros((N, N), np.float32); low[10, 10] = 1.0; low[200, 200] = -0.5
    high = np.zeros((N, N), np.float32); high[10, 10] = -0.5; high[200, 200] = 1.0
    for k, m in enumerate((low, high)):
        bad = pred.copy(); bad[2] = m
        r, _ = aae_auc_rows(torch.from_numpy(bad).to(DEV), dg)
        want = (10 - 100.0) / 0.5 if k == 0 else (200 - 5.0) / 0.5
        assert r[2, 4].item() == want and r[2, 5].item() == want
        with pytest.raises(ValueError, match="sample 2"):
            computeAAEAUC(torch.from_numpy(bad).to(DEV), dg)
    with pytest.raises(IndexError):
        O.compute_aae_auc(high, gt[0])
