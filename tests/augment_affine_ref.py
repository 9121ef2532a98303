"""Test-only numpy restatement of the affine resident gather (csrc/batch_gather.hip, egz_resident_gather_affine; DESIGN.md
section 21): the two further words of the draw (magnification g, angle theta), the fp32 matrices -- operation by operation on
np.float32, a polynomial sine and cosine, never np.sin / np.cos -- and the bilinear gather in integers (coordinates and flow vectors 64-bit).  Words 0 .. 4 and
the normalisation are tests/augment_ref.py's."""
import numpy as np

import augment_ref as A

F = np.float32
S1, S2, S3 = F(-1.6666654611e-1), F(8.3321608736e-3), F(-1.9515295891e-4)
C1, C2, C3 = F(4.166664568298827e-2), F(-1.388731625493765e-3), F(2.443315711809948e-5)
QUARTER_PI = F(np.pi / 4)
IDENTITY = A.IDENTITY + (F(1.0), F(0.0))
FLOW_MID, FLOW_BACK = 8355840, 547608330240               # 127.5 * 2^16, 127.5 * 2^32


def words(seed, epoch, sample):
    """The seven 64-bit words of a sample: the first five are augment_ref.words'."""
    key = A.mix(A.mix(A.mix(seed + A.GOLD) ^ (epoch & A.M64)) ^ (sample & A.M64))
    return [A.mix(key + (j + 1) * A.GOLD) for j in range(7)]


def rotate_rad(degrees):
    """Rr: the amplitude in radians, rounded once from fp64."""
    return F(float(degrees) * np.pi / 180.0)


def draw(seed, epoch, sample, flip_thr, shift, contrast, brightness, scale, rot_rad):
    """-> (flip, dy, dx, a, b, g, theta): augment_ref.draw's five, then g = fl(1 + fl(Sc t5)) and theta = fl(Rr t6)."""
    w = words(seed, epoch, sample)
    g = F(1.0) + F(scale) * A._unit(w[5])
    theta = F(rot_rad) * A._unit(w[6])
    return A.draw(seed, epoch, sample, flip_thr, shift, contrast, brightness) + (F(g), F(theta))


def sincos(theta):
    """(S, C) of the definition, every operation rounded to fp32 on its own."""
    t = F(theta)
    z = F(t * t)
    ps = F(F(F(F(S3 * z) + S2) * z) + S1)
    s = F(t + F(F(t * z) * ps))
    pc = F(F(F(F(C3 * z) + C2) * z) + C1)
    c = F(F(F(1.0) - F(F(0.5) * z)) + F(F(z * z) * pc))
    return s, c


def matrices(g, theta):
    """-> (M00, M01, A00, A10) Python ints in Q16: the inverse map for coordinates, the forward map for flow vectors."""
    g = F(g)
    s, c = sincos(theta)
    q = F(F(1.0) / g)
    k = F(65536.0)
    return (int(np.rint(F(F(q * c) * k))), int(np.rint(F(F(q * s) * k))),
            int(np.rint(F(F(g * c) * k))), int(np.rint(F(F(g * s) * k))))


def rows(params):
    """[(flip, dy, dx, a, b, g, theta), ...] -> the (B, 7) int32 layout of params_in / params_out."""
    out = np.empty((len(params), 7), dtype=np.int32)
    for i, p in enumerate(params):
        out[i, :3] = p[:3]
        out[i, 3:] = np.array(p[3:], dtype=np.float32).view(np.int32)
    return out


def unrows(table):
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    return [(int(r[0]), int(r[1]), int(r[2])) + tuple(r[3:].view(np.float32)) for r in table]


def draw_rows(seed, epoch, samples, flip_thr, shift, contrast, brightness, scale, rot_rad):
    return rows([draw(seed, epoch, int(s), flip_thr, shift, contrast, brightness, scale, rot_rad) for s in samples])


def source_q8(H, W, dy, dx, M00, M01):
    """-> (PY, PX) int64 (H, W): the source coordinate of every output pixel in the flipped frame, in 1/256 pixel."""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    X2, Y2 = 2 * (x - dx) - (W - 1), 2 * (y - dy) - (H - 1)
    XQ = M00 * X2 + M01 * Y2 + (W - 1) * 65536
    YQ = -M01 * X2 + M00 * Y2 + (H - 1) * 65536
    return (YQ + 256) >> 9, (XQ + 256) >> 9


def geometric(planes, flip, dy, dx, g, theta):
    """planes: (24, H, W) uint8 of one sample -> the augmented bytes (what ``raw`` carries)."""
    planes = np.asarray(planes)
    _, H, W = planes.shape
    M00, M01, A00, A10 = matrices(g, theta)
    PY, PX = source_q8(H, W, int(dy), int(dx), M00, M01)
    y0, fy, x0, fx = PY >> 8, PY & 255, PX >> 8, PX & 255
    src = planes
    if flip:
        src = planes[:, :, ::-1].copy()                   # F: column xc is read at W - 1 - xc ...
        src[A.FLOW_X, :, :] = 255 - src[A.FLOW_X, :, :]   # ... and an x-flow tap is 255 - byte
    src = np.ascontiguousarray(src).reshape(24, H * W)
    acc = np.zeros((24, H * W), dtype=np.int32)           # at most 65536 * 255
    for ty, tx, wgt in ((y0, x0, (256 - fx) * (256 - fy)), (y0, x0 + 1, fx * (256 - fy)),
                        (y0 + 1, x0, (256 - fx) * fy), (y0 + 1, x0 + 1, fx * fy)):
        tap = np.take(src, (np.clip(ty, 0, H - 1) * W + np.clip(tx, 0, W - 1)).ravel(), axis=1).astype(np.int32)
        inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        tap[23] *= inside.ravel()                         # a gaze map has no mass outside the picture
        acc += wgt.ravel().astype(np.int32) * tap
    out = ((acc + 32768) >> 16).reshape(24, H, W)
    cx = acc[3:23:2].astype(np.int64).reshape(10, H, W) - FLOW_MID
    cy = acc[4:23:2].astype(np.int64).reshape(10, H, W) - FLOW_MID
    out[3:23:2] = np.clip((A00 * cx - A10 * cy + FLOW_BACK + (1 << 31)) >> 32, 0, 255)
    out[4:23:2] = np.clip((A10 * cx + A00 * cy + FLOW_BACK + (1 << 31)) >> 32, 0, 255)
    return out.astype(np.uint8)


def batch(planes, params, mean, std):
    """planes: (B, 24, H, W) uint8 gathered bytes, params: B tuples of 7 -> (raw uint8 (B,24,H,W), fp32 (B,24,H,W))."""
    raw = np.stack([geometric(p, q[0], q[1], q[2], q[5], q[6]) for p, q in zip(planes, params)])
    out = np.stack([A.normalise(r, q[3], q[4], mean, std) for r, q in zip(raw, params)])
    return raw, out
