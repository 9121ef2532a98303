"""Test-only numpy restatement of the augmented resident gather (csrc/batch_gather.hip, egz_resident_gather_aug; DESIGN.md
section 20).  Two parts: the parameter draw -- a counter-based hash of (seed, epoch, sample number) in wrapping unsigned 64-bit
arithmetic, here on Python ints -- and its application to the 24 uint8 planes of a sample.  The fp32 steps are performed
operation by operation on np.float32 (one rounding each, no fused multiply-add), so the device tests can ask for equal bits."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
FLOW_X = tuple(range(3, 23, 2))                    # planes of the 24 that hold an x-flow: output flow channels 0, 2, ..., 18
IDENTITY = (0, 0, 0, np.float32(1.0), np.float32(0.0))


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words(seed, epoch, sample):
    """The five 64-bit words of a sample; ``sample`` is the dataset sample number, never the batch position."""
    key = mix(mix(mix(seed + GOLD) ^ (epoch & M64)) ^ (sample & M64))
    return [mix(key + (j + 1) * GOLD) for j in range(5)]


def flip_threshold(p):
    return int(np.floor(float(p) * 4294967296.0))


def _unit(word):
    """2 * (float32(word >> 40) * 2^-24) - 1: exact in fp32, in [-1, 1)."""
    return np.float32(2.0) * (np.float32(word >> 40) * np.float32(2.0 ** -24)) - np.float32(1.0)


def draw(seed, epoch, sample, flip_thr, shift, contrast, brightness):
    """-> (flip, dy, dx, a, b): ints and two np.float32 (gain, bias)."""
    w = words(seed, epoch, sample)
    flip = int((w[0] >> 32) < flip_thr)
    dy = (w[1] >> 32) % (2 * shift + 1) - shift
    dx = (w[2] >> 32) % (2 * shift + 1) - shift
    a = np.float32(1.0) + np.float32(contrast) * _unit(w[3])
    b = np.float32(brightness) * _unit(w[4])
    return flip, int(dy), int(dx), np.float32(a), np.float32(b)


def rows(params):
    """[(flip, dy, dx, a, b), ...] -> the (B, 5) int32 layout of params_in / params_out: flip, dy, dx, bits(a), bits(b)."""
    out = np.empty((len(params), 5), dtype=np.int32)
    for i, (flip, dy, dx, a, b) in enumerate(params):
        out[i, :3] = (flip, dy, dx)
        out[i, 3:] = np.array([a, b], dtype=np.float32).view(np.int32)
    return out


def unrows(table):
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    return [(int(r[0]), int(r[1]), int(r[2]), r[3:4].view(np.float32)[0], r[4:5].view(np.float32)[0]) for r in table]


def draw_rows(spec_seed, epoch, samples, flip_thr, shift, contrast, brightness):
    return rows([draw(spec_seed, epoch, int(s), flip_thr, shift, contrast, brightness) for s in samples])


def geometric(planes, flip, dy, dx):
    """planes: (24, H, W) uint8 of one sample (image 0:3, flow 3:23, ground truth 23) -> the augmented bytes (what ``raw``
    carries).  out(y, x) = F(y - dy, x - dx), F(y, x) = src(y, W - 1 - x if flip else x): colour and flow take the coordinate
    clamped to the frame, the ground truth is 0 outside it; an x-flow plane becomes 255 - byte under a flip."""
    planes = np.asarray(planes)
    _, H, W = planes.shape
    yy, xx = np.arange(H) - dy, np.arange(W) - dx
    ys, xs = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
    if flip:
        xs = W - 1 - xs
    out = planes[:, ys][:, :, xs].copy()
    inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
    out[23] = np.where(inside, out[23], 0)
    if flip:
        out[FLOW_X, :, :] = 255 - out[FLOW_X, :, :]
    return out


def normalise(u8, a, b, mean, std):
    """u8: (24, H, W) augmented bytes -> fp32 (24, H, W): u8 / 255, the photometric step on planes 0:3 only
    (min(max(fl(fl(a x) + b), 0), 1)), then (v - mean[c]) / std[c]."""
    x = u8.astype(np.float32) / np.float32(255.0)
    v = x.copy()
    v[:3] = np.minimum(np.maximum(np.float32(a) * x[:3] + np.float32(b), np.float32(0.0)), np.float32(1.0))
    m = np.asarray(mean, dtype=np.float32).reshape(24, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(24, 1, 1)
    return (v - m) / s


def batch(planes, params, mean, std):
    """planes: (B, 24, H, W) uint8 gathered bytes, params: B tuples -> (raw uint8 (B,24,H,W), fp32 (B,24,H,W))."""
    raw = np.stack([geometric(p, q[0], q[1], q[2]) for p, q in zip(planes, params)])
    out = np.stack([normalise(r, q[3], q[4], mean, std) for r, q in zip(raw, params)])
    return raw, out
