"""Writes tests/golden/jpeg_encode.npz: input pixels and the bytes Pillow's (libjpeg-turbo's default) encoder makes of them,
for tests/test_jpeg_enc_host.py and tests/test_hip_jpeg_encode.py.  Run from the repository root:
python tests/golden/make_golden_jpegenc.py

Grey inputs are (H, W); colour inputs are stored (H, W, 3) BGR, as hipops.heatmap_overlay returns them and cv2 takes them,
and turned to RGB for Pillow.  Colour files use Pillow's default sub-sampling, 4:2:0 (checked in SOF0 while generating)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_jpeg import content  # noqa: E402

OUT = os.path.join(HERE, "jpeg_encode.npz")


def pil_encode(arr, quality):
    """arr: (H, W) grey or (H, W, 3) BGR uint8 -> the file Image.save(format="JPEG", quality=quality) writes."""
    b = io.BytesIO()
    im = Image.fromarray(np.ascontiguousarray(arr[:, :, ::-1]) if arr.ndim == 3 else np.ascontiguousarray(arr))
    im.save(b, format="JPEG", quality=quality)
    data = b.getvalue()
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == (0x22 if arr.ndim == 3 else 0x11), hex(data[sof + 11])
    return data


def gaze_map(cx, cy, sigma=70.0, src=(960, 1280), out=(224, 224)):
    """A ground-truth gaze map in the geometry data/dataset_preprocessing.py renders: a sigma-70 Gaussian of the 960 x 1280
    gaze frame, min-max normalised to 0 .. 255 and area-averaged down to 224 x 224."""
    H, W = src
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))
    g = (g - g.min()) / (g.max() - g.min()) * 255.0
    ys = np.linspace(0, H, out[0] + 1)
    xs = np.linspace(0, W, out[1] + 1)
    m = np.empty(out)
    for i in range(out[0]):
        r = g[int(ys[i]):max(int(np.ceil(ys[i + 1])), int(ys[i]) + 1)].mean(0)
        for j in range(out[1]):
            m[i, j] = r[int(xs[j]):max(int(np.ceil(xs[j + 1])), int(xs[j]) + 1)].mean()
    return np.clip(np.rint(m), 0, 255).astype(np.uint8)


def jet_overlay(h, w, seed):
    """A JET heat map blended over a frame, as vis_features writes them (BGR)."""
    frame = content(h, w, seed)[:, :, ::-1].astype(np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.exp(-((x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2) / (2 * (0.2 * w) ** 2))
    r = np.clip(1.5 - np.abs(4 * v - 3), 0, 1)
    g = np.clip(1.5 - np.abs(4 * v - 2), 0, 1)
    b = np.clip(1.5 - np.abs(4 * v - 1), 0, 1)
    jet = np.stack([b, g, r], -1) * 255.0
    return np.clip(np.rint(0.5 * frame + 0.5 * jet), 0, 255).astype(np.uint8)


def noise(h, w, c, seed):
    shape = (h, w, 3) if c == 3 else (h, w)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def checker(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    a = (((x + y) & 1) * 255).astype(np.uint8)
    return np.stack([a, a, a], -1) if c == 3 else a


def cases():
    sizes = [(224, 224), (225, 223), (17, 31), (8, 8), (9, 2), (1, 1)]
    seed = 100
    for h, w in sizes:
        big = h * w > 10000                                # the two large geometries: one colour and two grey cases each
        for q in (95, 75) if big else (95, 75, 1):
            seed += 1
            bgr = np.ascontiguousarray(content(h, w, seed)[:, :, ::-1])
            yield f"gray_{h}x{w}_q{q}", bgr[..., 1].copy(), q
            if not big or q == 95:
                yield f"bgr_{h}x{w}_q{q}", bgr, q
    for q in (1, 50, 75, 95, 100):
        yield f"gray_noise_40x56_q{q}", noise(40, 56, 1, q), q
        yield f"bgr_noise_33x47_q{q}", noise(33, 47, 3, q + 7), q
    yield "gray_noise_224x224_q95", noise(224, 224, 1, 3), 95
    for v in (0, 128, 255):
        yield f"gray_flat{v}_24x40_q95", np.full((24, 40), v, np.uint8), 95
        yield f"bgr_flat{v}_24x40_q75", np.full((24, 40, 3), v, np.uint8), 75
    for name, px in (("blue", (255, 0, 0)), ("green", (0, 255, 0)), ("red", (0, 0, 255)), ("yellow", (0, 255, 255))):
        yield f"bgr_{name}_20x36_q95", np.tile(np.array(px, np.uint8), (20, 36, 1)), 95
    # half blue / half red: the largest chroma DC steps
    two = np.zeros((32, 48, 3), np.uint8)
    two[:, :24, 0] = 255
    two[:, 24:, 2] = 255
    yield "bgr_blue_red_32x48_q100", two, 100
    yield "gray_checker_64x64_q100", checker(64, 64, 1), 100
    yield "bgr_checker_41x27_q100", checker(41, 27, 3), 100
    yield "gray_gazemap_224x224_q95", gaze_map(700.3, 420.8), 95
    yield "gray_gazemap_corner_224x224_q95", gaze_map(3.0, 950.0), 95
    yield "bgr_jet_overlay_224x224_q95", jet_overlay(224, 224, 77), 95


def main():
    names, quals, hs, ws, cs, px, files = [], [], [], [], [], [], []
    for name, arr, q in cases():
        names.append(name); quals.append(q); hs.append(arr.shape[0]); ws.append(arr.shape[1])
        cs.append(3 if arr.ndim == 3 else 1)
        px.append(np.ascontiguousarray(arr).reshape(-1))
        files.append(np.frombuffer(pil_encode(arr, q), np.uint8))
    poff = np.concatenate([[0], np.cumsum([len(p) for p in px])]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    np.savez_compressed(OUT, names=np.array(names), quality=np.array(quals, np.int32), h=np.array(hs, np.int32),
                        w=np.array(ws, np.int32), channels=np.array(cs, np.int32), pixels=np.concatenate(px),
                        pixel_offsets=poff, files=np.concatenate(files), file_offsets=foff)
    print(f"{OUT}: {len(names)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
