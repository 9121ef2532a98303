"""Writes tests/golden/jpeg_decode.npz: JPEG streams encoded with Pillow and Pillow's (libjpeg-turbo's default) decode of each,
for tests/test_jpeg_host.py and tests/test_hip_jpeg.py.  Run from the repository root: python tests/golden/make_golden_jpeg.py

Expected outputs are uint8 (C, H, W) planes in BGR order for colour, as cv2.imread returns them; a grayscale decode of a
colour file is the Y plane (Image.draft("L"), libjpeg's JCS_GRAYSCALE), a colour decode of a grayscale file replicates it.
The progressive file and the PNG are kept apart with their host decodes: the GPU decoder does not take them."""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_decode.npz")


def content(h, w, seed):
    """Smooth gradients, a few sharp shapes and mild noise: every coefficient band is exercised, the decode compresses."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.empty((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.01, 0.08, 2).tolist() + [rng.uniform(0, 6.28)]
        im[..., c] = 128 + 90 * np.sin(fx * x + ph) * np.cos(fy * y)
    for _ in range(3):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, max(3, min(h, w) // 3))
        im[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = rng.integers(0, 256, 3)
    im += rng.normal(0, 3, im.shape)
    return np.clip(im, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", **kw)
    return b.getvalue()


def decode(data, channels):
    im = Image.open(io.BytesIO(data))
    if channels == 1:
        if im.mode != "L":
            im.draft("L", im.size)              # libjpeg JCS_GRAYSCALE at full scale: the Y plane
        a = np.asarray(im)
        assert im.mode == "L" and a.shape == (im.size[1], im.size[0]), (im.mode, a.shape)
        return a[None].copy()
    a = np.asarray(im.convert("RGB"))[:, :, ::-1]
    return a.transpose(2, 0, 1).copy()


def cases():
    plan = {(224, 224): ((95, ("gray", "420")), (50, ("gray", "444"))),
            (225, 223): ((75, ("gray", "422")), (100, ("420",))),
            (8, 8): ((75, ("gray", "444", "422", "420")), (100, ("gray", "444", "422", "420"))),
            (17, 31): ((75, ("gray", "444", "422", "420")), (100, ("gray", "444", "422", "420")))}
    seed = 0
    for (h, w), runs in plan.items():
        for q, kinds in runs:
            seed += 1
            rgb = content(h, w, seed)
            for k in kinds:
                if k == "gray":
                    yield f"gray_{h}x{w}_q{q}", encode(rgb[..., 0], quality=q), 1
                else:
                    yield f"c{k}_{h}x{w}_q{q}", encode(rgb, quality=q, subsampling=("444", "422", "420").index(k)), 3
    yield "gray_224_opt", encode(content(224, 224, 99)[..., 1], quality=90, optimize=True), 1
    yield "c420_64x80_opt", encode(content(64, 80, 98), quality=90, optimize=True, subsampling=2), 3
    yield "c422_61x45_opt_rst_blocks", encode(content(61, 45, 7), quality=85, subsampling=1, optimize=True,
                                              restart_marker_blocks=5), 3
    yield "c420_96x72_rst_rows", encode(content(96, 72, 9), quality=80, subsampling=2, restart_marker_rows=1), 3
    yield "gray_17x31_rst_blocks", encode(content(17, 31, 8)[..., 2], quality=75, restart_marker_blocks=1), 1
    yield "y_from_c420_225x223", encode(content(225, 223, 11), quality=95, subsampling=2), 1
    yield "y_from_c444_17x31", encode(content(17, 31, 12), quality=75, subsampling=0), 1
    yield "bgr_from_gray_45x61", encode(content(45, 61, 13)[..., 0], quality=95), 3
    # chroma rows of <= 2 samples: libjpeg's box upsampling instead of the fancy filter
    yield "c420_6x4_box", encode(content(6, 4, 14), quality=90, subsampling=2), 3
    yield "c422_5x3_box", encode(content(5, 3, 15), quality=90, subsampling=1), 3
    yield "c420_9x2_box", encode(content(9, 2, 16), quality=75, subsampling=2), 3


def main():
    names, streams, chans, hs, ws, exp = [], [], [], [], [], []
    for name, data, ch in cases():
        d = decode(data, ch)
        names.append(name); streams.append(np.frombuffer(data, np.uint8)); chans.append(ch)
        hs.append(d.shape[1]); ws.append(d.shape[2]); exp.append(d.reshape(-1))
    prog_rgb = content(224, 224, 21)
    prog = encode(prog_rgb, quality=90, progressive=True)
    gt = np.clip(content(224, 224, 22)[..., 0].astype(int) * 2 - 128, 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(gt).save(b, format="PNG")
    png = b.getvalue()
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.int64)
    np.savez_compressed(
        OUT, names=np.array(names), data=np.concatenate(streams), offsets=off, channels=np.array(chans, np.int32),
        h=np.array(hs, np.int32), w=np.array(ws, np.int32), expect=np.concatenate(exp), expect_offsets=eoff,
        progressive=np.frombuffer(prog, np.uint8), progressive_bgr=decode(prog, 3),
        png=np.frombuffer(png, np.uint8), png_gray=gt[None])
    print(f"{OUT}: {len(names)} streams, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
