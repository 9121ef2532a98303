"""The numpy restatement of egz_lstm_store (hipops.lstm_store): what extractLSTMw.channel_weight(feat, gt, size, align=False)
computes on the host, step by step, with every fp32 sum written out in the order ATen's CPU kernels take -- no np.sum, whose
pairwise order is another one.  test_lstm_handover_host checks it against torch on the CPU; test_hip_lstm_handover checks the
kernel against it."""
import math

import numpy as np

F32 = np.float32


def cell_scores(u8_plane, cell=16):
    """avg_pool2d(u8.float() / 255, cell) of one (H cell, W cell) uint8 plane -> (H, W) fp32: per cell s = 0.f, s += u / 255.f
    over its cell x cell bytes in row-major order, then s / (cell cell).  (Vectorised over the cells; the order inside a cell
    is the loop's.)"""
    u8_plane = np.asarray(u8_plane)
    assert u8_plane.dtype == np.uint8 and u8_plane.ndim == 2
    H, W = u8_plane.shape[0] // cell, u8_plane.shape[1] // cell
    unit = u8_plane.astype(F32) / F32(255.0)
    s = np.zeros((H, W), dtype=F32)
    for r in range(cell):
        for x in range(cell):
            s = s + unit[r:H * cell:cell, x:W * cell:cell]        # fp32 + fp32, one add per byte of the cell
    return s / F32(cell * cell)


def gaze_cell(u8_plane, cell=16):
    """The flat index of the FIRST maximum of cell_scores (torch.max's)."""
    s = cell_scores(u8_plane, cell).ravel()
    best = 0
    for k in range(1, s.size):
        if s[k] > s[best]:
            best = k
    return best


def window(ind, size, H):
    """extractLSTMw.var_window for the flat cell ``ind`` of an H x H map, in the kernel's arithmetic: fp32 clip (every value is
    a small multiple of 0.5), truncation of both bounds, both coordinates clipped with H."""
    half, up = F32(0.5) * F32(size), (size + 1) // 2
    out = []
    for f in (ind // H, ind % H):
        f = min(max(F32(f), half), F32(H - up))
        out += [int(f - half), int(f + F32(up))]
    return tuple(out)


def window_mean(feat_b, win):
    """feat_b (H, W, C) fp32 -> (C,): the sequential fp32 sum over the window in (y, x) order, one divide by the count."""
    y0, y1, x0, x1 = win
    s = np.zeros(feat_b.shape[2], dtype=F32)
    for y in range(y0, y1):
        for x in range(x0, x1):
            s = s + feat_b[y, x]
    return s / F32((y1 - y0) * (x1 - x0))


def store_rows(feat, planes, gt_src, dst, size, cell=16):
    """feat (B, H, H, C) fp32 channels-last; planes (Q, H cell, H cell) uint8; gt_src, dst (B,) -> ({row: (C,) vector}, cells):
    what the kernel writes into pool row dst[b], and the gaze cell of every sample (-1 where dst[b] == -1: skipped)."""
    feat = np.asarray(feat, dtype=F32)
    B, H = feat.shape[0], feat.shape[1]
    assert feat.shape[2] == H and 1 <= size <= H and math.ceil(size / 2) == (size + 1) // 2
    rows, cells = {}, np.full(B, -1, dtype=np.int32)
    for b in range(B):
        if dst[b] == -1:
            continue
        cells[b] = gaze_cell(planes[gt_src[b]], cell)
        rows[int(dst[b])] = window_mean(feat[b], window(int(cells[b]), size, H))
    return rows, cells


def corner_blobs(n, seed=0, hw=224, cell=16):
    """``n`` uint8 Gaussian blobs (sigma 5 .. 40) centred on a cell corner or the middle of a cell edge: several cells have the
    same exact integer sum, and which of them has the largest fp32 sum depends on the order of the additions."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:hw, 0:hw].astype(np.float64)
    out = np.empty((n, hw, hw), dtype=np.uint8)
    for i in range(n):
        cy = cell * rs.randint(1, hw // cell) - 0.5                 # between the last pixel of a cell and the first of the next
        cx = cell * rs.randint(1, hw // cell) - 0.5
        if i % 3 == 2:                                             # an edge centre: two cells tie, not four
            cx += cell / 2
        sigma = rs.uniform(5.0, 40.0)
        out[i] = (255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma ** 2))).astype(np.uint8)
    return out


def integer_sum_cell(u8_plane, cell=16):
    """The first-wins arg-max of the EXACT cell sums: the rule a kernel must not use."""
    H, W = u8_plane.shape[0] // cell, u8_plane.shape[1] // cell
    sums = u8_plane.astype(np.int64).reshape(H, cell, W, cell).sum(axis=(1, 3)).ravel()
    return int(np.argmax(sums))
