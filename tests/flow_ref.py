"""Test-only numpy restatement of the dual TV-L1 optical flow that csrc/flow_tvl1.hip computes ("TV-L1 optical
flow"): Zach, Pock and Bischof (2007) in the form of Sanchez, Meinhardt-Llopis and Facciolo (IPOL 2013).  Every function takes
a ``dtype``: np.float64 is the yardstick of the accuracy tests; np.float32 performs the device's operations in the device's
order (one rounding per operation, no fused multiply-add), so the per-stage tests can ask for equal bits.

Images are (..., H, W) arrays; a run of F frames gives F - 1 pairs (pair i = frames i and i + 1)."""
import numpy as np

DEFAULTS = dict(tau=0.25, lam=0.15, theta=0.3, nscales=5, zfactor=0.5, warps=5, iterations=30)
PRESMOOTH_SIGMA = 0.8
MAX_LEVELS = 16          # of the pyramid, whatever nscales asks for ("at most 16 levels")


def gauss_weights(sigma, truncate=4.0):
    """scipy.ndimage's 1-D kernel (order 0), in fp64 -> (weights [2 R + 1], R)."""
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), radius


def pyramid_sigma(zfactor):
    return 0.6 * np.sqrt(zfactor ** -2 - 1.0)


def level_sizes(H, W, nscales, zfactor):
    """[(H, W), ...] from fine to coarse; nscales is clamped so that the coarsest level keeps 16 pixels per side, and to
    MAX_LEVELS levels."""
    sizes = [(int(H), int(W))]
    while len(sizes) < min(nscales, MAX_LEVELS):
        h, w = int(sizes[-1][0] * zfactor + 0.5), int(sizes[-1][1] * zfactor + 0.5)
        if h < 16 or w < 16:
            break
        sizes.append((h, w))
    return sizes


def gauss_filter(img, sigma, dtype):
    """Separable Gaussian, replicated border, axis -2 first (scipy's order), taps added from -R to R."""
    w64, R = gauss_weights(sigma)
    w = w64.astype(dtype)
    x = np.asarray(img).astype(dtype)
    for axis in (-2, -1):
        n = x.shape[axis]
        idx = np.arange(n)
        acc = np.zeros_like(x)
        for k in range(-R, R + 1):
            acc = acc + w[k + R] * np.take(x, np.clip(idx + k, 0, n - 1), axis=axis)
        x = acc
    return x


def cubic_weights(f, dtype):
    """Keys' bicubic convolution weights (a = -0.5) of the taps at -1, 0, 1, 2 for the fraction f."""
    A = dtype(-0.5)
    one, f1 = dtype(1), f + dtype(1)
    g = one - f
    w0 = ((A * f1 - dtype(5) * A) * f1 + dtype(8) * A) * f1 - dtype(4) * A
    w1 = ((A + dtype(2)) * f - (A + dtype(3))) * f * f + one
    w2 = ((A + dtype(2)) * g - (A + dtype(3))) * g * g + one
    w3 = one - w0 - w1 - w2
    return w0, w1, w2, w3


def sample_cubic(planes, py, px, dtype):
    """planes: list of (N, H, W) arrays sampled at the same positions py, px ((N, h, w) or (h, w), in dtype): the position
    is clamped to the image, the 4 x 4 tap indices likewise; rows are summed left to right, then top to bottom."""
    N, H, W = planes[0].shape
    py = np.minimum(np.maximum(py.astype(dtype), dtype(0)), dtype(H - 1))
    px = np.minimum(np.maximum(px.astype(dtype), dtype(0)), dtype(W - 1))
    fy0, fx0 = np.floor(py), np.floor(px)
    wy, wx = cubic_weights(py - fy0, dtype), cubic_weights(px - fx0, dtype)
    iy = np.broadcast_to(fy0.astype(np.int64), (N,) + py.shape[-2:])
    ix = np.broadcast_to(fx0.astype(np.int64), (N,) + px.shape[-2:])
    n = np.arange(N)[:, None, None]
    out = []
    for p in planes:
        acc = None
        for r in range(4):
            yy = np.clip(iy - 1 + r, 0, H - 1)
            row = None
            for c in range(4):
                v = wx[c] * p[n, yy, np.clip(ix - 1 + c, 0, W - 1)]
                row = v if row is None else row + v
            v = wy[r] * row
            acc = v if acc is None else acc + v
        out.append(acc.astype(dtype))
    return out


def resample(img, hd, wd, scale, dtype):
    """(N, hs, ws) -> (N, hd, wd): output (i, j) samples the source at ((i + 0.5) hs / hd - 0.5, (j + 0.5) ws / wd - 0.5);
    the result is multiplied by ``scale`` (1 for images, the size ratio for a flow component)."""
    _, hs, ws = img.shape
    half = dtype(0.5)
    py = (np.arange(hd).astype(dtype) + half) * dtype(hs) / dtype(hd) - half
    px = (np.arange(wd).astype(dtype) + half) * dtype(ws) / dtype(wd) - half
    out, = sample_cubic([img], np.broadcast_to(py[:, None], (hd, wd)), np.broadcast_to(px[None, :], (hd, wd)), dtype)
    return out * dtype(scale)


def pyramid_down(img, zfactor, dtype):
    _, H, W = img.shape
    return resample(gauss_filter(img, pyramid_sigma(zfactor), dtype), int(H * zfactor + 0.5), int(W * zfactor + 0.5), 1.0, dtype)


def grad_central(img, dtype):
    """Central differences with a replicated border -> (d/dx, d/dy)."""
    H, W = img.shape[-2:]
    j, i = np.arange(W), np.arange(H)
    gx = dtype(0.5) * (img[..., :, np.clip(j + 1, 0, W - 1)] - img[..., :, np.clip(j - 1, 0, W - 1)])
    gy = dtype(0.5) * (img[..., np.clip(i + 1, 0, H - 1), :] - img[..., np.clip(i - 1, 0, H - 1), :])
    return gx, gy


def warp(I0, I1, I1x, I1y, u1, u2, dtype):
    """-> (gx, gy, g2, rc): I1 and its gradient sampled at x + u, and the constant part of the residual."""
    _, H, W = I0.shape
    px = np.arange(W).astype(dtype)[None, None, :] + u1
    py = np.arange(H).astype(dtype)[None, :, None] + u2
    I1w, gx, gy = sample_cubic([I1, I1x, I1y], py, px, dtype)
    g2 = gx * gx + gy * gy
    rc = I1w - gx * u1 - gy * u2 - I0
    return gx, gy, g2, rc


def _div(px, py):
    """Backward differences with Chambolle's border rule (first: p[0]; last: -p[n - 2])."""
    dx = np.empty_like(px)
    dx[..., :, 0] = px[..., :, 0]
    dx[..., :, 1:-1] = px[..., :, 1:-1] - px[..., :, :-2]
    dx[..., :, -1] = -px[..., :, -2]
    dy = np.empty_like(py)
    dy[..., 0, :] = py[..., 0, :]
    dy[..., 1:-1, :] = py[..., 1:-1, :] - py[..., :-2, :]
    dy[..., -1, :] = -py[..., -2, :]
    return dx + dy


def _fwd(u):
    ux, uy = np.zeros_like(u), np.zeros_like(u)
    ux[..., :, :-1] = u[..., :, 1:] - u[..., :, :-1]
    uy[..., :-1, :] = u[..., 1:, :] - u[..., :-1, :]
    return ux, uy


def iterate(state, consts, n, lam, theta, tau, dtype):
    """n inner iterations.  state = (u1, u2, p11, p12, p21, p22), consts = (gx, gy, g2, rc) -> the new state."""
    u1, u2, p11, p12, p21, p22 = (np.array(a, dtype) for a in state)
    gx, gy, g2, rc = (np.asarray(a, dtype) for a in consts)
    lt, theta = dtype(lam) * dtype(theta), dtype(theta)
    t = dtype(tau) / theta
    thr = lt * g2
    big = g2 > dtype(1e-10)
    for _ in range(n):
        rho = rc + gx * u1 + gy * u2
        f = np.zeros_like(rho)
        np.divide(-rho, g2, out=f, where=big)
        lo, hi = rho < -thr, rho > thr
        d1 = np.where(lo, lt * gx, np.where(hi, -(lt * gx), f * gx))
        d2 = np.where(lo, lt * gy, np.where(hi, -(lt * gy), f * gy))
        u1 = (u1 + d1) + theta * _div(p11, p12)
        u2 = (u2 + d2) + theta * _div(p21, p22)
        ux, uy = _fwd(u1)
        den = dtype(1) + t * np.sqrt(ux * ux + uy * uy)
        p11, p12 = (p11 + t * ux) / den, (p12 + t * uy) / den
        ux, uy = _fwd(u2)
        den = dtype(1) + t * np.sqrt(ux * ux + uy * uy)
        p21, p22 = (p21 + t * ux) / den, (p22 + t * uy) / den
    return u1, u2, p11, p12, p21, p22


def build_pyramid(frames_u8, nscales, zfactor, dtype):
    """The presmoothed frames and their reductions, fine to coarse: the levels of level_sizes, so MAX_LEVELS at most."""
    pyr = [gauss_filter(frames_u8, PRESMOOTH_SIGMA, dtype)]
    for _ in level_sizes(*frames_u8.shape[-2:], nscales, zfactor)[1:]:
        pyr.append(pyramid_down(pyr[-1], zfactor, dtype))
    return pyr


def tvl1_flow(frames_u8, dtype=np.float64, tau=0.25, lam=0.15, theta=0.3, nscales=5, zfactor=0.5, warps=5, iterations=30):
    """(F, H, W) uint8 -> (u1, u2), each (F - 1, H, W): I1(x + u) ~ I0(x) for I0 = frame i, I1 = frame i + 1."""
    frames_u8 = np.asarray(frames_u8)
    pyr = build_pyramid(frames_u8, nscales, zfactor, dtype)
    u1 = u2 = None
    for lvl in range(len(pyr) - 1, -1, -1):
        img = pyr[lvl]
        I0, I1 = img[:-1], img[1:]
        h, w = img.shape[-2:]
        if u1 is None:
            u1, u2 = np.zeros(I0.shape, dtype), np.zeros(I0.shape, dtype)
        else:
            hc, wc = u1.shape[-2:]
            u1 = resample(u1, h, w, dtype(w) / dtype(wc), dtype)
            u2 = resample(u2, h, w, dtype(h) / dtype(hc), dtype)
        I1x, I1y = grad_central(I1, dtype)
        p = [np.zeros(I0.shape, dtype) for _ in range(4)]
        for _ in range(warps):
            consts = warp(I0, I1, I1x, I1y, u1, u2, dtype)
            u1, u2, *p = iterate((u1, u2, *p), consts, iterations, lam, theta, tau, dtype)
    return u1, u2


def bgr_to_gray(frames_hwc):
    """OpenCV's 8-bit fixed-point rule on (..., 3) BGR bytes."""
    x = np.asarray(frames_hwc).astype(np.int64)
    return ((4899 * x[..., 2] + 9617 * x[..., 1] + 1868 * x[..., 0] + 8192) >> 14).astype(np.uint8)


def flow_to_u8(v, bound=20.0):
    v = np.asarray(v).astype(np.float64)
    q = np.rint(255.0 * (v + bound) / (2.0 * bound))          # half to even
    return np.where(v > bound, 255, np.where(v < -bound, 0, q)).astype(np.uint8)


def texture(H, W, shift=(0.0, 0.0), seed=0, nwaves=24, fmax=0.35):
    """Analytic texture T(x - sx, y - sy) as uint8: a sum of sinusoids with |frequency| <= fmax rad/px.  texture(shift=0) and
    texture(shift=(sx, sy)) are a frame pair whose true flow is the constant (sx, sy)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, nwaves)
    mag = rng.uniform(0.05, fmax, nwaves)
    ph = rng.uniform(0, 2 * np.pi, nwaves)
    amp = rng.uniform(0.5, 1.0, nwaves)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    t = sum(a * np.sin(m * np.cos(g) * x + m * np.sin(g) * y + p) for a, m, g, p in zip(amp, mag, ang, ph))
    t = 127.5 + t * (100.0 / amp.sum())
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def endpoint_error(u1, u2, shift, trim=8):
    e = np.hypot(u1 - shift[0], u2 - shift[1])[..., trim:-trim, trim:-trim]
    return float(e.mean()), float(e.max())
