// Dual TV-L1 optical flow (Zach, Pock, Bischof 2007, in the form of Sanchez, Meinhardt-Llopis, Facciolo, IPOL 2013): the producer of
// the flow_x / flow_y images the temporal stream reads (data/extract_flow.py).  DESIGN.md "TV-L1 optical flow" is the definition;
// tests/flow_ref.py restates it in numpy.  A batch is a run of F = N + 1 grey planes; pair i is planes i and i + 1.
//
//   grey -> Gaussian (sigma 0.8) -> pyramid (Gaussian + bicubic) -> per level, coarse to fine: central gradient of I1, then
//   `warps` times { warp: I1, dI1 sampled at x + u -> gx gy g2 rc;  `iterations` times { u from p;  p from u } }
//
// The inner solver is the hot path.  tvl1_tile_kernel runs K iterations per launch on a (T + 2K)^2 region per block: every
// thread owns Q pixels of the region and keeps their six state values and four constants in registers; LDS holds the six
// state planes only for the neighbour exchange (p one pixel left / up, u one pixel right / down).  An iteration makes what
// lies within one pixel of the region's edge stale, so after K iterations exactly the inner T x T is still right, and that is
// what the block writes.  The image-border rules are taken from image coordinates, never from the tile.  tvl1_iter1_kernel is
// the one-iteration-per-launch form on global memory (k = 1), the yardstick the tiled form must equal bit for bit: both call
// tvl1_u_step / tvl1_p_step, and contraction is off for the file, so each operation below is one IEEE operation in both.
#include "egz_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int MAX_R = 16;            // Gaussian tap radius
constexpr int MAX_LEVELS = 16;       // of the pyramid, part of the definition: hipops.FLOW_MAX_LEVELS, tests/flow_ref.py MAX_LEVELS

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------ small kernels
__global__ __launch_bounds__(NT) void gray_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                  long n, long plane, int planar) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    int b, g, r;
    if (planar) {
        const long f = i / plane, p = i - f * plane;
        const unsigned char* s = src + f * 3 * plane + p;
        b = s[0]; g = s[plane]; r = s[2 * plane];
    } else {
        b = src[3 * i]; g = src[3 * i + 1]; r = src[3 * i + 2];
    }
    dst[i] = (unsigned char)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14);
}

// One axis of the separable Gaussian, replicated border, taps added from -R to R.  vertical: along H, else along W.
template <typename TI>
__global__ __launch_bounds__(NT) void gauss_kernel(const TI* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                   const float* __restrict__ gw, int R, int vertical) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const long base = (long)blockIdx.z * H * W;
    float acc = 0.f;
    for (int k = -R; k <= R; ++k) {
        const int y = vertical ? clampi(i + k, 0, H - 1) : i, x = vertical ? j : clampi(j + k, 0, W - 1);
        acc = acc + gw[k + R] * (float)src[base + (long)y * W + x];
    }
    dst[base + (long)i * W + j] = acc;
}

// Keys' bicubic convolution, a = -0.5: weights of the taps at -1, 0, 1, 2 for the fraction f.
__device__ __forceinline__ void cubic_weights(float f, float w[4]) {
    const float A = -0.5f, f1 = f + 1.f, g = 1.f - f;
    w[0] = ((A * f1 - 5.f * A) * f1 + 8.f * A) * f1 - 4.f * A;
    w[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
    w[2] = ((A + 2.f) * g - (A + 3.f)) * g * g + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

struct CubicTaps {
    float wy[4], wx[4];
    int y[4], x[4];
};

// position clamped to the image, tap indices likewise
__device__ __forceinline__ CubicTaps cubic_taps(float py, float px, int H, int W) {
    CubicTaps t;
    py = fminf(fmaxf(py, 0.f), (float)(H - 1));
    px = fminf(fmaxf(px, 0.f), (float)(W - 1));
    const float fy = floorf(py), fx = floorf(px);
    cubic_weights(py - fy, t.wy);
    cubic_weights(px - fx, t.wx);
    const int iy = (int)fy, ix = (int)fx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.y[k] = clampi(iy - 1 + k, 0, H - 1);
        t.x[k] = clampi(ix - 1 + k, 0, W - 1);
    }
    return t;
}

// rows summed left to right, then top to bottom
__device__ __forceinline__ float cubic_sample(const float* __restrict__ p, int W, const CubicTaps& t) {
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float* row = p + (long)t.y[r] * W;
        float s = t.wx[0] * row[t.x[0]];
#pragma unroll
        for (int c = 1; c < 4; ++c) s = s + t.wx[c] * row[t.x[c]];
        acc = r == 0 ? t.wy[0] * s : acc + t.wy[r] * s;
    }
    return acc;
}

// (planes, hs, ws) -> (planes, hd, wd), times `scale`
__global__ __launch_bounds__(NT) void resample_kernel(const float* __restrict__ src, float* __restrict__ dst, int hs, int ws,
                                                      int hd, int wd, float scale) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= wd) return;
    const float py = ((float)i + 0.5f) * (float)hs / (float)hd - 0.5f;
    const float px = ((float)j + 0.5f) * (float)ws / (float)wd - 0.5f;
    const CubicTaps t = cubic_taps(py, px, hs, ws);
    dst[((long)blockIdx.z * hd + i) * wd + j] = cubic_sample(src + (long)blockIdx.z * hs * ws, ws, t) * scale;
}

__global__ __launch_bounds__(NT) void grad_kernel(const float* __restrict__ img, float* __restrict__ gx, float* __restrict__ gy,
                                                  int H, int W) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const float* p = img + (long)blockIdx.z * H * W;
    const long o = (long)blockIdx.z * H * W + (long)i * W + j;
    gx[o] = 0.5f * (p[(long)i * W + min(j + 1, W - 1)] - p[(long)i * W + max(j - 1, 0)]);
    gy[o] = 0.5f * (p[(long)min(i + 1, H - 1) * W + j] - p[(long)max(i - 1, 0) * W + j]);
}

// img: (N + 1) planes (pair n: I0 = plane n, I1 = plane n + 1); i1x, i1y: the gradient of planes 1 .. N (N planes);
// u: planes u1, u2 of the state (plane stride `ps` = N H W); c: gx, gy, g2, rc with the same plane stride.
__global__ __launch_bounds__(NT) void warp_kernel(const float* __restrict__ img, const float* __restrict__ i1x,
                                                  const float* __restrict__ i1y, const float* __restrict__ u,
                                                  float* __restrict__ c, int H, int W, long ps) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const long hw = (long)H * W, o = (long)blockIdx.z * hw + (long)i * W + j;
    const float u1 = u[o], u2 = u[ps + o];
    const CubicTaps t = cubic_taps((float)i + u2, (float)j + u1, H, W);
    const float i1w = cubic_sample(img + (long)(blockIdx.z + 1) * hw, W, t);
    const float gx = cubic_sample(i1x + (long)blockIdx.z * hw, W, t);
    const float gy = cubic_sample(i1y + (long)blockIdx.z * hw, W, t);
    c[o] = gx;
    c[ps + o] = gy;
    c[2 * ps + o] = gx * gx + gy * gy;
    c[3 * ps + o] = i1w - gx * u1 - gy * u2 - img[o];
}

__global__ __launch_bounds__(NT) void quant_kernel(const float* __restrict__ v, unsigned char* __restrict__ out, long n,
                                                   double bound) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const double x = (double)v[i];
    unsigned char q;
    if (x > bound) q = 255;
    else if (x < -bound) q = 0;
    else q = (unsigned char)__builtin_rint(255.0 * (x + bound) / (2.0 * bound));       // half to even
    out[i] = q;
}

// ------------------------------------------------------------------------------------------------ the iteration body
struct Tvl1Par {
    float lt, theta, t;              // lambda * theta, theta, tau / theta
};

// Chambolle's backward difference: first p[0], last -p[n - 2]
__device__ __forceinline__ float bdiff(float c, float prev, bool first, bool last) {
    return first ? c : (last ? -prev : c - prev);
}

// u <- u + threshold step + theta div(p), for one component pair at once.  pXc: p at the pixel, pXl / pXu: one left / up.
__device__ __forceinline__ void tvl1_u_step(float gx, float gy, float g2, float rc, float& u1, float& u2, float p11c, float p11l,
                                            float p12c, float p12u, float p21c, float p21l, float p22c, float p22u,
                                            bool fc, bool lc, bool fr, bool lr, const Tvl1Par& q) {
    const float rho = rc + gx * u1 + gy * u2;
    const float thr = q.lt * g2;
    float d1, d2;
    if (rho < -thr) {
        d1 = q.lt * gx; d2 = q.lt * gy;
    } else if (rho > thr) {
        d1 = -(q.lt * gx); d2 = -(q.lt * gy);
    } else {
        const float f = g2 > 1e-10f ? -rho / g2 : 0.f;
        d1 = f * gx; d2 = f * gy;
    }
    const float div1 = bdiff(p11c, p11l, fc, lc) + bdiff(p12c, p12u, fr, lr);
    const float div2 = bdiff(p21c, p21l, fc, lc) + bdiff(p22c, p22u, fr, lr);
    u1 = (u1 + d1) + q.theta * div1;
    u2 = (u2 + d2) + q.theta * div2;
}

// p <- (p + t grad u) / (1 + t |grad u|), forward differences (0 in the last column / row).  uc, ur, ud: the new u here, right, below.
__device__ __forceinline__ void tvl1_p_step(float uc, float ur, float ud, bool lc, bool lr, float& px, float& py,
                                            const Tvl1Par& q) {
    const float ux = lc ? 0.f : ur - uc, uy = lr ? 0.f : ud - uc;
    const float den = 1.f + q.t * sqrtf(ux * ux + uy * uy);
    px = (px + q.t * ux) / den;
    py = (py + q.t * uy) / den;
}

// ------------------------------------------------------------------------------------------------ k = 1: one launch per iteration
// State planes (stride ps): u1 u2 p11 p12 p21 p22; constants: gx gy g2 rc.  Reads `in`, writes `out` (never the same buffer).
__device__ __forceinline__ void u_at(const float* __restrict__ in, const float* __restrict__ c, long ps, long o, int i, int j,
                                     int H, int W, const Tvl1Par& q, float& u1, float& u2) {
    u1 = in[o];
    u2 = in[ps + o];
    const long l = j > 0 ? o - 1 : o, up = i > 0 ? o - W : o;
    tvl1_u_step(c[o], c[ps + o], c[2 * ps + o], c[3 * ps + o], u1, u2, in[2 * ps + o], in[2 * ps + l], in[3 * ps + o],
                in[3 * ps + up], in[4 * ps + o], in[4 * ps + l], in[5 * ps + o], in[5 * ps + up], j == 0, j == W - 1, i == 0,
                i == H - 1, q);
}

__global__ __launch_bounds__(NT) void tvl1_iter1_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const float* __restrict__ c, int H, int W, long ps, Tvl1Par q) {
    const int j = blockIdx.x * NT + threadIdx.x, i = blockIdx.y;
    if (j >= W) return;
    const long o = (long)blockIdx.z * H * W + (long)i * W + j;
    const bool lc = j == W - 1, lr = i == H - 1;
    float u1, u2, u1r = 0.f, u2r = 0.f, u1d = 0.f, u2d = 0.f;
    u_at(in, c, ps, o, i, j, H, W, q, u1, u2);
    if (!lc) u_at(in, c, ps, o + 1, i, j + 1, H, W, q, u1r, u2r);
    if (!lr) u_at(in, c, ps, o + W, i + 1, j, H, W, q, u1d, u2d);
    float p11 = in[2 * ps + o], p12 = in[3 * ps + o], p21 = in[4 * ps + o], p22 = in[5 * ps + o];
    tvl1_p_step(u1, u1r, u1d, lc, lr, p11, p12, q);
    tvl1_p_step(u2, u2r, u2d, lc, lr, p21, p22, q);
    out[o] = u1; out[ps + o] = u2;
    out[2 * ps + o] = p11; out[3 * ps + o] = p12; out[4 * ps + o] = p21; out[5 * ps + o] = p22;
}

// ------------------------------------------------------------------------------------------------ k > 1: overlapped tiles
// Block (bx, by, n) owns output tile [by T, by T + T) x [bx T, bx T + T) of pair n and works on the region grown by K on every
// side (E = T + 2K per side).  Region pixel idx = tid + NT q (q < Q) belongs to thread tid.  Pixels of the region outside the
// image hold zeros and are computed like any other; no pixel of the image ever reads them (the border rules below come from the
// image coordinates).  A neighbour index that would leave the region is replaced by the pixel's own: the value is wrong, and
// it is one of those the halo is there to absorb.
enum { F_FC = 1, F_LC = 2, F_FR = 4, F_LR = 8, F_IN = 16, F_L = 32, F_U = 64, F_R = 128, F_D = 256, F_OUT = 512 };

template <int T, int K>
__global__ __launch_bounds__(NT) void tvl1_tile_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       const float* __restrict__ c, int H, int W, long ps, int niter,
                                                       Tvl1Par q) {
    constexpr int E = T + 2 * K, NPIX = E * E, Q = (NPIX + NT - 1) / NT;
    __shared__ float lds[6][NPIX];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * T - K, y0 = blockIdx.y * T - K;
    const long base = (long)blockIdx.z * H * W;

    float s[Q][6], k[Q][4];
    int flag[Q];
    long off[Q];
#pragma unroll
    for (int e = 0; e < Q; ++e) {
        const int idx = tid + NT * e, ly = idx / E, lx = idx - ly * E;
        const int y = y0 + ly, x = x0 + lx;
        const bool live = idx < NPIX, inimg = live && y >= 0 && y < H && x >= 0 && x < W;
        int f = 0;
        if (x == 0) f |= F_FC;
        if (x == W - 1) f |= F_LC;
        if (y == 0) f |= F_FR;
        if (y == H - 1) f |= F_LR;
        if (inimg) f |= F_IN;
        if (lx > 0) f |= F_L;
        if (ly > 0) f |= F_U;
        if (lx < E - 1) f |= F_R;
        if (ly < E - 1) f |= F_D;
        if (inimg && lx >= K && lx < K + T && ly >= K && ly < K + T) f |= F_OUT;
        if (!live) f = 0;
        flag[e] = f;
        off[e] = base + (long)y * W + x;
#pragma unroll
        for (int m = 0; m < 6; ++m) s[e][m] = inimg ? in[m * ps + off[e]] : 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) k[e][m] = inimg ? c[m * ps + off[e]] : 0.f;
        if (live) {
#pragma unroll
            for (int m = 2; m < 6; ++m) lds[m][idx] = s[e][m];
        }
    }
    __syncthreads();

    for (int it = 0; it < niter; ++it) {
        // u from p (left / up neighbours through LDS)
#pragma unroll
        for (int e = 0; e < Q; ++e) {
            const int idx = tid + NT * e, f = flag[e];
            if (Q * NT > NPIX && idx >= NPIX) continue;
            const int l = (f & F_L) ? idx - 1 : idx, u = (f & F_U) ? idx - E : idx;
            tvl1_u_step(k[e][0], k[e][1], k[e][2], k[e][3], s[e][0], s[e][1], s[e][2], lds[2][l], s[e][3], lds[3][u], s[e][4],
                        lds[4][l], s[e][5], lds[5][u], f & F_FC, f & F_LC, f & F_FR, f & F_LR, q);
            lds[0][idx] = s[e][0];
            lds[1][idx] = s[e][1];
        }
        __syncthreads();
        // p from the new u (right / down neighbours through LDS)
#pragma unroll
        for (int e = 0; e < Q; ++e) {
            const int idx = tid + NT * e, f = flag[e];
            if (Q * NT > NPIX && idx >= NPIX) continue;
            const int r = (f & F_R) ? idx + 1 : idx, d = (f & F_D) ? idx + E : idx;
            tvl1_p_step(s[e][0], lds[0][r], lds[0][d], f & F_LC, f & F_LR, s[e][2], s[e][3], q);
            tvl1_p_step(s[e][1], lds[1][r], lds[1][d], f & F_LC, f & F_LR, s[e][4], s[e][5], q);
#pragma unroll
            for (int m = 2; m < 6; ++m) lds[m][idx] = s[e][m];
        }
        __syncthreads();
    }

#pragma unroll
    for (int e = 0; e < Q; ++e) {
        if (flag[e] & F_OUT) {
#pragma unroll
            for (int m = 0; m < 6; ++m) out[m * ps + off[e]] = s[e][m];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
constexpr int TILE = 32;
constexpr int DEFAULT_K = 4;             // measured at 224 x 224, 32 and 128 pairs: profiles/flow_tvl1.txt

bool shape_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 16 && H <= 2048 && W >= 16 && W <= 2048; }

dim3 row_grid(int planes, int H, int W) { return dim3(egz_cdiv(W, NT), H, planes); }

template <int K>
void launch_tile(const float* in, float* out, const float* c, int N, int H, int W, int niter, Tvl1Par q, hipStream_t st) {
    hipLaunchKernelGGL((tvl1_tile_kernel<TILE, K>), dim3(egz_cdiv(W, TILE), egz_cdiv(H, TILE), N), dim3(NT), 0, st, in, out, c, H,
                       W, (long)N * H * W, niter, q);
}

// `iterations` iterations from buffer a, ping-ponging with b; *where = 0 if the result is in a, 1 if in b.
int iterate(float* a, float* b, const float* c, int N, int H, int W, int iterations, int k, Tvl1Par q, hipStream_t st,
            int* where) {
    float* cur = a;
    float* nxt = b;
    for (int done = 0; done < iterations; done += k) {
        const int n = iterations - done < k ? iterations - done : k;
        switch (k) {
            case 1: hipLaunchKernelGGL(tvl1_iter1_kernel, row_grid(N, H, W), dim3(NT), 0, st, cur, nxt, c, H, W, (long)N * H * W, q); break;
            case 2: launch_tile<2>(cur, nxt, c, N, H, W, n, q, st); break;
            case 3: launch_tile<3>(cur, nxt, c, N, H, W, n, q, st); break;
            case 4: launch_tile<4>(cur, nxt, c, N, H, W, n, q, st); break;
            case 6: launch_tile<6>(cur, nxt, c, N, H, W, n, q, st); break;
            default: launch_tile<8>(cur, nxt, c, N, H, W, n, q, st); break;
        }
        float* t = cur; cur = nxt; nxt = t;
    }
    *where = cur == a ? 0 : 1;
    return 0;
}

bool k_ok(int k) { return (k >= 1 && k <= 4) || k == 6 || k == 8; }

int level_sizes(int H, int W, int nscales, double zfactor, int hs[MAX_LEVELS], int ws[MAX_LEVELS]) {
    int L = 1;
    hs[0] = H; ws[0] = W;
    while (L < nscales && L < MAX_LEVELS) {
        const int h = (int)(hs[L - 1] * zfactor + 0.5), w = (int)(ws[L - 1] * zfactor + 0.5);
        if (h < 16 || w < 16) break;
        hs[L] = h; ws[L] = w;
        ++L;
    }
    return L;
}

template <typename TI>
void launch_gauss(const TI* src, float* tmp, float* dst, int planes, int H, int W, const float* gw, int R, hipStream_t st) {
    hipLaunchKernelGGL(gauss_kernel<TI>, row_grid(planes, H, W), dim3(NT), 0, st, src, tmp, H, W, gw, R, 1);
    hipLaunchKernelGGL(gauss_kernel<float>, row_grid(planes, H, W), dim3(NT), 0, st, (const float*)tmp, dst, H, W, gw, R, 0);
}

}  // namespace

EGZ_API int egz_tvl1_default_k() { return DEFAULT_K; }

// src: N images of H x W BGR bytes, interleaved (N, H, W, 3) or planar (N, 3, H, W) -> dst (N, H, W)
EGZ_API int egz_bgr_to_gray_u8(const unsigned char* src, int N, int H, int W, int planar, unsigned char* dst, hipStream_t st) {
    EGZ_CHECK_ARG(src && dst, "egz_bgr_to_gray_u8: null pointer");
    EGZ_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "egz_bgr_to_gray_u8: empty batch or image (N %d, %d x %d)", N, H, W);
    const long n = (long)N * H * W;
    hipLaunchKernelGGL(gray_kernel, dim3(egz_cdiv(n, NT)), dim3(NT), 0, st, src, dst, n, (long)H * W, planar);
    EGZ_CHECK_LAUNCH("egz_bgr_to_gray_u8");
    return 0;
}

// Separable Gaussian of `planes` images; src is uint8 (src_u8 != 0) or float; tmp and dst: planes x H x W floats each.
EGZ_API int egz_flow_gauss(const void* src, int src_u8, int planes, int H, int W, const float* gw, int R, float* tmp, float* dst,
                           hipStream_t st) {
    EGZ_CHECK_ARG(src && gw && tmp && dst, "egz_flow_gauss: null pointer");
    EGZ_CHECK_ARG(shape_ok(planes, H, W), "egz_flow_gauss: planes %d of %d x %d outside 1 .. 65535 planes of 16 .. 2048", planes, H, W);
    EGZ_CHECK_ARG(R >= 0 && R <= MAX_R, "egz_flow_gauss: tap radius %d outside 0 .. %d", R, MAX_R);
    if (src_u8) launch_gauss((const unsigned char*)src, tmp, dst, planes, H, W, gw, R, st);
    else launch_gauss((const float*)src, tmp, dst, planes, H, W, gw, R, st);
    EGZ_CHECK_LAUNCH("egz_flow_gauss");
    return 0;
}

EGZ_API int egz_flow_resample(const float* src, int planes, int hs, int ws, float* dst, int hd, int wd, float scale,
                              hipStream_t st) {
    EGZ_CHECK_ARG(src && dst, "egz_flow_resample: null pointer");
    EGZ_CHECK_ARG(shape_ok(planes, hs, ws) && shape_ok(planes, hd, wd), "egz_flow_resample: %d planes, %d x %d -> %d x %d: "
                  "1 .. 65535 planes of 16 .. 2048 per side", planes, hs, ws, hd, wd);
    hipLaunchKernelGGL(resample_kernel, row_grid(planes, hd, wd), dim3(NT), 0, st, src, dst, hs, ws, hd, wd, scale);
    EGZ_CHECK_LAUNCH("egz_flow_resample");
    return 0;
}

EGZ_API int egz_flow_grad(const float* img, int planes, int H, int W, float* gx, float* gy, hipStream_t st) {
    EGZ_CHECK_ARG(img && gx && gy, "egz_flow_grad: null pointer");
    EGZ_CHECK_ARG(shape_ok(planes, H, W), "egz_flow_grad: planes %d of %d x %d outside 1 .. 65535 planes of 16 .. 2048", planes, H, W);
    hipLaunchKernelGGL(grad_kernel, row_grid(planes, H, W), dim3(NT), 0, st, img, gx, gy, H, W);
    EGZ_CHECK_LAUNCH("egz_flow_grad");
    return 0;
}

// img: N + 1 planes; i1x, i1y: N planes (gradient of planes 1 .. N); u: (2+, N, H, W) state (u1, u2 read); consts: (4, N, H, W)
EGZ_API int egz_tvl1_warp(const float* img, const float* i1x, const float* i1y, const float* u, float* consts, int N, int H,
                          int W, hipStream_t st) {
    EGZ_CHECK_ARG(img && i1x && i1y && u && consts, "egz_tvl1_warp: null pointer");
    EGZ_CHECK_ARG(shape_ok(N, H, W), "egz_tvl1_warp: N %d pairs of %d x %d outside 1 .. 65535 pairs of 16 .. 2048", N, H, W);
    hipLaunchKernelGGL(warp_kernel, row_grid(N, H, W), dim3(NT), 0, st, img, i1x, i1y, u, consts, H, W, (long)N * H * W);
    EGZ_CHECK_LAUNCH("egz_tvl1_warp");
    return 0;
}

// a, b: (6, N, H, W) state buffers (u1 u2 p11 p12 p21 p22), the state is read from a; consts: (4, N, H, W) gx gy g2 rc.
// k iterations per launch: 1 (streaming form) or 2 / 3 / 4 / 6 / 8 (tiled), 0 = the default.  The result is in a if
// ceil(iterations / k) is even, else in b; the other buffer is overwritten.
EGZ_API int egz_tvl1_iterate(float* a, float* b, const float* consts, int N, int H, int W, int iterations, int k, double tau,
                             double lambda, double theta, hipStream_t st) {
    EGZ_CHECK_ARG(a && b && consts && a != b, "egz_tvl1_iterate: null pointer or one buffer given twice");
    EGZ_CHECK_ARG(shape_ok(N, H, W), "egz_tvl1_iterate: N %d pairs of %d x %d outside 1 .. 65535 pairs of 16 .. 2048", N, H, W);
    EGZ_CHECK_ARG(iterations >= 1 && tau > 0 && lambda > 0 && theta > 0, "egz_tvl1_iterate: iterations %d, tau %g, lambda %g, "
                  "theta %g must be positive", iterations, tau, lambda, theta);
    if (k == 0) k = DEFAULT_K;
    EGZ_CHECK_ARG(k_ok(k), "egz_tvl1_iterate: k = %d iterations per launch is not built (1, 2, 3, 4, 6, 8)", k);
    const Tvl1Par q = {(float)lambda * (float)theta, (float)theta, (float)tau / (float)theta};
    int where;
    iterate(a, b, consts, N, H, W, iterations, k, q, st, &where);
    EGZ_CHECK_LAUNCH("egz_tvl1_iterate");
    return 0;
}

EGZ_API int egz_flow_to_u8(const float* v, long n, double bound, unsigned char* out, hipStream_t st) {
    EGZ_CHECK_ARG(v && out, "egz_flow_to_u8: null pointer");
    EGZ_CHECK_ARG(n >= 1 && bound > 0, "egz_flow_to_u8: n %ld and bound %g must be positive", n, bound);
    hipLaunchKernelGGL(quant_kernel, dim3(egz_cdiv(n, NT)), dim3(NT), 0, st, v, out, n, bound);
    EGZ_CHECK_LAUNCH("egz_flow_to_u8");
    return 0;
}

// Workspace of egz_tvl1_flow in bytes (0: arguments out of range).  Floats: tmp F HW | pyramid F sum(h w) | gradient 2 N HW |
// consts 4 N HW | two states 6 N HW each.
EGZ_API size_t egz_tvl1_flow_ws_bytes(int F, int H, int W, int nscales, double zfactor) {
    if (!shape_ok(F - 1, H, W) || nscales < 1 || !(zfactor > 0 && zfactor < 1)) return 0;
    int hs[MAX_LEVELS], ws[MAX_LEVELS];
    const int L = level_sizes(H, W, nscales, zfactor, hs, ws);
    size_t pyr = 0;
    for (int l = 0; l < L; ++l) pyr += (size_t)hs[l] * ws[l];
    const size_t hw = (size_t)H * W, N = F - 1;
    return sizeof(float) * ((size_t)F * hw + (size_t)F * pyr + 18 * N * hw);
}

// frames: (F, H, W) grey bytes -> u1, u2: (F - 1, H, W) floats each.  gw0 / gw1: the presmoothing / pyramid Gaussian taps
// (2 R + 1 floats each, on the device).  k as in egz_tvl1_iterate.
EGZ_API int egz_tvl1_flow(const unsigned char* frames, int F, int H, int W, const float* gw0, int R0, const float* gw1, int R1,
                          double tau, double lambda, double theta, int nscales, double zfactor, int warps, int iterations, int k,
                          void* ws, size_t ws_bytes, float* u1, float* u2, hipStream_t st) {
    EGZ_CHECK_ARG(frames && gw0 && gw1 && ws && u1 && u2, "egz_tvl1_flow: null pointer");
    const int N = F - 1;
    EGZ_CHECK_ARG(shape_ok(N, H, W), "egz_tvl1_flow: F %d frames of %d x %d outside 2 .. 65536 frames of 16 .. 2048", F, H, W);
    EGZ_CHECK_ARG(tau > 0 && lambda > 0 && theta > 0 && nscales >= 1 && zfactor > 0 && zfactor < 1 && warps >= 1 && iterations >= 1,
                  "egz_tvl1_flow: tau %g, lambda %g, theta %g, nscales %d, warps %d, iterations %d must be positive and "
                  "zfactor %g in (0, 1)", tau, lambda, theta, nscales, warps, iterations, zfactor);
    EGZ_CHECK_ARG(R0 >= 0 && R0 <= MAX_R && R1 >= 0 && R1 <= MAX_R, "egz_tvl1_flow: tap radius %d / %d outside 0 .. %d", R0, R1, MAX_R);
    if (k == 0) k = DEFAULT_K;
    EGZ_CHECK_ARG(k_ok(k), "egz_tvl1_flow: k = %d iterations per launch is not built (1, 2, 3, 4, 6, 8)", k);
    const size_t need = egz_tvl1_flow_ws_bytes(F, H, W, nscales, zfactor);
    EGZ_CHECK_ARG(ws_bytes >= need, "egz_tvl1_flow: workspace of %zu bytes, %zu needed", ws_bytes, need);

    int hs[MAX_LEVELS], wsz[MAX_LEVELS];
    const int L = level_sizes(H, W, nscales, zfactor, hs, wsz);
    const size_t hw = (size_t)H * W;
    float* tmp = (float*)ws;
    float* pyr[MAX_LEVELS];
    float* p = tmp + (size_t)F * hw;
    for (int l = 0; l < L; ++l) { pyr[l] = p; p += (size_t)F * hs[l] * wsz[l]; }
    float* gradx = p;
    float* grady = gradx + (size_t)N * hw;
    float* consts = grady + (size_t)N * hw;
    float* sa = consts + 4 * (size_t)N * hw;
    float* sb = sa + 6 * (size_t)N * hw;
    const Tvl1Par q = {(float)lambda * (float)theta, (float)theta, (float)tau / (float)theta};

    launch_gauss(frames, tmp, pyr[0], F, H, W, gw0, R0, st);
    for (int l = 1; l < L; ++l) {
        launch_gauss((const float*)pyr[l - 1], tmp, sa, F, hs[l - 1], wsz[l - 1], gw1, R1, st);      // sa: idle until the solve
        hipLaunchKernelGGL(resample_kernel, row_grid(F, hs[l], wsz[l]), dim3(NT), 0, st, (const float*)sa, pyr[l], hs[l - 1],
                           wsz[l - 1], hs[l], wsz[l], 1.f);
    }
    EGZ_CHECK_LAUNCH("egz_tvl1_flow (pyramid)");

    float* cur = sa;                 // the state of the level being solved
    float* oth = sb;
    for (int l = L - 1; l >= 0; --l) {
        const int h = hs[l], w = wsz[l];
        const size_t ps = (size_t)N * h * w;
        if (l == L - 1) {
            (void)hipMemsetAsync(cur, 0, 6 * ps * sizeof(float), st);
        } else {
            // the coarse flow sits in `cur` with the coarse plane stride: resample it into the other buffer
            const int hc = hs[l + 1], wc = wsz[l + 1];
            const size_t pc = (size_t)N * hc * wc;
            hipLaunchKernelGGL(resample_kernel, row_grid(N, h, w), dim3(NT), 0, st, (const float*)cur, oth, hc, wc, h, w,
                               (float)w / (float)wc);
            hipLaunchKernelGGL(resample_kernel, row_grid(N, h, w), dim3(NT), 0, st, (const float*)(cur + pc), oth + ps, hc, wc, h,
                               w, (float)h / (float)hc);
            (void)hipMemsetAsync(oth + 2 * ps, 0, 4 * ps * sizeof(float), st);
            float* t = cur; cur = oth; oth = t;
        }
        hipLaunchKernelGGL(grad_kernel, row_grid(N, h, w), dim3(NT), 0, st, (const float*)(pyr[l] + (size_t)h * w), gradx, grady, h, w);
        for (int wi = 0; wi < warps; ++wi) {
            hipLaunchKernelGGL(warp_kernel, row_grid(N, h, w), dim3(NT), 0, st, (const float*)pyr[l], (const float*)gradx,
                               (const float*)grady, (const float*)cur, consts, h, w, (long)ps);
            int where;
            iterate(cur, oth, consts, N, h, w, iterations, k, q, st, &where);
            if (where) { float* t = cur; cur = oth; oth = t; }
        }
        EGZ_CHECK_LAUNCH("egz_tvl1_flow (level)");
    }
    (void)hipMemcpyAsync(u1, cur, (size_t)N * hw * sizeof(float), hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(u2, cur + (size_t)N * hw, (size_t)N * hw * sizeof(float), hipMemcpyDeviceToDevice, st);
    EGZ_CHECK_LAUNCH("egz_tvl1_flow");
    return 0;
}
