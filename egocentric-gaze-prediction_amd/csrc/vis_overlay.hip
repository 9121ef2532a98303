// Feature visualisation (vis_features.py of the reference): OpenCV's INTER_LINEAR resize of 8-bit images, the whole
// resize -> applyColorMap(JET) -> heatmap * 0.3 + img * 0.5 -> imwrite chain of one overlay, and the ground-truth cell of a gaze
// map (argmax of AvgPool2d(cell)).
//
// INTER_LINEAR, 8-bit (imgproc/resize.cpp: resizeGeneric_, HResizeLinear, the uchar specialisation of VResizeLinear), restated:
// per axis, the host builds the source index s and two 11-bit coefficients of each output index in OpenCV's float arithmetic
// (hipops.linear_table); here everything is integer.
//   x: s is already clamped into [0, sw - 1] (coefficient of the right neighbour 0 there), so
//      S[x] = src[s] * a0 + src[min(s + 1, sw - 1)] * a1                    (== src[s] * 2048 at the clamped right edge)
//   y: the rows s and s + 1 are each clamped into [0, sh - 1], the coefficients b0, b1 are left as computed, and
//      dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
// The overlay blend is numpy's float64 expression followed by OpenCV's convertTo(CV_8U) (cvRound: half to even, saturated):
//   out = rint(fl64(fl64(h * 0.3) + fl64(i * 0.5)))
// Every operation is a separate IEEE operation: contraction into FMA is off for this file (build.sh flags unchanged).
#include "egz_common.h"
#include "linear_u8.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

// (linear_sample: one 8-bit channel sample of INTER_LINEAR, linear_u8.h)

// grid (ceil(dh * dw / NT), N); one thread per output pixel, all C channels
__global__ __launch_bounds__(NT) void resize_linear_u8_kernel(const unsigned char* __restrict__ src, int C, int sh, int sw,
                                                              int dh, int dw, int interleaved, const int* __restrict__ xofs,
                                                              const short* __restrict__ xalpha, const int* __restrict__ yofs,
                                                              const short* __restrict__ yalpha, unsigned char* __restrict__ dst) {
    const int n = blockIdx.y;
    const long idx = (long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long)dh * dw) return;
    const int dy = (int)(idx / dw), dx = (int)(idx - (long)dy * dw);
    const int sx = xofs[dx], a0 = xalpha[2 * dx], a1 = xalpha[2 * dx + 1];
    const int sy = yofs[dy], b0 = yalpha[2 * dy], b1 = yalpha[2 * dy + 1];
    const long simg = (long)C * sh * sw, dimg = (long)C * dh * dw;
    const unsigned char* s = src + n * simg;
    unsigned char* d = dst + n * dimg;
    for (int c = 0; c < C; ++c) {
        int v;
        if (interleaved) {
            v = linear_sample(s + c, (long)sw * C, C, sh, sw, sx, a0, a1, sy, b0, b1);
            d[idx * C + c] = (unsigned char)v;
        } else {
            v = linear_sample(s + c * (long)sh * sw, sw, 1, sh, sw, sx, a0, a1, sy, b0, b1);
            d[c * (long)dh * dw + idx] = (unsigned char)v;
        }
    }
}

__device__ __forceinline__ unsigned int blend(int h, int i) {
    const double v = (double)h * 0.3 + (double)i * 0.5;       // two roundings of the products, one of the sum (no FMA)
    return (unsigned int)fmin(fmax(__builtin_rint(v), 0.0), 255.0);
}

// grid (ceil(H * W / (4 NT)), M); one thread per group of 4 consecutive pixels of one overlay.  A full group reads one dword of
// each frame plane and writes its 12 BGR bytes as 3 dwords (the group's offset is a multiple of 12 bytes); a tail group (H W not a
// multiple of 4) goes byte by byte.
__global__ __launch_bounds__(NT) void heatmap_overlay_kernel(const unsigned char* __restrict__ maps, int h, int w,
                                                             const int* __restrict__ frame_index,
                                                             const unsigned char* __restrict__ frames, int H, int W,
                                                             const unsigned char* __restrict__ lut, const int* __restrict__ xofs,
                                                             const short* __restrict__ xalpha, const int* __restrict__ yofs,
                                                             const short* __restrict__ yalpha, unsigned char* __restrict__ out) {
    const int m = blockIdx.y;
    const long HW = (long)H * W;
    const long p0 = ((long)blockIdx.x * NT + threadIdx.x) * 4;
    if (p0 >= HW) return;
    const unsigned char* map = maps + (long)m * h * w;
    const unsigned char* fr = frames + (long)frame_index[m] * 3 * HW;
    unsigned char* o = out + ((long)m * HW + p0) * 3;
    const int npx = (int)min(4L, HW - p0);
    unsigned int res[12];
    unsigned int img[3] = {0u, 0u, 0u};
    const bool full = npx == 4 && (HW & 3) == 0;
    if (full) {
#pragma unroll
        for (int c = 0; c < 3; ++c) img[c] = *reinterpret_cast<const unsigned int*>(fr + c * HW + p0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < npx) {
            const long p = p0 + k;
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const int v = linear_sample(map, w, 1, h, w, xofs[x], xalpha[2 * x], xalpha[2 * x + 1], yofs[y], yalpha[2 * y],
                                        yalpha[2 * y + 1]) & 0xff;           // uchar(...) as OpenCV stores it: a LUT index
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int iv = full ? (int)((img[c] >> (8 * k)) & 0xffu) : (int)fr[c * HW + p];
                res[3 * k + c] = blend(lut[3 * v + c], iv);
            }
        }
    }
    if (full) {
        unsigned int* o32 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            o32[q] = res[4 * q] | (res[4 * q + 1] << 8) | (res[4 * q + 2] << 16) | (res[4 * q + 3] << 24);
    } else {
        for (int k = 0; k < 3 * npx; ++k) o[k] = (unsigned char)res[k];
    }
}

// grid (N); block-wide first arg-max of the exact integer cell sums (ties: the lowest row-major cell index, numpy's rule)
__global__ __launch_bounds__(NT) void cell_argmax_u8_kernel(const unsigned char* __restrict__ gt, int H, int W, int cell,
                                                            int* __restrict__ out) {
    __shared__ long long red[NT / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int ch = H / cell, cw = W / cell, ncell = ch * cw;
    const unsigned char* g = gt + (long)n * H * W;
    // key = sum << 32 | (0xffffffff - index): the maximum key is the largest sum at the smallest index
    long long best = -1;
    for (int q = tid; q < ncell; q += NT) {
        const int cy = q / cw, cx = q - cy * cw;
        long long s = 0;
        for (int y = cy * cell; y < cy * cell + cell; ++y)
            for (int x = cx * cell; x < cx * cell + cell; ++x) s += g[(long)y * W + x];
        const long long key = (s << 32) | (long long)(0xffffffffu - (unsigned int)q);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        long long b = red[0];
        for (int k = 1; k < NT / 64; ++k) b = red[k] > b ? red[k] : b;
        out[n] = (int)(0xffffffffu - (unsigned int)(b & 0xffffffffLL));
    }
}

}  // namespace

// src: N images of C x sh x sw bytes, planar (C, sh, sw) or interleaved (sh, sw, C); dst likewise at dh x dw.  Tables
// (hipops.linear_table): xofs[dw] in [0, sw - 1], xalpha[2 dw]; yofs[dh] (unclamped), yalpha[2 dh].
EGZ_API int egz_resize_linear_u8(const unsigned char* src, int N, int C, int sh, int sw, int dh, int dw, int interleaved,
                                 const int* xofs, const short* xalpha, const int* yofs, const short* yalpha, unsigned char* dst,
                                 hipStream_t st) {
    EGZ_CHECK_ARG(src && dst && xofs && xalpha && yofs && yalpha, "egz_resize_linear_u8: null pointer");
    EGZ_CHECK_ARG(N > 0 && (C == 1 || C == 3) && sh > 0 && sw > 0 && dh > 0 && dw > 0,
                  "egz_resize_linear_u8: bad geometry (N %d, C %d, %d x %d -> %d x %d)", N, C, sh, sw, dh, dw);
    EGZ_CHECK_ARG(N <= 65535, "egz_resize_linear_u8: %d images in one launch (65535 at most)", N);
    hipLaunchKernelGGL(resize_linear_u8_kernel, dim3(egz_cdiv((long)dh * dw, NT), N), dim3(NT), 0, st, src, C, sh, sw, dh, dw,
                       interleaved ? 1 : 0, xofs, xalpha, yofs, yalpha, dst);
    EGZ_CHECK_LAUNCH("egz_resize_linear_u8");
    return 0;
}

// maps: (M, h, w) bytes; frame_index: M ints in [0, F); frames: (F, 3, H, W) BGR planes; lut: 256 x 3 BGR bytes; tables as above
// for h x w -> H x W; out: (M, H, W, 3) BGR bytes.
EGZ_API int egz_heatmap_overlay(const unsigned char* maps, int M, int h, int w, const int* frame_index,
                                const unsigned char* frames, int F, int H, int W, const unsigned char* lut, const int* xofs,
                                const short* xalpha, const int* yofs, const short* yalpha, unsigned char* out,
                                hipStream_t st) {
    EGZ_CHECK_ARG(maps && frame_index && frames && lut && xofs && xalpha && yofs && yalpha && out,
                  "egz_heatmap_overlay: null pointer");
    EGZ_CHECK_ARG(M > 0 && M <= 65535 && F > 0 && h > 0 && w > 0 && H > 0 && W > 0,
                  "egz_heatmap_overlay: bad geometry (M %d, F %d, %d x %d -> %d x %d)", M, F, h, w, H, W);
    hipLaunchKernelGGL(heatmap_overlay_kernel, dim3(egz_cdiv((long)H * W, 4L * NT), M), dim3(NT), 0, st, maps, h, w,
                       frame_index, frames, H, W, lut, xofs, xalpha, yofs, yalpha, out);
    EGZ_CHECK_LAUNCH("egz_heatmap_overlay");
    return 0;
}

// gt: (N, H, W) bytes -> out[n] = row-major index of the first maximal cell-sum over the (H / cell) x (W / cell) cells (a
// remainder of rows / columns is dropped, as AvgPool2d does).
EGZ_API int egz_cell_argmax_u8(const unsigned char* gt, int N, int H, int W, int cell, int* out, hipStream_t st) {
    EGZ_CHECK_ARG(gt && out, "egz_cell_argmax_u8: null pointer");
    EGZ_CHECK_ARG(N > 0 && cell > 0 && H >= cell && W >= cell, "egz_cell_argmax_u8: bad geometry (N %d, %d x %d, cell %d)", N,
                  H, W, cell);
    hipLaunchKernelGGL(cell_argmax_u8_kernel, dim3(N), dim3(NT), 0, st, gt, H, W, cell, out);
    EGZ_CHECK_LAUNCH("egz_cell_argmax_u8");
    return 0;
}
