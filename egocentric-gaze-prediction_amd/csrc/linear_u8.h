// OpenCV's 8-bit INTER_LINEAR arithmetic (imgproc/resize.cpp: HResizeLinear and the uchar VResizeLinear), shared by the
// translation units that resize 8-bit planes on the device (vis_overlay.hip, late_input.hip).  Integer only; the per-axis tables
// come from hipops.linear_table.
#pragma once

// The four neighbours of one output sample and its coefficients -> the 8-bit result (before the store's uchar cast):
//   S0 = p00 a0 + p01 a1, S1 = p10 a0 + p11 a1, dst = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2
__device__ __forceinline__ int linear_mix(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
    const int S0 = p00 * a0 + p01 * a1;
    const int S1 = p10 * a0 + p11 * a1;
    return (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
}

// One 8-bit channel sample of INTER_LINEAR at output (dy, dx); plane = the source channel's first byte, pitch = bytes between
// two source rows, step = bytes between two horizontally adjacent samples of the channel (1 planar, C interleaved).  sx is
// already clamped into [0, sw - 1] by the table; the rows sy and sy + 1 are clamped here.
__device__ __forceinline__ int linear_sample(const unsigned char* __restrict__ plane, long pitch, int step, int sh, int sw,
                                             int sx, int a0, int a1, int sy, int b0, int b1) {
    const int x1 = min(sx + 1, sw - 1);
    const int r0 = min(max(sy, 0), sh - 1), r1 = min(max(sy + 1, 0), sh - 1);
    const unsigned char* p0 = plane + r0 * pitch;
    const unsigned char* p1 = plane + r1 * pitch;
    return linear_mix((int)p0[(long)sx * step], (int)p0[(long)x1 * step], (int)p1[(long)sx * step], (int)p1[(long)x1 * step],
                      a0, a1, b0, b1);
}
