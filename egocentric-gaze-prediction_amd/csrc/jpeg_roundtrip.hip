// jpeg_decode(jpeg_encode(x, quality)) of N grey planes of one geometry in one launch, bit for bit, without the bitstream:
// per 8x8 block FDCT + quantisation (jpeg_enc_core.h) then dequantisation + IDCT + range limit (jpeg_core.h), composed in
// jpeg_roundtrip_core.h.  The Huffman stage between the two is lossless, so it is left out, and with it the workspace, the
// bit-position scans and the read-back of the file lengths.  The quantisation is the lossy step and stays.
//
// One thread per 8x8 block, blocks of all planes on one grid axis (grid-stride, so no plane count meets a grid limit).
// Thread 0 of a workgroup builds the call's tables with jpge::setup -- the function that writes a file's DQT segment -- into
// LDS; only q[0] of them is read.  A thread reads the 64 samples of its footprint (edge blocks replicate the last row /
// column) before it stores any, and no thread reads outside its footprint, so a destination plane may be the source plane.
// Plane i goes to plane planes[i] of dst (null: i); an index outside [0, dst_planes) sets status[i] = 1 and writes nothing.
#include "egz_common.h"
#include "jpeg_roundtrip_core.h"

namespace {

constexpr int NT = 256;
constexpr long MAX_GRID = 1L << 20;

__global__ void __launch_bounds__(NT) jpeg_roundtrip_kernel(const uint8_t* src, jpge::Geo g, int quality, long N,
                                                            const long* __restrict__ planes, uint8_t* dst, long dst_planes,
                                                            int* __restrict__ status) {
    __shared__ jpge::Setup s;
    __shared__ uint16_t q[64];
    if (threadIdx.x == 0) jpge::setup(s, g, quality);
    __syncthreads();
    if (threadIdx.x < 64) q[threadIdx.x] = s.q[0][threadIdx.x];
    __syncthreads();
    const long HW = (long)g.H * g.W, total = N * g.nblk;
    for (long gb = (long)blockIdx.x * NT + threadIdx.x; gb < total; gb += (long)gridDim.x * NT) {
        const long n = gb / g.nblk;
        const int b = (int)(gb - n * g.nblk);
        const long p = planes ? planes[n] : n;
        const bool ok = p >= 0 && p < dst_planes;
        if (b == 0) status[n] = ok ? 0 : 1;
        if (!ok) continue;
        uint8_t px[64];
        jprt::block(g, s, q, src + n * HW, b, px);
        const int y0 = (b / g.ybw) * 8, x0 = (b % g.ybw) * 8;
        uint8_t* o = dst + p * HW + (long)y0 * g.W + x0;
        const bool wide = x0 + 8 <= g.W;
#pragma unroll
        for (int y = 0; y < 8; y++) {
            if (y0 + y < g.H) {
                uint8_t* r = o + (long)y * g.W;
                if (wide && ((uintptr_t)r & 7) == 0) {
                    uint2 v;
                    v.x = px[8 * y] | (px[8 * y + 1] << 8) | (px[8 * y + 2] << 16) | ((uint32_t)px[8 * y + 3] << 24);
                    v.y = px[8 * y + 4] | (px[8 * y + 5] << 8) | (px[8 * y + 6] << 16) | ((uint32_t)px[8 * y + 7] << 24);
                    *(uint2*)r = v;
                } else {
#pragma unroll
                    for (int x = 0; x < 8; x++)
                        if (x0 + x < g.W) r[x] = px[8 * y + x];
                }
            }
        }
    }
}

}  // namespace

EGZ_API int egz_jpeg_roundtrip(const unsigned char* src, long N, int H, int W, int quality, const long* planes,
                               unsigned char* dst, long dst_planes, int* status, hipStream_t stream) {
    EGZ_CHECK_ARG(N >= 1, "egz_jpeg_roundtrip: N=%ld < 1", N);
    EGZ_CHECK_ARG(H > 0 && W > 0 && H <= jpge::MAX_DIM && W <= jpge::MAX_DIM,
                  "egz_jpeg_roundtrip: bad geometry H=%d W=%d (1 <= H, W <= %d)", H, W, jpge::MAX_DIM);
    EGZ_CHECK_ARG(quality >= 1 && quality <= 100, "egz_jpeg_roundtrip: quality=%d outside 1 .. 100", quality);
    EGZ_CHECK_ARG(src && dst && status && dst_planes >= 1, "egz_jpeg_roundtrip: null pointer or empty destination");
    jpge::Geo g;
    jpge::make_geo(g, H, W, 1);
    const long wgs = (N * g.nblk + NT - 1) / NT;
    jpeg_roundtrip_kernel<<<(unsigned)(wgs > MAX_GRID ? MAX_GRID : wgs), NT, 0, stream>>>(src, g, quality, N, planes, dst,
                                                                                         dst_planes, status);
    EGZ_CHECK_LAUNCH("egz_jpeg_roundtrip");
    return 0;
}
