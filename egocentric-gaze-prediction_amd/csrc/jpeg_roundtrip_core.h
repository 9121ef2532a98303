// Grey baseline JPEG round trip without the bitstream, shared by the HIP kernel (jpeg_roundtrip.hip) and the host build the
// tests compile with g++ and run under AddressSanitizer / UBSan (tests/jpeg_roundtrip_host_driver.cpp).
//
// A grey baseline JPEG is, per 8x8 block, load -> FDCT -> quantise -> [Huffman coding, lossless] -> dequantise -> IDCT ->
// range limit.  The entropy coder carries the quantised coefficients unchanged, so the pixels a decoder gives for an
// encoder's file are a function of the block's own 64 samples and the quantisation table alone: jpge::block_coefs (the
// encoder's half, jpeg_enc_core.h) followed by jpg::idct_islow (the decoder's half, jpeg_core.h), with the one table both
// files would have shared.  Nothing of either half is restated here.
#pragma once
#include "jpeg_core.h"
#include "jpeg_enc_core.h"

#if defined(__HIPCC__)
#define JPR_FN __host__ __device__ inline
#else
#define JPR_FN inline
#endif

namespace jprt {

// The decoder's view of the table jpge::setup built: DQT entries are read back as 16-bit values, natural order
JPR_FN void widen_q(const jpge::Setup& s, uint16_t* q) {
    for (int k = 0; k < 64; k++) q[k] = s.q[0][k];
}

// The 64 samples (row-major, stride 8) a decoder gives for block b (raster order, g.ybw blocks per row) of the file an
// encoder writes for the grey plane `img`.  Samples of a partial block beyond the plane are computed too (from the
// replicated edge, as the encoder codes them); the caller crops.  All of `img` that is read lies inside block b's own
// 8x8 footprint, and it is read before anything is written to px.
JPR_FN void block(const jpge::Geo& g, const jpge::Setup& s, const uint16_t* q, const uint8_t* img, int b, uint8_t* px) {
    int16_t zz[64];
    jpge::block_coefs(g, s, img, b, zz);
    jpg::idct_islow(zz, q, px, 8);
}

#if !defined(__HIPCC__)
// Host reference of the whole round trip (tests only): out is H x W.  Returns 0, or -1 for arguments outside the scope.
inline int roundtrip_image(const uint8_t* img, int H, int W, int quality, uint8_t* out) {
    jpge::Geo g;
    if (!jpge::make_geo(g, H, W, 1) || quality < 1 || quality > 100) return -1;
    static jpge::Setup s;
    jpge::setup(s, g, quality);
    uint16_t q[64];
    widen_q(s, q);
    for (int b = 0; b < g.nblk; b++) {
        uint8_t px[64];
        block(g, s, q, img, b, px);
        const int y0 = (b / g.ybw) * 8, x0 = (b % g.ybw) * 8;
        for (int y = 0; y < 8 && y0 + y < H; y++)
            for (int x = 0; x < 8 && x0 + x < W; x++) out[(int64_t)(y0 + y) * W + x0 + x] = px[y * 8 + x];
    }
    return 0;
}
#endif

}  // namespace jprt
