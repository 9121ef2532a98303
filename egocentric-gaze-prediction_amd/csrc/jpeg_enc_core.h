// Baseline JPEG encode core, shared by the HIP encoder (jpeg_encode.hip) and the host build the tests compile with g++ and
// run under AddressSanitizer / UBSan (tests/jpeg_enc_host_driver.cpp).  The package itself has no CPU encode path.
//
// Scope: 8-bit input, one component (grey) or three (interleaved BGR, written as YCbCr 4:2:0: Y 2x2, Cb / Cr 1x1), 1x1 to
// 4096x4096, quality 1..100, sequential Huffman (SOF0) with the Annex K tables, no restart markers, no optimisation pass.
// Parity target: libjpeg-turbo with its defaults as Pillow's Image.save(format="JPEG", quality=q) and cv2.imwrite run it,
// whole file, byte for byte -- rgb_ycc_convert's 16-bit fixed point, right / bottom edge replication before the h2v2
// down-sampling with its alternating bias, jfdctint ("islow"), jpeg_quality_scaling with force-baseline, quantisation by
// q << 3 rounding half away from zero, the coefficient controller's dummy blocks (all-zero AC, the DC of the block before
// them in the MCU) where the luma plane does not fill its last MCU, encode_one_block's entropy coding, 0xFF stuffing and
// the 1-bit padding of the last byte, and the header segments in libjpeg's order.
//
// Every block is coded on its own: block_coefs() gives block b of the scan its quantised coefficients in zigzag order from
// the pixels alone, prev_block() names the block whose DC it is predicted from, block bit counts add up to bit positions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPE_FN __host__ __device__ inline
#define JPE_TAB static __device__ __constant__ const
#else
#define JPE_FN inline
#define JPE_TAB static const
#endif

namespace jpge {

enum Status { OK = 0, TOO_SMALL = 1 };
constexpr int MAX_DIM = 4096;
constexpr int HDR_MAX = 640;           // 623 bytes for three components
// the longest a block can code: DC 9 + 11 bits, 63 AC coefficients of 16 + 10 bits
constexpr int MAX_BLOCK_BITS = 20 + 63 * 26;

// zigzag index of natural position p
constexpr uint8_t kZigzag[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K base quantisation tables, natural order
JPE_TAB uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K Huffman tables: counts of the code lengths 1..16, then the symbols in code order
JPE_TAB uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
JPE_TAB uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
JPE_TAB uint8_t kAcVals[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161,
     8,   35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,
     39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,
     87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
     178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
     215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249,
     250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,
     145, 161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,
     26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,
     86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
     132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
     169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
     213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249,
     250}};

// Geometry of one image.  nc 1: every MCU is one block, bw x bh blocks in raster order.  nc 3: MCUs of 16 x 16 pixels in
// raster order, six blocks each -- Y (0,0) (0,1) (1,0) (1,1), Cb, Cr; ybw x ybh luma blocks are real, the others dummies.
struct Geo {
    int32_t W, H, nc;
    int32_t ybw, ybh;                  // luma blocks that hold pixels: ceil(W / 8), ceil(H / 8)
    int32_t mcux, mcuy;
    int32_t nblk;                      // blocks in the scan
};

JPE_FN bool make_geo(Geo& g, int H, int W, int nc) {
    if (H < 1 || W < 1 || H > MAX_DIM || W > MAX_DIM || (nc != 1 && nc != 3)) return false;
    g.W = W; g.H = H; g.nc = nc;
    g.ybw = (W + 7) / 8;
    g.ybh = (H + 7) / 8;
    g.mcux = nc == 1 ? g.ybw : (W + 15) / 16;
    g.mcuy = nc == 1 ? g.ybh : (H + 15) / 16;
    g.nblk = g.mcux * g.mcuy * (nc == 1 ? 1 : 6);
    return true;
}

// What one call needs besides the pixels, the same for every image of it: header bytes, quantisation tables (natural
// order) and the Huffman code / length of every symbol (jpeg_make_c_derived_tbl).  Table 0: luma, 1: chroma.
struct Setup {
    uint8_t hdr[HDR_MAX];
    int32_t hdr_len;
    uint8_t q[2][64];
    uint16_t dc_code[2][16];
    uint8_t dc_size[2][16];
    uint16_t ac_code[2][256];
    uint8_t ac_size[2][256];
};

JPE_FN void derive(const uint8_t* bits, const uint8_t* vals, int n, uint16_t* code_of, uint8_t* size_of, int table_len) {
    for (int i = 0; i < table_len; i++) { code_of[i] = 0; size_of[i] = 0; }
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1] && p < n; i++, p++) {
            code_of[vals[p]] = (uint16_t)code++;
            size_of[vals[p]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

JPE_FN void setup(Setup& s, const Geo& g, int quality) {
    // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) {
            long v = ((long)kBaseQ[t][k] * scale + 50) / 100;
            s.q[t][k] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    uint8_t dcv[12];
    for (int i = 0; i < 12; i++) dcv[i] = (uint8_t)i;
    for (int t = 0; t < 2; t++) {
        derive(kDcBits[t], dcv, 12, s.dc_code[t], s.dc_size[t], 16);
        derive(kAcBits[t], kAcVals[t], 162, s.ac_code[t], s.ac_size[t], 256);
    }
    uint8_t* h = s.hdr;
    int n = 0;
    const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; i++) h[n++] = app0[i];
    const int nt = g.nc == 1 ? 1 : 2;
    for (int t = 0; t < nt; t++) {
        h[n++] = 0xFF; h[n++] = 0xDB; h[n++] = 0; h[n++] = 67; h[n++] = (uint8_t)t;
        for (int p = 0; p < 64; p++) h[n + kZigzag[p]] = s.q[t][p];
        n += 64;
    }
    h[n++] = 0xFF; h[n++] = 0xC0; h[n++] = 0; h[n++] = (uint8_t)(8 + 3 * g.nc); h[n++] = 8;
    h[n++] = (uint8_t)(g.H >> 8); h[n++] = (uint8_t)g.H; h[n++] = (uint8_t)(g.W >> 8); h[n++] = (uint8_t)g.W;
    h[n++] = (uint8_t)g.nc;
    for (int c = 0; c < g.nc; c++) {
        h[n++] = (uint8_t)(c + 1);
        h[n++] = (g.nc == 3 && c == 0) ? 0x22 : 0x11;
        h[n++] = c ? 1 : 0;
    }
    for (int t = 0; t < nt; t++) {
        h[n++] = 0xFF; h[n++] = 0xC4; h[n++] = 0; h[n++] = 31; h[n++] = (uint8_t)t;
        for (int i = 0; i < 16; i++) h[n++] = kDcBits[t][i];
        for (int i = 0; i < 12; i++) h[n++] = dcv[i];
        h[n++] = 0xFF; h[n++] = 0xC4; h[n++] = 0; h[n++] = 181; h[n++] = (uint8_t)(0x10 | t);
        for (int i = 0; i < 16; i++) h[n++] = kAcBits[t][i];
        for (int i = 0; i < 162; i++) h[n++] = kAcVals[t][i];
    }
    h[n++] = 0xFF; h[n++] = 0xDA; h[n++] = 0; h[n++] = (uint8_t)(6 + 2 * g.nc); h[n++] = (uint8_t)g.nc;
    for (int c = 0; c < g.nc; c++) {
        h[n++] = (uint8_t)(c + 1);
        h[n++] = c ? 0x11 : 0x00;
    }
    h[n++] = 0; h[n++] = 63; h[n++] = 0;
    s.hdr_len = n;
}

// Component (0 Y, 1 Cb, 2 Cr) of block b of the scan
JPE_FN int block_comp(const Geo& g, int b) {
    if (g.nc == 1) return 0;
    const int k = b % 6;
    return k < 4 ? 0 : k - 3;
}

// The block whose DC predicts block b's: the one before it of the same component in scan order (-1: none, predictor 0)
JPE_FN int prev_block(const Geo& g, int b) {
    if (g.nc == 1) return b - 1;
    const int k = b % 6;
    if (k >= 1 && k <= 3) return b - 1;
    if (b < 6) return -1;
    return k == 0 ? b - 3 : b - 6;
}

JPE_FN int imin(int a, int b) { return a < b ? a : b; }

// rgb_ycc_convert (SCALEBITS 16) of one interleaved BGR pixel
JPE_FN int ycc_y(const uint8_t* p) { return (19595 * p[2] + 38470 * p[1] + 7471 * p[0] + 32768) >> 16; }
JPE_FN int ycc_cb(const uint8_t* p) { return (-11059 * p[2] - 21709 * p[1] + 32768 * p[0] + (128 << 16) + 32767) >> 16; }
JPE_FN int ycc_cr(const uint8_t* p) { return (32768 * p[2] - 27439 * p[1] - 5329 * p[0] + (128 << 16) + 32767) >> 16; }

// The 64 samples of luma block (r, c), level-shifted; coordinates past the image replicate its last column / row
JPE_FN void load_luma(const Geo& g, const uint8_t* img, int r, int c, int* d) {
    for (int y = 0; y < 8; y++) {
        const int64_t row = (int64_t)imin(r * 8 + y, g.H - 1) * g.W;
        for (int x = 0; x < 8; x++) {
            const int64_t px = row + imin(c * 8 + x, g.W - 1);
            d[y * 8 + x] = (g.nc == 1 ? img[px] : ycc_y(img + 3 * px)) - 128;
        }
    }
}

// The 64 samples of chroma block (r, c) of component comp: h2v2_downsample of the edge-expanded plane.  Columns are
// replicated before the down-sampling; rows are replicated to an even count before it and the down-sampled rows after it.
JPE_FN void load_chroma(const Geo& g, const uint8_t* img, int comp, int r, int c, int* d) {
    const int ch = (g.H + 1) / 2;
    for (int y = 0; y < 8; y++) {
        const int cy = imin(r * 8 + y, ch - 1);
        const int64_t r0 = (int64_t)imin(2 * cy, g.H - 1) * g.W, r1 = (int64_t)imin(2 * cy + 1, g.H - 1) * g.W;
        for (int x = 0; x < 8; x++) {
            const int cx = c * 8 + x;
            const int x0 = imin(2 * cx, g.W - 1), x1 = imin(2 * cx + 1, g.W - 1);
            const uint8_t *a = img + 3 * (r0 + x0), *b = img + 3 * (r0 + x1), *e = img + 3 * (r1 + x0), *f = img + 3 * (r1 + x1);
            const int s = comp == 1 ? ycc_cb(a) + ycc_cb(b) + ycc_cb(e) + ycc_cb(f) : ycc_cr(a) + ycc_cr(b) + ycc_cr(e) + ycc_cr(f);
            d[y * 8 + x] = ((s + 1 + (cx & 1)) >> 2) - 128;
        }
    }
}

// jfdctint.c: CONST_BITS 13, PASS1_BITS 2; the output is the DCT scaled up by 8
JPE_FN void fdct_1d(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7, const int pass) {
    const int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
              F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6;
    int tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int sh = pass == 1 ? 11 : 15;            // CONST_BITS -/+ PASS1_BITS
    const int rnd = 1 << (sh - 1);
    if (pass == 1) {
        d0 = (tmp10 + tmp11) * 4;
        d4 = (tmp10 - tmp11) * 4;
    } else {
        d0 = (tmp10 + tmp11 + 2) >> 2;
        d4 = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * F0541;
    d2 = (z1 + tmp13 * F0765 + rnd) >> sh;
    d6 = (z1 - tmp12 * F1847 + rnd) >> sh;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F1175;
    tmp4 *= F0298; tmp5 *= F2053; tmp6 *= F3072; tmp7 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    d7 = (tmp4 + z1 + z3 + rnd) >> sh;
    d5 = (tmp5 + z2 + z4 + rnd) >> sh;
    d3 = (tmp6 + z2 + z3 + rnd) >> sh;
    d1 = (tmp7 + z1 + z4 + rnd) >> sh;
}

JPE_FN void fdct_islow(int* d) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        int* p = d + 8 * r;
        fdct_1d(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], 1);
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int* p = d + c;
        fdct_1d(p[0], p[8], p[16], p[24], p[32], p[40], p[48], p[56], 2);
    }
}

// Division by q << 3, rounding half away from zero.  libjpeg-turbo multiplies by a 16-bit reciprocal with a correction
// term chosen so that the product equals this quotient for every 16-bit input (tests/test_jpeg_enc_host.py compares
// whole files with Pillow's over all qualities).
JPE_FN int quantise(int v, int q) {
    const int div = q << 3;
    return v < 0 ? -((-v + (div >> 1)) / div) : (v + (div >> 1)) / div;
}

// Quantised coefficients of block b of the scan, zigzag order
JPE_FN void block_coefs(const Geo& g, const Setup& s, const uint8_t* img, int b, int16_t* zz) {
    int d[64];
    int comp = 0, r, c;
    if (g.nc == 1) {
        r = b / g.ybw;
        c = b % g.ybw;
    } else {
        const int m = b / 6, k = b % 6, my = m / g.mcux, mx = m % g.mcux;
        if (k < 4) {
            r = 2 * my + (k >> 1);
            c = 2 * mx + (k & 1);
            if (r >= g.ybh || c >= g.ybw) {
                // dummy block: the DC of the block before it in the MCU (for a bottom row: of the MCU's block (0, 1), itself a
                // copy of (0, 0) where that is a dummy), no AC.  A block's DC is the sum of its level-shifted samples.
                load_luma(g, img, imin(r, g.ybh - 1), imin(r >= g.ybh ? 2 * mx + 1 : c, g.ybw - 1), d);
                int sum = 0;
                for (int i = 0; i < 64; i++) sum += d[i];
                zz[0] = (int16_t)quantise(sum, s.q[0][0]);
                for (int i = 1; i < 64; i++) zz[i] = 0;
                return;
            }
        } else {
            comp = k - 3;
            r = my;
            c = mx;
        }
    }
    if (comp == 0) load_luma(g, img, r, c, d);
    else load_chroma(g, img, comp, r, c, d);
    fdct_islow(d);
    const uint8_t* q = s.q[comp ? 1 : 0];
#pragma unroll
    for (int p = 0; p < 64; p++) zz[kZigzag[p]] = (int16_t)quantise(d[p], q[p]);
}

// JPEG size category: bits needed for |v|
JPE_FN int nbits(int v) {
    int a = v < 0 ? -v : v, n = 0;
    while (a) { n++; a >>= 1; }
    return n;
}

// Scan bits of a block's 63 AC coefficients (run / size codes with ZRL and EOB, plus the value bits)
JPE_FN int ac_bits(const int16_t* zz, const uint8_t* ac_size) {
    int bits = 0, run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = zz[k];
        if (v == 0) { run++; continue; }
        while (run > 15) { bits += ac_size[0xF0]; run -= 16; }
        const int n = nbits(v);
        bits += ac_size[(run << 4) + n] + n;
        run = 0;
    }
    if (run > 0) bits += ac_size[0];
    return bits;
}

JPE_FN int dc_bits(int diff, const uint8_t* dc_size) {
    const int n = nbits(diff);
    return dc_size[n] + n;
}

// encode_one_block: sink.put(value, nbits) takes up to 27 bits at a time, most significant first
template <class Sink>
JPE_FN void emit_block(const int16_t* zz, int prev_dc, const uint16_t* dc_code, const uint8_t* dc_size,
                       const uint16_t* ac_code, const uint8_t* ac_size, Sink& sink) {
    int v = zz[0] - prev_dc;
    int n = nbits(v);
    uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
    sink.put(((uint32_t)dc_code[n] << n) | low, dc_size[n] + n);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        v = zz[k];
        if (v == 0) { run++; continue; }
        while (run > 15) { sink.put(ac_code[0xF0], ac_size[0xF0]); run -= 16; }
        n = nbits(v);
        low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
        const int sym = (run << 4) + n;
        sink.put(((uint32_t)ac_code[sym] << n) | low, ac_size[sym] + n);
        run = 0;
    }
    if (run > 0) sink.put(ac_code[0], ac_size[0]);
}

#if !defined(__HIPCC__)
// Host reference of the whole encoder (tests only): a bounded byte sink with 0xFF stuffing.  Returns the length the
// file needs; nothing is written at or beyond `cap`, and the file is complete only if the return value is <= cap.
struct ByteSink {
    uint8_t* out;
    int64_t cap, n;
    uint64_t acc;
    int nacc;
    void byte(int v) {
        if (n < cap) out[n] = (uint8_t)v;
        n++;
    }
    void put(uint32_t v, int len) {
        acc = (acc << len) | v;
        nacc += len;
        while (nacc >= 8) {
            const int c = (int)((acc >> (nacc - 8)) & 0xFF);
            byte(c);
            if (c == 0xFF) byte(0);
            nacc -= 8;
        }
    }
};

inline int64_t encode_image(const uint8_t* img, int H, int W, int nc, int quality, uint8_t* out, int64_t cap) {
    Geo g;
    if (!make_geo(g, H, W, nc) || quality < 1 || quality > 100) return -1;
    static Setup s;
    setup(s, g, quality);
    ByteSink sink{out, cap, 0, 0, 0};
    for (int i = 0; i < s.hdr_len; i++) sink.byte(s.hdr[i]);
    int16_t* dcs = new int16_t[g.nblk];
    int16_t zz[64];
    for (int b = 0; b < g.nblk; b++) {
        block_coefs(g, s, img, b, zz);
        dcs[b] = zz[0];
        const int pb = prev_block(g, b), t = block_comp(g, b) ? 1 : 0;
        emit_block(zz, pb < 0 ? 0 : dcs[pb], s.dc_code[t], s.dc_size[t], s.ac_code[t], s.ac_size[t], sink);
    }
    delete[] dcs;
    if (sink.nacc) sink.put((1u << (8 - sink.nacc)) - 1, 8 - sink.nacc);
    sink.byte(0xFF);
    sink.byte(0xD9);
    return sink.n;
}
#endif

}  // namespace jpge
