// Baseline JPEG decode core, shared by the HIP decoder (jpeg_decode.hip) and the host build the tests compile with g++ and
// run under AddressSanitizer / UBSan (tests/jpeg_host_driver.cpp).  The package itself has no CPU decode path.
//
// Scope: sequential Huffman JPEG (SOF0, 8-bit SOF1), 1 or 3 components, luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, one
// scan holding every component, restart intervals, APPn / COM skipped.  Parity target: libjpeg-turbo's default decode as
// cv2.imread runs it -- jpeg_idct_islow, h2v1 / h2v2 fancy upsampling (box upsampling when the chroma row is <= 2 samples
// wide), ycc_rgb_convert's fixed-point tables; libjpeg's corrupt-data rules: a marker or the end of the data pads the bit
// stream with zeros, the MCUs after the one that ran out stay all-zero until the next restart marker, a bad Huffman code
// decodes as symbol 0, and the restart resync follows jpeg_resync_to_restart.
//
// Every byte read is checked against the stream's length, every table index against its table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPG_FN __host__ __device__ inline
#define JPG_TAB static __device__ __constant__ const
#else
#define JPG_FN inline
#define JPG_TAB static const
#endif

namespace jpg {

// CORRUPT: damage inside the scan, decoded with libjpeg's zero padding (cv2 warns and returns the image).  FATAL: a file
// libjpeg refuses (unreadable header, missing or invalid table, EOI before the scan, DC overflow): cv2 returns None.
enum Status { OK = 0, CORRUPT = 1, UNSUPPORTED = 2, GEOMETRY = 3, FATAL = 4 };
constexpr int MAX_DIM = 4096;

// jpeg_natural_order plus libjpeg's 16 guard entries: a run that overshoots coefficient 63 lands on 63
JPG_TAB uint8_t kNatural[80] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
    6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
    39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// zigzag index of natural position p (the inverse of kNatural[0..63]); constexpr, so unrolled uses fold to constants
constexpr uint8_t kZigzag[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

constexpr int LOOK = 9;                // Huffman lookahead bits

// jpeg_make_d_derived_tbl's tables: maxcode / valoffset per code length, and a 9-bit lookahead of (length << 8) | symbol
struct Huff {
    uint16_t look[1 << LOOK];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t val[256];
    int32_t ok;                        // 0: undefined or invalid (JERR_NO_HUFF_TABLE / JERR_BAD_HUFF_TABLE at use)
};

// Per-image result of the entropy stage, read by the IDCT and colour stages.  Planes are stored MCU-padded: plane p has
// bw[p] x bh[p] blocks of 64 natural-order coefficients, then 8 bw x 8 bh samples after the IDCT.
enum Up { UP_NONE = 0, UP_H2V1 = 1, UP_H2V2 = 2, UP_BOX_H2V1 = 3, UP_BOX_H2V2 = 4 };
struct ImgInfo {
    int32_t status;
    int32_t write;                     // 1: the output slot is written (status 0 or 1)
    int32_t nstore;                    // planes decoded: 1 (Y or the only component) or 3
    int32_t cout;                      // channels requested: 1 or 3
    int32_t base_plane;                // first workspace plane of this image
    int32_t up;                        // chroma upsampling (Up)
    int32_t bw[3], bh[3], dw[3], dh[3];
    uint16_t q[3][64];                 // natural order
};

struct Comp {
    int32_t id, h, v, tq, td, ta;
};

struct Decoder {
    Huff ht[8];                        // DC 0..3, AC 0..3
    uint16_t q[4][64];
    Comp comp[3];
    int32_t scan_order[3];
    int32_t nf, ns, width, height, hmax, vmax, restart;
    int32_t jfif, adobe, adobe_transform, sof_seen;
    int64_t scan_pos;                  // first byte of the entropy-coded data
    int32_t warn;                      // a corrupt-data warning was raised (status 1)
};

JPG_FN int be16(const uint8_t* d) { return (d[0] << 8) | d[1]; }

JPG_FN int build_huff(Huff& t, const uint8_t* bits /* [16]: counts of lengths 1..16 */, const uint8_t* vals, int n, bool dc) {
    t.ok = 0;
    int code = 0, p = 0;
    uint16_t hcode[256];
    for (int l = 1; l <= 16; l++) {
        const int c = bits[l - 1];
        if (c) {
            t.valoff[l] = p - code;
            for (int i = 0; i < c; i++) hcode[p++] = (uint16_t)code++;
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
            t.valoff[l] = 0;
        }
        if (code >= (1 << l)) return 0;         // code space overflow (JERR_BAD_HUFF_TABLE)
        code <<= 1;
    }
    t.maxcode[0] = -1; t.valoff[0] = 0;
    t.maxcode[17] = 0xFFFFF; t.valoff[17] = 0;
    for (int i = 0; i < 256; i++) t.val[i] = i < n ? vals[i] : 0;
    if (dc)
        for (int i = 0; i < n; i++)
            if (vals[i] > 15) return 0;
    for (int i = 0; i < (1 << LOOK); i++) t.look[i] = 0;
    p = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < bits[l - 1]; i++, p++) {
            if (l > LOOK) continue;
            const int lb = hcode[p] << (LOOK - l);
            for (int r = 0; r < (1 << (LOOK - l)); r++) t.look[lb + r] = (uint16_t)((l << 8) | t.val[p]);
        }
    }
    t.ok = 1;
    return 1;
}

// Header parse up to the first SOS.  Returns a Status (never CORRUPT: header damage is FATAL, as in libjpeg).
JPG_FN int parse_header(Decoder& s, const uint8_t* d, int64_t len, int want_h, int want_w, int want_c) {
    s.nf = s.ns = s.width = s.height = s.restart = 0;
    s.jfif = s.adobe = s.sof_seen = s.warn = 0;
    s.adobe_transform = 1;
    for (int i = 0; i < 8; i++) s.ht[i].ok = 0;
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 64; k++) s.q[i][k] = 0;
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return FATAL;
    int64_t pos = 2;
    for (;;) {
        // next_marker: skip garbage (warns), swallow fill bytes
        while (pos < len && d[pos] != 0xFF) { pos++; s.warn = 1; }
        while (pos < len && d[pos] == 0xFF) pos++;
        if (pos >= len) return FATAL;
        const int m = d[pos++];
        if (m == 0x00) { s.warn = 1; continue; }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;          // standalone markers
        if (m == 0xD8 || m == 0xD9) return FATAL;                    // SOI again / EOI before any scan
        if (pos + 2 > len) return FATAL;
        const int L = be16(d + pos);
        if (L < 2 || pos + L > len) return FATAL;
        const uint8_t* seg = d + pos + 2;
        const int n = L - 2;
        pos += L;
        if (m == 0xC0 || m == 0xC1) {
            if (s.sof_seen) return FATAL;
            s.sof_seen = 1;
            if (n < 6) return FATAL;
            if (seg[0] != 8) return UNSUPPORTED;                         // 12-bit
            s.height = be16(seg + 1);
            s.width = be16(seg + 3);
            s.nf = seg[5];
            if (s.height == 0) return UNSUPPORTED;                       // height by DNL
            if (s.width == 0) return FATAL;
            if (s.nf != 1 && s.nf != 3) return UNSUPPORTED;              // CMYK / YCCK / two-component
            if (n != 6 + 3 * s.nf) return FATAL;
            s.hmax = s.vmax = 1;
            for (int c = 0; c < s.nf; c++) {
                s.comp[c].id = seg[6 + 3 * c];
                s.comp[c].h = seg[7 + 3 * c] >> 4;
                s.comp[c].v = seg[7 + 3 * c] & 15;
                s.comp[c].tq = seg[8 + 3 * c];
                if (s.comp[c].h < 1 || s.comp[c].h > 4 || s.comp[c].v < 1 || s.comp[c].v > 4 || s.comp[c].tq > 3)
                    return FATAL;
                if (s.comp[c].h > s.hmax) s.hmax = s.comp[c].h;
                if (s.comp[c].v > s.vmax) s.vmax = s.comp[c].v;
            }
            if (s.nf == 1) {
                s.comp[0].h = s.comp[0].v = 1;                           // non-interleaved: one block per MCU
                s.hmax = s.vmax = 1;
            } else {
                const int h0 = s.comp[0].h, v0 = s.comp[0].v;
                if (!((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return UNSUPPORTED;
                for (int c = 1; c < 3; c++)
                    if (s.comp[c].h != 1 || s.comp[c].v != 1) return UNSUPPORTED;
            }
            if (s.width != want_w || s.height != want_h) return GEOMETRY;
        } else if ((m >= 0xC2 && m <= 0xCB && m != 0xC4 && m != 0xC8) || (m >= 0xCD && m <= 0xCF) || m == 0xCC || m == 0xDC) {
            return UNSUPPORTED;                                          // progressive, lossless, arithmetic, DNL
        } else if (m == 0xC4) {
            int o = 0;
            while (o < n) {
                if (o + 17 > n) return FATAL;
                const int tc = seg[o] >> 4, th = seg[o] & 15;
                if (tc > 1 || th > 3) return FATAL;
                int cnt = 0;
                for (int l = 0; l < 16; l++) cnt += seg[o + 1 + l];
                if (cnt > 256 || o + 17 + cnt > n) return FATAL;
                build_huff(s.ht[tc * 4 + th], seg + o + 1, seg + o + 17, cnt, tc == 0);
                o += 17 + cnt;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < n) {
                const int pq = seg[o] >> 4, tq = seg[o] & 15;
                if (pq > 1 || tq > 3) return FATAL;
                if (o + 1 + 64 * (pq + 1) > n) return FATAL;
                for (int k = 0; k < 64; k++)
                    s.q[tq][kNatural[k]] = pq ? (uint16_t)be16(seg + o + 1 + 2 * k) : seg[o + 1 + k];
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (n != 2) return FATAL;
            s.restart = be16(seg);
        } else if (m == 0xE0) {
            if (n >= 5 && seg[0] == 'J' && seg[1] == 'F' && seg[2] == 'I' && seg[3] == 'F' && seg[4] == 0) s.jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') {
                s.adobe = 1;
                s.adobe_transform = seg[11];
            }
        } else if (m == 0xDA) {
            if (!s.sof_seen) return FATAL;
            if (n < 1) return FATAL;
            s.ns = seg[0];
            if (n != 4 + 2 * s.ns || s.ns < 1 || s.ns > 4) return FATAL;
            if (s.ns != s.nf) return UNSUPPORTED;                        // one scan per component: multi-scan baseline
            for (int i = 0; i < s.ns; i++) {
                const int id = seg[1 + 2 * i];
                int c = -1;
                for (int j = 0; j < s.nf; j++)
                    if (s.comp[j].id == id) c = j;
                if (c < 0) return FATAL;
                for (int j = 0; j < i; j++)
                    if (s.scan_order[j] == c) return FATAL;
                s.scan_order[i] = c;
                s.comp[c].td = seg[2 + 2 * i] >> 4;
                s.comp[c].ta = seg[2 + 2 * i] & 15;
                if (s.comp[c].td > 3 || s.comp[c].ta > 3) return FATAL;
                if (!s.ht[s.comp[c].td].ok || !s.ht[4 + s.comp[c].ta].ok) return FATAL;
            }
            if (seg[1 + 2 * s.ns] != 0 || seg[2 + 2 * s.ns] != 63 || seg[3 + 2 * s.ns] != 0) return UNSUPPORTED;
            if (s.nf == 3) {                                             // libjpeg's colour-space guess
                bool rgb = false;
                if (!s.jfif) {
                    if (s.adobe) rgb = s.adobe_transform == 0;
                    else rgb = s.comp[0].id == 'R' && s.comp[1].id == 'G' && s.comp[2].id == 'B';
                }
                if (rgb) return UNSUPPORTED;
            }
            s.scan_pos = pos;
            return OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
    (void)want_c;
}

// Geometry of the stored planes and the per-image info of the later stages.  want_c: 1 (grayscale request: Y only) or 3.
JPG_FN void fill_info(const Decoder& s, ImgInfo& I, int want_c) {
    I.cout = want_c;
    I.nstore = (s.nf == 3 && want_c == 3) ? 3 : 1;
    const int mcux = (s.width + 8 * s.hmax - 1) / (8 * s.hmax), mcuy = (s.height + 8 * s.vmax - 1) / (8 * s.vmax);
    for (int c = 0; c < 3; c++) {
        const int cc = c < s.nf ? c : 0;
        const int h = s.comp[cc].h, v = s.comp[cc].v;
        I.bw[c] = s.nf == 1 ? (s.width + 7) / 8 : mcux * h;
        I.bh[c] = s.nf == 1 ? (s.height + 7) / 8 : mcuy * v;
        I.dw[c] = (s.width * h + s.hmax - 1) / s.hmax;
        I.dh[c] = (s.height * v + s.vmax - 1) / s.vmax;
        for (int k = 0; k < 64; k++) I.q[c][k] = s.q[s.comp[cc].tq][k];
    }
    I.up = UP_NONE;
    if (I.nstore == 3 && s.hmax == 2) {
        const bool fancy = I.dw[1] > 2;
        if (s.vmax == 1) I.up = fancy ? UP_H2V1 : UP_BOX_H2V1;
        else I.up = fancy ? UP_H2V2 : UP_BOX_H2V2;
    }
}

// ----------------------------------------------------------------------------------------------------- entropy decoding
struct Bits {
    const uint8_t* d;
    int64_t len, pos;
    uint64_t buf;                      // low `n` bits valid, the last `pad` of them zero padding
    int n, pad;
    int marker;                        // unread marker (0: none); the end of the data reads as EOI
    int insufficient;
};

JPG_FN int next_byte(Bits& b) {       // -1 at the end of the data
    return b.pos < b.len ? b.d[b.pos++] : -1;
}

JPG_FN void fill(Bits& b) {
    while (b.n <= 56) {
        if (b.marker) {
            b.buf <<= 8; b.n += 8; b.pad += 8;
            continue;
        }
        int c = next_byte(b);
        if (c < 0) { b.marker = 0xD9; continue; }
        if (c == 0xFF) {
            int c2;
            do { c2 = next_byte(b); } while (c2 == 0xFF);
            if (c2 < 0) { b.marker = 0xD9; continue; }
            if (c2 != 0) { b.marker = c2; continue; }
        }
        b.buf = (b.buf << 8) | (uint64_t)c;
        b.n += 8;
    }
}

JPG_FN void consume(Bits& b, int k) {
    if (k > b.n - b.pad) b.insufficient = 1;   // libjpeg: more bits asked for than the segment holds (JWRN_HIT_MARKER)
    b.n -= k;
    if (b.pad > b.n) b.pad = b.n;
}

JPG_FN int get_bits(Bits& b, int k) {
    if (k == 0) return 0;
    if (b.n < k) fill(b);
    const int v = (int)((b.buf >> (b.n - k)) & ((1u << k) - 1));
    consume(b, k);
    return v;
}

JPG_FN int huff_decode(Bits& b, const Huff& t, int& warn) {
    if (b.n < 17) fill(b);
    const int peek = (int)((b.buf >> (b.n - LOOK)) & ((1 << LOOK) - 1));
    const int e = t.look[peek];
    if (e) {
        consume(b, e >> 8);
        return e & 0xFF;
    }
    int l = LOOK + 1;
    int code = (int)((b.buf >> (b.n - l)) & ((1 << l) - 1));
    while (l <= 16 && code > t.maxcode[l]) {
        l++;
        code = (int)((b.buf >> (b.n - l)) & ((1 << l) - 1));
    }
    if (l > 16) {                      // JWRN_HUFF_BAD_CODE: 17 bits consumed, symbol 0
        consume(b, 17);
        warn = 1;
        return 0;
    }
    consume(b, l);
    return t.val[(code + t.valoff[l]) & 0xFF];
}

JPG_FN int extend(int r, int s) { return r < (1 << (s - 1)) ? r + (int)((~0u) << s) + 1 : r; }

// next_marker after the bit buffer is dropped: skip to FF xx, xx not 00 / FF
JPG_FN void next_marker(Bits& b, int& warn) {
    for (;;) {
        int c = next_byte(b);
        while (c >= 0 && c != 0xFF) { warn = 1; c = next_byte(b); }
        if (c < 0) { b.marker = 0xD9; return; }
        do { c = next_byte(b); } while (c == 0xFF);
        if (c < 0) { b.marker = 0xD9; return; }
        if (c != 0) { b.marker = c; return; }
        warn = 1;
    }
}

// process_restart + read_restart_marker + jpeg_resync_to_restart
JPG_FN void restart(Bits& b, int& next_rst, int& warn) {
    b.n = b.pad = 0;
    b.buf = 0;
    if (!b.marker) next_marker(b, warn);
    if (b.marker == 0xD0 + next_rst) {
        b.marker = 0;
    } else {
        warn = 1;
        for (;;) {
            const int m = b.marker;
            int action;
            if (m < 0xC0) action = 2;
            else if (m < 0xD0 || m > 0xD7) action = 3;
            else if (m == 0xD0 + ((next_rst + 1) & 7) || m == 0xD0 + ((next_rst + 2) & 7)) action = 3;
            else if (m == 0xD0 + ((next_rst - 1) & 7) || m == 0xD0 + ((next_rst - 2) & 7)) action = 2;
            else action = 1;
            if (action == 1) { b.marker = 0; break; }
            if (action == 3) break;
            if (b.marker == 0xD9 && b.pos >= b.len) break;               // nothing left to scan
            b.marker = 0;
            next_marker(b, warn);
        }
    }
    next_rst = (next_rst + 1) & 7;
    if (b.marker == 0) b.insufficient = 0;
}

// Entropy-decodes the scan into `coef` (planes of I.nstore: plane p at coef + p * plane_elems, zero-filled by the caller).
// Coefficients are stored in zigzag order (idct_islow reorders).  Returns OK, CORRUPT (a warning was raised) or FATAL.
JPG_FN int decode_scan(Decoder& s, const ImgInfo& I, const uint8_t* d, int64_t len, int16_t* coef, int64_t plane_elems) {
    Bits b;
    b.d = d; b.len = len; b.pos = s.scan_pos; b.buf = 0; b.n = b.pad = 0; b.marker = 0; b.insufficient = 0;
    int warn = s.warn;
    int last_dc[3] = {0, 0, 0};
    const int mcux = s.nf == 1 ? I.bw[0] : (s.width + 8 * s.hmax - 1) / (8 * s.hmax);
    const int mcuy = s.nf == 1 ? I.bh[0] : (s.height + 8 * s.vmax - 1) / (8 * s.vmax);
    int to_go = s.restart, next_rst = 0;
    bool dead = false;                 // DC overflow (JERR_BAD_DCT_COEF): stop
    for (int my = 0; my < mcuy && !dead; my++) {
        for (int mx = 0; mx < mcux && !dead; mx++) {
            if (s.restart) {
                if (to_go == 0) {
                    restart(b, next_rst, warn);
                    for (int c = 0; c < 3; c++) last_dc[c] = 0;
                    to_go = s.restart;
                }
                to_go--;
            }
            if (b.insufficient) continue;
            for (int si = 0; si < s.ns; si++) {
                const int c = s.scan_order[si];
                const Comp& cp = s.comp[c];
                const Huff& dct = s.ht[cp.td];
                const Huff& act = s.ht[4 + cp.ta];
                const bool store = c < I.nstore;
                for (int by = 0; by < cp.v; by++) {
                    for (int bx = 0; bx < cp.h; bx++) {
                        const int gx = mx * cp.h + bx, gy = my * cp.v + by;
                        int16_t* blk = store ? coef + c * plane_elems + ((int64_t)gy * I.bw[c] + gx) * 64 : nullptr;
                        int t = huff_decode(b, dct, warn);
                        int diff = 0;
                        if (t) diff = extend(get_bits(b, t), t);
                        const int64_t dc = (int64_t)last_dc[c] + diff;
                        if (dc > 2147483647LL || dc < -2147483647LL - 1) { dead = true; warn = 1; break; }
                        last_dc[c] = (int)dc;
                        if (blk) blk[0] = (int16_t)(uint16_t)(uint32_t)dc;
                        for (int k = 1; k < 64; k++) {
                            const int rs = huff_decode(b, act, warn);
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz) {
                                k += r;
                                const int v = extend(get_bits(b, sz), sz);
                                if (blk) blk[k < 63 ? k : 63] = (int16_t)v;    // kNatural's guard entries
                            } else {
                                if (r != 15) break;
                                k += 15;
                            }
                        }
                    }
                    if (dead) break;
                }
                if (dead) break;
            }
        }
    }
    if (b.insufficient) warn = 1;
    return dead ? FATAL : (warn ? CORRUPT : OK);
}

// ----------------------------------------------------------------------------------------------------- IDCT (jidctint.c)
JPG_FN uint8_t idct_limit(int64_t x) {   // range_limit[x & RANGE_MASK] of the post-IDCT table: 10-bit wrap, + 128, clamp
    int m = (int)(x & 1023);
    if (m >= 512) m -= 1024;
    m += 128;
    return (uint8_t)(m < 0 ? 0 : (m > 255 ? 255 : m));
}

// zz: one block's coefficients in zigzag order; q in natural order
JPG_FN void idct_islow(const int16_t* zz, const uint16_t* q, uint8_t* out, int stride) {
    int16_t in[64];
#pragma unroll
    for (int p = 0; p < 64; p++) in[p] = zz[kZigzag[p]];
    const int64_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                  F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    int ws[64];
    for (int c = 0; c < 8; c++) {
        const int16_t* ip = in + c;
        const uint16_t* qp = q + c;
        if (ip[8] == 0 && ip[16] == 0 && ip[24] == 0 && ip[32] == 0 && ip[40] == 0 && ip[48] == 0 && ip[56] == 0) {
            const int dc = (int)((int64_t)ip[0] * qp[0] * 4);
            for (int r = 0; r < 8; r++) ws[r * 8 + c] = dc;
            continue;
        }
        int64_t z2 = (int64_t)ip[16] * qp[16], z3 = (int64_t)ip[48] * qp[48];
        int64_t z1 = (z2 + z3) * F0541;
        int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
        z2 = (int64_t)ip[0] * qp[0];
        z3 = (int64_t)ip[32] * qp[32];
        int64_t tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = (int64_t)ip[56] * qp[56];
        tmp1 = (int64_t)ip[40] * qp[40];
        tmp2 = (int64_t)ip[24] * qp[24];
        tmp3 = (int64_t)ip[8] * qp[8];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1175;
        tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
        z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        const int64_t R = 1 << 10;     // DESCALE(x, CONST_BITS - PASS1_BITS = 11)
        ws[0 * 8 + c] = (int)((tmp10 + tmp3 + R) >> 11);
        ws[7 * 8 + c] = (int)((tmp10 - tmp3 + R) >> 11);
        ws[1 * 8 + c] = (int)((tmp11 + tmp2 + R) >> 11);
        ws[6 * 8 + c] = (int)((tmp11 - tmp2 + R) >> 11);
        ws[2 * 8 + c] = (int)((tmp12 + tmp1 + R) >> 11);
        ws[5 * 8 + c] = (int)((tmp12 - tmp1 + R) >> 11);
        ws[3 * 8 + c] = (int)((tmp13 + tmp0 + R) >> 11);
        ws[4 * 8 + c] = (int)((tmp13 - tmp0 + R) >> 11);
    }
    for (int r = 0; r < 8; r++) {
        const int* w = ws + r * 8;
        uint8_t* o = out + (int64_t)r * stride;
        int64_t z2 = w[2], z3 = w[6];
        int64_t z1 = (z2 + z3) * F0541;
        int64_t tmp2 = z1 + z3 * -F1847, tmp3 = z1 + z2 * F0765;
        int64_t tmp0 = ((int64_t)w[0] + w[4]) * 8192, tmp1 = ((int64_t)w[0] - w[4]) * 8192;
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = w[7]; tmp1 = w[5]; tmp2 = w[3]; tmp3 = w[1];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1175;
        tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
        z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        const int64_t R = 1 << 17;     // DESCALE(x, CONST_BITS + PASS1_BITS + 3 = 18)
        o[0] = idct_limit((tmp10 + tmp3 + R) >> 18);
        o[7] = idct_limit((tmp10 - tmp3 + R) >> 18);
        o[1] = idct_limit((tmp11 + tmp2 + R) >> 18);
        o[6] = idct_limit((tmp11 - tmp2 + R) >> 18);
        o[2] = idct_limit((tmp12 + tmp1 + R) >> 18);
        o[5] = idct_limit((tmp12 - tmp1 + R) >> 18);
        o[3] = idct_limit((tmp13 + tmp0 + R) >> 18);
        o[4] = idct_limit((tmp13 - tmp0 + R) >> 18);
    }
}

// ----------------------------------------------------------------------------------------------------- upsampling + colour
// One chroma sample of output pixel (x, y) from a plane of dw x dh samples (row stride `st`), libjpeg's jdsample.c rules
// written per output sample: neighbours clamp at the edges, which is what the first / last column special cases and the
// replicated context rows compute.
JPG_FN int chroma(const uint8_t* p, int st, int up, int dw, int dh, int x, int y) {
    switch (up) {
    case UP_H2V1: {
        const int i = x >> 1, t = 3 * p[(int64_t)y * st + i];
        return (x & 1) ? (t + p[(int64_t)y * st + (i + 1 < dw ? i + 1 : dw - 1)] + 2) >> 2
                       : (t + p[(int64_t)y * st + (i > 0 ? i - 1 : 0)] + 1) >> 2;
    }
    case UP_H2V2: {
        const int i = x >> 1, j = y >> 1;
        const int jn = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
        const uint8_t* r0 = p + (int64_t)j * st;
        const uint8_t* r1 = p + (int64_t)jn * st;
        const int in = (x & 1) ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
        const int t = 3 * r0[i] + r1[i], u = 3 * r0[in] + r1[in];
        return (x & 1) ? (t * 3 + u + 7) >> 4 : (t * 3 + u + 8) >> 4;
    }
    case UP_BOX_H2V1: return p[(int64_t)y * st + (x >> 1)];
    case UP_BOX_H2V2: return p[(int64_t)(y >> 1) * st + (x >> 1)];
    default: return p[(int64_t)y * st + x];
    }
}

JPG_FN uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// ycc_rgb_convert (jdcolor.c, SCALEBITS 16): -> b, g, r
JPG_FN void ycc_bgr(int y, int cb, int cr, uint8_t* bgr) {
    const int xb = cb - 128, xr = cr - 128;
    const int crr = (91881 * xr + 32768) >> 16;                         // FIX(1.40200)
    const int cbb = (116130 * xb + 32768) >> 16;                        // FIX(1.77200)
    const int g = (-22554 * xb + 32768 + -46802 * xr) >> 16;            // FIX(0.34414), FIX(0.71414)
    bgr[0] = clamp255(y + cbb);
    bgr[1] = clamp255(y + g);
    bgr[2] = clamp255(y + crr);
}

}  // namespace jpg
