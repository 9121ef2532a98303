// Host build of csrc/jpeg_core.h for tests/test_jpeg_host.py (g++ -fsanitize=address,undefined): runs the same header parse,
// entropy decode, IDCT and colour stages as csrc/jpeg_decode.hip, one stream after another.
//   input:  int32 count, then per stream: int32 H, W, channels, int64 length, `length` bytes
//   output: per stream: int32 status, then channels * H * W bytes (zeros where the decoder writes nothing: status 2, 3, 4)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_core.h"

static void read_exact(FILE* f, void* p, size_t n) {
    if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t count;
    read_exact(fi, &count, 4);
    jpg::Decoder* dec = new jpg::Decoder;
    for (int i = 0; i < count; i++) {
        int32_t hwc[3];
        int64_t len;
        read_exact(fi, hwc, 12);
        read_exact(fi, &len, 8);
        const int H = hwc[0], W = hwc[1], C = hwc[2];
        // exactly `len` bytes on the heap: AddressSanitizer flags any read past the stream
        uint8_t* d = (uint8_t*)malloc(len ? (size_t)len : 1);
        read_exact(fi, d, (size_t)len);
        std::vector<uint8_t> out((size_t)C * H * W, 0);
        jpg::ImgInfo I;
        memset(&I, 0, sizeof(I));
        int st = jpg::parse_header(*dec, d, len, H, W, C);
        if (st == jpg::OK) {
            jpg::fill_info(*dec, I, C);
            const long pb = (long)(2 * ((W + 15) / 16)) * (2 * ((H + 15) / 16));
            // exactly the planes this stream uses, so that a stray write is caught
            std::vector<int16_t> coef((size_t)I.nstore * pb * 64, 0);
            std::vector<uint8_t> pix((size_t)I.nstore * pb * 64, 0);
            st = jpg::decode_scan(*dec, I, d, len, coef.data(), pb * 64);
            for (int p = 0; st != jpg::FATAL && p < I.nstore; p++)
                for (int by = 0; by < I.bh[p]; by++)
                    for (int bx = 0; bx < I.bw[p]; bx++) {
                        const int stride = I.bw[p] * 8;
                        jpg::idct_islow(coef.data() + ((size_t)p * pb + (size_t)by * I.bw[p] + bx) * 64, I.q[p],
                                        pix.data() + (size_t)p * pb * 64 + (size_t)by * 8 * stride + bx * 8, stride);
                    }
            const size_t HW = (size_t)H * W;
            for (int y = 0; st != jpg::FATAL && y < H; y++)
                for (int x = 0; x < W; x++) {
                    const size_t px = (size_t)y * W + x;
                    const int Y = pix[(size_t)y * I.bw[0] * 8 + x];
                    if (C == 1 || I.nstore == 1) {
                        for (int c = 0; c < C; c++) out[c * HW + px] = (uint8_t)Y;
                        continue;
                    }
                    const int s1 = I.bw[1] * 8;
                    const int cb = jpg::chroma(pix.data() + pb * 64, s1, I.up, I.dw[1], I.dh[1], x, y);
                    const int cr = jpg::chroma(pix.data() + 2 * pb * 64, s1, I.up, I.dw[2], I.dh[2], x, y);
                    uint8_t bgr[3];
                    jpg::ycc_bgr(Y, cb, cr, bgr);
                    for (int c = 0; c < 3; c++) out[c * HW + px] = bgr[c];
                }
        }
        free(d);
        const int32_t s32 = st;
        fwrite(&s32, 4, 1, fo);
        fwrite(out.data(), 1, out.size(), fo);
    }
    delete dec;
    fclose(fi);
    fclose(fo);
    return 0;
}
