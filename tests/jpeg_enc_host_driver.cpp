// Host driver of the JPEG encode core for tests/test_jpeg_enc_host.py (built with g++ under AddressSanitizer + UBSan).
// Input file: int32 count, then per image int32 h, w, components, quality, int64 capacity, h * w * components pixel bytes
// (grey, or interleaved BGR).  Output file: per image int64 needed length, then min(needed, capacity) bytes.  Each output
// buffer is a heap block of exactly `capacity` bytes, so a write past the capacity is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_enc_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, fi) != 1) return 2;
    for (int i = 0; i < n; i++) {
        int32_t hd[4];
        int64_t cap;
        if (fread(hd, 4, 4, fi) != 4 || fread(&cap, 8, 1, fi) != 1) return 2;
        const size_t npx = (size_t)hd[0] * hd[1] * hd[2];
        std::vector<uint8_t> px(npx);
        if (npx && fread(px.data(), 1, npx, fi) != npx) return 2;
        uint8_t* out = (uint8_t*)malloc(cap > 0 ? (size_t)cap : 1);
        const int64_t need = jpge::encode_image(px.data(), hd[0], hd[1], hd[2], hd[3], out, cap);
        fwrite(&need, 8, 1, fo);
        if (need > 0) fwrite(out, 1, (size_t)(need < cap ? need : cap), fo);
        free(out);
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
