// Host driver of the JPEG round-trip core for tests/test_jpeg_roundtrip_host.py (built with g++ under AddressSanitizer +
// UBSan).  Input file: int32 count, then per image int32 h, w, quality and h * w grey pixel bytes.  Output file: per image
// int32 return code, then (code 0) h * w bytes.  Input and output are heap blocks of exactly h * w bytes, so a read or a
// write outside the plane is a sanitizer report.
#include <cstdio>
#include <cstdlib>

#include "jpeg_roundtrip_core.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, fi) != 1) return 2;
    for (int i = 0; i < n; i++) {
        int32_t hd[3];
        if (fread(hd, 4, 3, fi) != 3) return 2;
        const size_t npx = (size_t)hd[0] * hd[1];
        uint8_t* px = (uint8_t*)malloc(npx ? npx : 1);
        uint8_t* out = (uint8_t*)malloc(npx ? npx : 1);
        if (npx && fread(px, 1, npx, fi) != npx) return 2;
        const int32_t rc = jprt::roundtrip_image(px, hd[0], hd[1], hd[2], out);
        fwrite(&rc, 4, 1, fo);
        if (rc == 0) fwrite(out, 1, npx, fo);
        free(px);
        free(out);
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
