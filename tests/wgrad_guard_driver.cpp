// Host-only build of csrc/conv3x3_wgrad.hip for tests/test_wgrad_dispatch_host.py (-fsanitize=address,undefined on the host
// side).  Uses the public entry points only.  Three parts:
//   guard <name> <rc> <msg>   egz_conv3x3_wgrad with arguments each of its guards rejects, and the error the call left behind
//   sweep file (argv[1])      egz_conv3x3_wgrad_ws_bytes over a grid of geometries and flags: records of 6 int32 (B, H, W, C, K,
//                             flags) + 1 uint64 (bytes), compared with tests/golden/wgrad_ws_bytes.npz
//   short4 <calls> <bad>      at every point of the sweep, egz_conv3x3_wgrad with a workspace 4 bytes short of that, with and
//                             without dy_absmax / x_absmax: bad counts the calls not rejected as "workspace too small"
// No call gets as far as a launch, so no GPU is needed; the pointers are never dereferenced.
#include "conv3x3_wgrad.hip"
#include "egz_core.hip"
#include <cstdint>
#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
    static float buf[4];
    static unsigned int am[4];
    const float* x = buf;
    int bad = 0;
    auto report = [&](const char* name, int rc) {
        printf("guard\t%s\t%d\t%s\n", name, rc, egz_last_error());
        if (rc == 0) bad = 1;               // accepted: the dispatch would have launched
        egz_set_error("%s", "");
    };
    const size_t big = (size_t)1 << 40;
    const int SPLIT = 0x2000, XPRE = 0x8000, DPRE = 0x10000;
    //                                       x  dy  dw   B  H   W   C   K   flags  ws  ws_bytes dy_absmax x_absmax x_bn st
    report("null", egz_conv3x3_wgrad(nullptr, x, buf, 2, 16, 16, 64, 64, SPLIT, buf, big, am, am, nullptr, nullptr));
    report("null_ws", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT, nullptr, big, am, am, nullptr, nullptr));
    report("xbn_wide", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT, buf, big, am, am, x, nullptr));
    report("xbn_width12", egz_conv3x3_wgrad(x, x, buf, 2, 12, 12, 32, 32, SPLIT, buf, big, am, am, x, nullptr));
    report("xbn_ups", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 32, SPLIT | 1, buf, big, am, am, x, nullptr));
    report("xbn_pertap", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 32, SPLIT | 0x800, buf, big, am, am, x, nullptr));
    report("xbn_c6", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 6, 32, SPLIT, buf, big, am, am, x, nullptr));
    report("xbn_f32", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 32, 0, buf, big, nullptr, nullptr, x, nullptr));
    report("c6", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 6, 8, 0, buf, big, nullptr, nullptr, nullptr, nullptr));
    report("k0", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 8, 0, SPLIT, buf, big, nullptr, nullptr, nullptr, nullptr));
    report("ups_odd_h", egz_conv3x3_wgrad(x, x, buf, 2, 7, 8, 64, 64, SPLIT | 1, buf, big, am, am, nullptr, nullptr));
    report("ups_odd_w", egz_conv3x3_wgrad(x, x, buf, 2, 8, 7, 64, 64, 1, buf, big, nullptr, nullptr, nullptr, nullptr));
    report("xpre_ups", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT | XPRE | 1, buf, big, am, am, nullptr, nullptr));
    report("dpre_ups", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT | DPRE | 1, buf, big, am, am, nullptr, nullptr));
    report("xpre_no_dy_absmax", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT | XPRE, buf, big, nullptr, am, nullptr, nullptr));
    report("dpre_no_dy_absmax", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT | DPRE, buf, big, nullptr, am, nullptr, nullptr));
    report("xpre_no_x_absmax", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT | XPRE, buf, big, am, nullptr, nullptr, nullptr));
    report("xpre_f32", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, XPRE, buf, big, am, am, nullptr, nullptr));
    report("xpre_xbn", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 32, SPLIT | XPRE, buf, big, am, am, x, nullptr));
    report("dpre_xbn", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 32, SPLIT | DPRE, buf, big, am, am, x, nullptr));
    report("xpre_k32", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 32, SPLIT | XPRE, buf, big, am, am, nullptr, nullptr));
    report("dpre_c32", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 32, 64, SPLIT | DPRE, buf, big, am, am, nullptr, nullptr));
    report("xpre_width36", egz_conv3x3_wgrad(x, x, buf, 2, 12, 36, 64, 64, SPLIT | XPRE | DPRE, buf, big, am, am, nullptr, nullptr));
    report("xpre_4gib", egz_conv3x3_wgrad(x, x, buf, 32, 224, 224, 1024, 64, SPLIT | XPRE, buf, big, am, am, nullptr, nullptr));
    report("ws_small", egz_conv3x3_wgrad(x, x, buf, 2, 16, 16, 64, 64, SPLIT, buf,
                                         egz_conv3x3_wgrad_ws_bytes(2, 16, 16, 64, 64, SPLIT) - 4, am, am, nullptr, nullptr));
    report("ws_small_ups_f32", egz_conv3x3_wgrad(x, x, buf, 2, 16, 64, 64, 64, 1, buf,
                                                 egz_conv3x3_wgrad_ws_bytes(2, 16, 64, 64, 64, 1) - 4, nullptr, nullptr, nullptr, nullptr));

    FILE* out = argc > 1 ? fopen(argv[1], "wb") : nullptr;
    if (!out) { fprintf(stderr, "usage: %s <sweep file>\n", argv[0]); return 2; }
    long calls = 0, wrong = 0;
    auto point = [&](int B, int H, int W, int C, int K, int flags) {
        const uint64_t nb = egz_conv3x3_wgrad_ws_bytes(B, H, W, C, K, flags);
        const int32_t rec[6] = {B, H, W, C, K, flags};
        fwrite(rec, sizeof rec, 1, out);
        fwrite(&nb, sizeof nb, 1, out);
        for (int f16 = 0; f16 < 2; ++f16) {
            const unsigned int* a = f16 ? am : nullptr;
            const int rc = egz_conv3x3_wgrad(x, x, buf, B, H, W, C, K, flags, buf, (size_t)nb - 4, a, a, nullptr, nullptr);
            ++calls;
            if (rc != 1 || strcmp(egz_last_error(), "egz_conv3x3_wgrad: workspace too small") != 0) {
                if (!wrong++) fprintf(stderr, "B=%d H=%d W=%d C=%d K=%d flags=0x%x ws_bytes=%llu f16=%d: rc %d \"%s\"\n", B, H, W, C, K,
                                      flags, (unsigned long long)nb, f16, rc, egz_last_error());
                if (rc == 0) exit(3);                           // accepted: the next such call could reach a launch
            }
            egz_set_error("%s", "");
        }
    };
    const int Bs[] = {1, 2, 32}, Cs[] = {4, 8, 12, 32, 64, 128, 192, 512}, Ks[] = {4, 8, 16, 32, 64, 128, 512};
    const int HW[][2] = {{1, 16}, {2, 2}, {7, 8}, {8, 32}, {14, 14}, {16, 16}, {28, 28}, {10, 48}, {32, 32}, {56, 56}, {6, 96},
                         {112, 112}, {224, 224}, {33, 224}, {12, 12}, {9, 7}};
    const int variants[] = {0, 0x800, 0x1000, 0x100, 0x4000};
    for (int B : Bs)
        for (auto& hw : HW)
            for (int C : Cs)
                for (int K : Ks)
                    for (int base : {0, SPLIT})
                        for (int ups = 0; ups < 2; ++ups) {
                            if (ups && (hw[0] % 2 || hw[1] % 2)) continue;
                            for (int v : variants) point(B, hw[0], hw[1], C, K, base | ups | v);
                        }
    for (int base : {0, SPLIT})             // an operand of 4 GiB or more: the split-half request falls back to the f32 kernels
        for (int ups = 0; ups < 2; ++ups) point(32, 224, 224, 1024, 64, base | ups);
    fclose(out);
    printf("short4\t%ld\t%ld\n", calls, wrong);
    return bad;
}
