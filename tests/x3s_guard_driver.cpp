// Host-only build of csrc/conv3x3_igemm_x3s.hip for tests/test_x3s_dispatch_host.py (-fsanitize=address,undefined on the
// host side): calls egz_conv3x3_fwd_streamed with arguments every guard of its dispatch rejects and prints the error each
// call left behind.  No call gets as far as a launch, so no GPU is needed; the pointers are never dereferenced.
#include "conv3x3_igemm_x3s.hip"
#include "egz_core.hip"
#include <cstdio>

int main() {
    static float buf[4];
    static double stat[4];
    static unsigned int am[4];
    const float* x = buf;
    const void* wq = buf;
    int bad = 0;
    auto report = [&](const char* name, int rc) {
        printf("%s\t%d\t%s\n", name, rc, egz_last_error());
        if (rc == 0) bad = 1;               // accepted: the dispatch would have launched
        egz_set_error("%s", "");
    };
    //                                 x  wq  bias  y    stat  B  H   W   C   K   epi dtype mode   x_absmax mask absmax_out bn    minmax st
    report("null", egz_conv3x3_fwd_streamed(nullptr, wq, nullptr, buf, nullptr, 2, 16, 16, 32, 128, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("bf16_p2", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, nullptr, 2, 16, 16, 32, 128, 0, 0x12, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("pre_epi1", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, nullptr, 2, 16, 16, 32, 128, 1, 1, 0x100, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("pre_bf16", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 16, 16, 32, 128, 2, 2, 0x100, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("pre_k32", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 16, 16, 32, 32, 2, 1, 0x100, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("mask_32col", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 10, 12, 32, 8, 3, 1, 0, am, buf, am, nullptr, nullptr, nullptr));
    report("mask_narrow_geometry", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 16, 16, 32, 32, 3, 2, 0, nullptr, buf, am, nullptr, nullptr, nullptr));
    report("mask_no_src", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 16, 16, 32, 128, 3, 1, 0, am, nullptr, am, nullptr, nullptr, nullptr));
    report("bnsums_mode1", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 32, 32, 32, 128, 5, 1, 1, am, buf, nullptr, buf, nullptr, nullptr));
    report("bnsums_32col", egz_conv3x3_fwd_streamed(x, wq, nullptr, buf, stat, 2, 10, 12, 32, 8, 5, 1, 0, am, buf, nullptr, buf, nullptr, nullptr));
    report("upsf_stats", egz_conv3x3_fwd_streamed(x, wq, buf, buf, stat, 2, 32, 32, 32, 64, 2, 1, 2, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("upsf_stats_k128", egz_conv3x3_fwd_streamed(x, wq, buf, buf, stat, 2, 32, 32, 32, 128, 2, 1, 2, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("upsf_bf16", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 32, 32, 32, 64, 1, 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("stats_no_rows", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 16, 16, 32, 128, 2, 1, 0, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("geometry", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 16, 16, 30, 128, 0, 1, 0, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("bad_epi", egz_conv3x3_fwd_streamed(x, wq, buf, buf, stat, 2, 16, 16, 32, 128, 4, 1, 0, am, nullptr, nullptr, nullptr, nullptr, nullptr));
    report("absmax_32col", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 10, 12, 32, 8, 1, 1, 0, am, nullptr, am, nullptr, nullptr, nullptr));
    report("bn_in_wide", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 16, 16, 32, 128, 0, 1, 0, am, nullptr, nullptr, buf, nullptr, nullptr));
    report("minmax_epi0", egz_conv3x3_fwd_streamed(x, wq, buf, buf, nullptr, 2, 16, 16, 32, 128, 0, 1, 0, am, nullptr, nullptr, nullptr, buf, nullptr));
    report("splitk_epi3", egz_conv3x3_fwd_streamed_splitk(x, wq, buf, buf, stat, 1, 14, 14, 128, 128, 3, 1, am, buf, 1u << 30, 2, nullptr, nullptr));
    report("splitk_nsplit", egz_conv3x3_fwd_streamed_splitk(x, wq, buf, buf, stat, 1, 14, 14, 128, 128, 0, 1, am, buf, 1u << 30, 5, nullptr, nullptr));
    return bad;
}
