// Host-only build of csrc/bn_pool.hip and csrc/conv_first.hip for tests/test_bn_dispatch_host.py (-fsanitize=address,undefined
// on the host side).  Uses the public entry points only.  Three parts:
//   guard <name> <rc> <msg>   an entry point called with arguments one of its guards rejects, and the error the call left behind
//   sweep file (argv[1])      the size queries over their grids: records of 6 int32 (query, then its arguments, zero-padded) +
//                             1 uint64 (the value), compared with tests/golden/bn_host_sizes.npz
//   short8 <calls> <bad>      at every point of the sweep, each entry point that takes that workspace, given 8 bytes less than
//                             it needs: bad counts the calls not rejected with its "workspace too small" message
// No call gets as far as a launch, so no GPU is needed; the pointers are never dereferenced.
#include "bn_pool.hip"
#include "conv_first.hip"
#include "egz_core.hip"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

enum Query { BN_WS, BN_BWD_WS, RELU_BIAS_WS, FIRST_BWD_WS, FIRST_WGRAD_WS, FIRST_STAT_ROWS };

int main(int argc, char** argv) {
    static float buf[4];
    static double dbuf[4];
    static unsigned int am[4];
    static long long nbt[1];
    float* const F = buf;
    float* const NF = nullptr;
    double* const D = dbuf;
    unsigned int* const U = am;
    unsigned int* const NU = nullptr;
    const size_t big = (size_t)1 << 40;
    int bad = 0;
    auto report = [&](const char* name, int rc) {
        printf("guard\t%s\t%d\t%s\n", name, rc, egz_last_error());
        if (rc == 0) bad = 1;               // accepted: the entry point would have launched
        egz_set_error("%s", "");
    };
    const size_t fin_ws = (size_t)egz_channel_stats_rows() * 2 * 64 * sizeof(double);      // what a finalize of K = 64 needs

    //                                    stat rows K  count g  b  rm  rv mom   eps    mean istd scale shift nbt  ws ws_bytes
    report("fin_null_stat", egz_bn_finalize(nullptr, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, nullptr));
    report("fin_null_shift", egz_bn_finalize(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, NF, nbt, D, big, nullptr));
    report("fin_null_ws", egz_bn_finalize(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, nullptr, big, nullptr));
    report("fin_ws_small", egz_bn_finalize(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, fin_ws - 8, nullptr));
    report("fin_unpaired", egz_bn_finalize(D, 3, 64, 8., F, F, F, NF, .1f, 1e-5f, F, F, F, F, nbt, D, big, nullptr));
    report("finb_null_stat", egz_bn_finalize_bound(nullptr, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, U, U, nullptr));
    report("finb_null_minmax", egz_bn_finalize_bound(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, NU, U, nullptr));
    report("finb_null_absmax", egz_bn_finalize_bound(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, U, NU, nullptr));
    report("finb_k32", egz_bn_finalize_bound(D, 3, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, U, U, nullptr));
    report("finb_ws_small", egz_bn_finalize_bound(D, 3, 64, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, fin_ws - 8, U, U, nullptr));
    report("finb_unpaired", egz_bn_finalize_bound(D, 3, 64, 8., F, F, NF, F, .1f, 1e-5f, F, F, F, F, nbt, D, big, U, U, nullptr));
    //                                                                                                      minmax mm_rows absmax
    report("find_null_stat", egz_bn_finalize_deferred(nullptr, 3, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, F, 3, U, nullptr));
    report("find_null_minmax", egz_bn_finalize_deferred(D, 3, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, NF, 3, U, nullptr));
    report("find_null_absmax", egz_bn_finalize_deferred(D, 3, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, F, 3, NU, nullptr));
    report("find_k128", egz_bn_finalize_deferred(D, 3, 128, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, F, 3, U, nullptr));
    report("find_rows0", egz_bn_finalize_deferred(D, 0, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, F, 3, U, nullptr));
    report("find_mm_rows0", egz_bn_finalize_deferred(D, 3, 32, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, F, 0, U, nullptr));
    report("find_unpaired", egz_bn_finalize_deferred(D, 3, 32, 8., F, F, F, NF, .1f, 1e-5f, F, F, F, F, nbt, F, 3, U, nullptr));
    report("eval_null_mean", egz_bn_eval_coeffs(64, F, F, NF, F, 1e-5f, F, F, nullptr));
    report("eval_null_shift", egz_bn_eval_coeffs(64, F, F, F, F, 1e-5f, F, NF, nullptr));

    //                                         y scale shift out B  H  W   K  pool absmax
    report("fwd_null_y", egz_bn_relu_pool_fwd(NF, F, F, F, 2, 4, 4, 64, 0, U, nullptr));
    report("fwd_null_out", egz_bn_relu_pool_fwd(F, F, F, NF, 2, 4, 4, 64, 0, U, nullptr));
    report("fwd_k6", egz_bn_relu_pool_fwd(F, F, F, F, 2, 4, 4, 6, 0, U, nullptr));
    report("fwd_pool_odd_h", egz_bn_relu_pool_fwd(F, F, F, F, 2, 5, 4, 64, 1, U, nullptr));
    report("fwd_pool_odd_w", egz_bn_relu_pool_fwd(F, F, F, F, 2, 4, 5, 64, 1, U, nullptr));
    report("fwdp_null_y", egz_bn_relu_pool_fwd_presplit(NF, F, F, F, 2, 4, 4, 64, 0, U, nullptr));
    report("fwdp_null_absmax", egz_bn_relu_pool_fwd_presplit(F, F, F, F, 2, 4, 4, 64, 0, NU, nullptr));
    report("fwdp_k6", egz_bn_relu_pool_fwd_presplit(F, F, F, F, 2, 4, 4, 6, 0, U, nullptr));
    report("fwdp_pool_odd_h", egz_bn_relu_pool_fwd_presplit(F, F, F, F, 2, 5, 4, 64, 1, U, nullptr));
    report("fwdp_pool_odd_w", egz_bn_relu_pool_fwd_presplit(F, F, F, F, 2, 4, 5, 64, 1, U, nullptr));

    //                                         y dout scale shift mean istd dy dg db B  H  W   K pool ws ws_bytes absmax sums rows
    report("bwd_null_y", egz_bn_relu_pool_bwd(NF, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, U, nullptr, 0, nullptr));
    report("bwd_null_dy", egz_bn_relu_pool_bwd(F, F, F, F, F, F, NF, F, F, 2, 4, 4, 64, 0, D, big, U, nullptr, 0, nullptr));
    report("bwd_null_ws", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, nullptr, big, U, nullptr, 0, nullptr));
    report("bwd_sums_rows0", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, U, D, 0, nullptr));
    report("bwd_sums_pool", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 1, D, big, U, D, 3, nullptr));
    report("bwd_k6", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 6, 0, D, big, U, nullptr, 0, nullptr));
    report("bwd_k1028", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 1028, 0, D, big, U, nullptr, 0, nullptr));
    report("bwd_pool_odd_h", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 5, 4, 64, 1, D, big, U, nullptr, 0, nullptr));
    report("bwd_pool_odd_w", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 5, 64, 1, D, big, U, nullptr, 0, nullptr));
    report("bwd_ws_small", egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, egz_bn_relu_pool_bwd_ws_bytes(64) - 8,
                                                U, nullptr, 0, nullptr));
    //                                                                                                        y_minmax dout_absmax
    report("bwdp_null_absmax", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, NU, nullptr, 0, U, U, nullptr));
    report("bwdp_null_minmax", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, U, nullptr, 0, NU, U, nullptr));
    report("bwdp_null_dout_absmax", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, U, nullptr, 0, U, NU, nullptr));
    report("bwdp_k32", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 32, 0, D, big, U, nullptr, 0, U, U, nullptr));
    report("bwdp_k576", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 576, 0, D, big, U, nullptr, 0, U, U, nullptr));
    report("bwdp_null_y", egz_bn_relu_pool_bwd_presplit(NF, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, big, U, nullptr, 0, U, U, nullptr));
    report("bwdp_sums_pool", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 1, D, big, U, D, 3, U, U, nullptr));
    report("bwdp_pool_odd", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 5, 4, 64, 1, D, big, U, nullptr, 0, U, U, nullptr));
    report("bwdp_ws_small", egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, 64, 0, D, egz_bn_relu_pool_bwd_ws_bytes(64) - 8,
                                                          U, nullptr, 0, U, U, nullptr));

    //                                         y dout scale shift mean istd x dw dg db B  H  W  C   K  ws ws_bytes sums rows
    report("fwg_null_x", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, NF, F, F, F, 2, 4, 4, 2, 32, D, big, nullptr, 0, nullptr));
    report("fwg_null_dw", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, NF, F, F, 2, 4, 4, 2, 32, D, big, nullptr, 0, nullptr));
    report("fwg_null_ws", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 2, 32, nullptr, big, nullptr, 0, nullptr));
    report("fwg_k16", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 2, 16, D, big, nullptr, 0, nullptr));
    report("fwg_c4", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 4, 64, D, big, nullptr, 0, nullptr));
    report("fwg_c0", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 0, 32, D, big, nullptr, 0, nullptr));
    report("fwg_b0", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 0, 4, 4, 2, 32, D, big, nullptr, 0, nullptr));
    report("fwg_w0", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 0, 2, 32, D, big, nullptr, 0, nullptr));
    report("fwg_2gi", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 1024, 256, 256, 2, 32, D, big, nullptr, 0, nullptr));
    report("fwg_sums_rows0", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 2, 32, D, big, D, 0, nullptr));
    report("fwg_ws_small", egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, 2, 32, D,
                                                  egz_bn_bwd_first_wgrad_ws_bytes(2, 32) - 8, nullptr, 0, nullptr));

    //                                          out dout dy db rows K  ws ws_bytes absmax
    report("rbb_null_db", egz_relu_bwd_bias(F, F, F, NF, 32, 64, D, big, U, nullptr));
    report("rbb_null_ws", egz_relu_bwd_bias(F, F, F, F, 32, 64, nullptr, big, U, nullptr));
    report("rbb_k6", egz_relu_bwd_bias(F, F, F, F, 32, 6, D, big, U, nullptr));
    report("rbb_k1028", egz_relu_bwd_bias(F, F, F, F, 32, 1028, D, big, U, nullptr));
    report("rbb_ws_small", egz_relu_bwd_bias(F, F, F, F, 32, 64, D, egz_relu_bwd_bias_ws_bytes(64) - 8, U, nullptr));
    report("colsum_null_x", egz_colsum(NF, 32, 64, F, D, big, nullptr));
    report("colsum_null_ws", egz_colsum(F, 32, 64, F, nullptr, big, nullptr));
    report("colsum_ws_small", egz_colsum(F, 32, 64, F, D, (size_t)egz_channel_stats_rows() * 64 * sizeof(double) - 8, nullptr));
    //                                            part rows cols nout out ws ws_bytes
    report("colsum64_null_part", egz_colsum_f64(nullptr, 3, 64, 32, F, D, big, nullptr));
    report("colsum64_null_ws", egz_colsum_f64(D, 3, 64, 32, F, nullptr, big, nullptr));
    report("colsum64_rows0", egz_colsum_f64(D, 0, 64, 32, F, D, big, nullptr));
    report("colsum64_cols0", egz_colsum_f64(D, 3, 0, 0, F, D, big, nullptr));
    report("colsum64_nout0", egz_colsum_f64(D, 3, 64, 0, F, D, big, nullptr));
    report("colsum64_nout_wide", egz_colsum_f64(D, 3, 64, 65, F, D, big, nullptr));
    report("colsum64_ws_small", egz_colsum_f64(D, 3, 64, 32, F, D, (size_t)egz_channel_stats_rows() * 64 * sizeof(double) - 8, nullptr));

    //                                        x  w bias y stat B  H  W  C   K  minmax_out minmax_ordered
    report("cff_null_x", egz_conv_first_fwd(NF, F, F, F, D, 2, 4, 4, 3, 64, NF, NU, nullptr));
    report("cff_null_y", egz_conv_first_fwd(F, F, F, NF, D, 2, 4, 4, 3, 64, NF, NU, nullptr));
    report("cff_mm_no_stat", egz_conv_first_fwd(F, F, F, F, nullptr, 2, 4, 4, 2, 32, F, NU, nullptr));
    report("cff_mmo_no_stat", egz_conv_first_fwd(F, F, F, F, nullptr, 2, 4, 4, 2, 32, NF, U, nullptr));
    report("cff_mm_c20", egz_conv_first_fwd(F, F, F, F, D, 2, 4, 4, 20, 64, F, NU, nullptr));
    report("cff_mm_2gi", egz_conv_first_fwd(F, F, F, F, D, 1024, 256, 256, 2, 32, F, NU, nullptr));
    report("cff_k16", egz_conv_first_fwd(F, F, F, F, D, 2, 4, 4, 3, 16, NF, NU, nullptr));
    report("cff_c0", egz_conv_first_fwd(F, F, F, F, D, 2, 4, 4, 0, 64, NF, NU, nullptr));
    report("cff_c65", egz_conv_first_fwd(F, F, F, F, D, 2, 4, 4, 65, 64, NF, NU, nullptr));
    report("cff_h0", egz_conv_first_fwd(F, F, F, F, D, 2, 0, 4, 3, 64, NF, NU, nullptr));
    //                                           x dy dw B  H  W  C   K  ws ws_bytes
    report("cfw_null_dy", egz_conv_first_wgrad(F, NF, F, 2, 4, 4, 3, 64, F, big, nullptr));
    report("cfw_null_ws", egz_conv_first_wgrad(F, F, F, 2, 4, 4, 3, 64, nullptr, big, nullptr));
    report("cfw_k16", egz_conv_first_wgrad(F, F, F, 2, 4, 4, 3, 16, F, big, nullptr));
    report("cfw_c4", egz_conv_first_wgrad(F, F, F, 2, 4, 4, 4, 64, F, big, nullptr));
    report("cfw_c22", egz_conv_first_wgrad(F, F, F, 2, 4, 4, 22, 64, F, big, nullptr));
    report("cfw_ws_small", egz_conv_first_wgrad(F, F, F, 2, 4, 4, 3, 64, F, egz_conv_first_wgrad_ws_bytes(2, 4, 4, 3) - 8, nullptr));

    FILE* out = argc > 1 ? fopen(argv[1], "wb") : nullptr;
    if (!out) { fprintf(stderr, "usage: %s <sweep file>\n", argv[0]); return 2; }
    long calls = 0, wrong = 0;
    auto record = [&](int query, int a0, int a1, int a2, int a3, int a4, uint64_t value) {
        const int32_t rec[6] = {query, a0, a1, a2, a3, a4};
        fwrite(rec, sizeof rec, 1, out);
        fwrite(&value, sizeof value, 1, out);
    };
    // a call that was handed 8 bytes less than it needs: rejected, with `msg`
    auto short8 = [&](const char* what, int a0, int a1, int rc, const std::string& msg) {
        ++calls;
        if (rc != 1 || msg != egz_last_error()) {
            if (!wrong++) fprintf(stderr, "%s(%d, %d): rc %d \"%s\", expected \"%s\"\n", what, a0, a1, rc, egz_last_error(), msg.c_str());
            if (rc == 0) exit(3);                               // accepted: the next such call could reach a launch
        }
        egz_set_error("%s", "");
    };
    auto sized = [](const char* who, size_t have, size_t need) {           // the two messages that state the sizes
        char m[160];
        snprintf(m, sizeof m, "%s: workspace too small (%zu < %zu)", who, have, need);
        return std::string(m);
    };
    const size_t red_rows = (size_t)egz_channel_stats_rows();
    for (int K = 4; K <= 1024; K += 4) {
        record(BN_WS, K, 0, 0, 0, 0, egz_bn_ws_bytes(K));
        // the forward finalize folds into RED_ROWS rows of (sum, sum of squares): what it needs of the egz_bn_ws_bytes buffer
        const size_t fin = red_rows * 2 * K * sizeof(double) - 8;
        short8("egz_bn_finalize", K, 0, egz_bn_finalize(D, 3, K, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, fin, nullptr),
               "egz_bn_finalize: workspace too small");
        if (K % 64 == 0)
            short8("egz_bn_finalize_bound", K, 0,
                   egz_bn_finalize_bound(D, 3, K, 8., F, F, F, F, .1f, 1e-5f, F, F, F, F, nbt, D, fin, U, U, nullptr),
                   "egz_bn_finalize_bound: workspace too small");
        const size_t col = red_rows * K * sizeof(double) - 8;                // egz_colsum / egz_colsum_f64: RED_ROWS rows of K
        short8("egz_colsum", K, 0, egz_colsum(F, 32, K, F, D, col, nullptr), "egz_colsum: workspace too small");
        short8("egz_colsum_f64", K, 0, egz_colsum_f64(D, 3, K, K, F, D, col, nullptr), "egz_colsum_f64: workspace too small");

        const size_t nb = egz_bn_relu_pool_bwd_ws_bytes(K);
        record(BN_BWD_WS, K, 0, 0, 0, 0, nb);
        const std::string small = sized("egz_bn_relu_pool_bwd", nb - 8, nb);
        for (int with_sums = 0; with_sums < 2; ++with_sums) {
            const double* sums = with_sums ? D : nullptr;
            short8("egz_bn_relu_pool_bwd", K, with_sums,
                   egz_bn_relu_pool_bwd(F, F, F, F, F, F, F, F, F, 2, 4, 4, K, 0, D, nb - 8, U, sums, 3 * with_sums, nullptr), small);
            if (K % 64 == 0 && K <= 512)
                short8("egz_bn_relu_pool_bwd_presplit", K, with_sums,
                       egz_bn_relu_pool_bwd_presplit(F, F, F, F, F, F, F, F, F, 2, 4, 4, K, 0, D, nb - 8, U, sums, 3 * with_sums, U, U,
                                                     nullptr), small);
        }
        const size_t rb = egz_relu_bwd_bias_ws_bytes(K);
        record(RELU_BIAS_WS, K, 0, 0, 0, 0, rb);
        short8("egz_relu_bwd_bias", K, 0, egz_relu_bwd_bias(F, F, F, F, 32, K, D, rb - 8, U, nullptr),
               "egz_relu_bwd_bias: workspace too small");
    }
    for (int C = 1; C <= 3; ++C)
        for (int K : {32, 64}) {
            const size_t nb = egz_bn_bwd_first_wgrad_ws_bytes(C, K);
            record(FIRST_BWD_WS, C, K, 0, 0, 0, nb);
            for (int with_sums = 0; with_sums < 2; ++with_sums)
                short8("egz_bn_bwd_first_wgrad", C, K,
                       egz_bn_bwd_first_wgrad(F, F, F, F, F, F, F, F, F, F, 2, 4, 4, C, K, D, nb - 8, with_sums ? D : nullptr,
                                              3 * with_sums, nullptr), sized("egz_bn_bwd_first_wgrad", nb - 8, nb));
        }
    const int Bs[] = {1, 2, 32}, Cs[] = {1, 2, 3, 4, 18, 20, 21, 64};
    const int HW[][2] = {{1, 16}, {2, 2}, {9, 7}, {9, 13}, {12, 16}, {16, 18}, {32, 32}, {48, 48}, {33, 224}, {224, 224}, {512, 512},
                         {1024, 1024}};
    for (int B : Bs)
        for (auto& hw : HW)
            for (int C : Cs) {
                const int H = hw[0], W = hw[1];
                const size_t nb = egz_conv_first_wgrad_ws_bytes(B, H, W, C);
                record(FIRST_WGRAD_WS, B, H, W, C, 0, nb);
                for (int K : {32, 64}) {
                    record(FIRST_STAT_ROWS, B, H, W, C, K, (uint64_t)egz_conv_first_stat_rows_for(B, H, W, C, K));
                    if (C > 3 && (C < 18 || C > 21)) continue;             // no weight-gradient kernel for this Cin
                    // the query is sized for 64 filters: 32 filters on Cin = 18..21 (one partial row per split) need half of it
                    const size_t need = (K == 32 && C > 3) ? nb / 2 : nb;
                    short8("egz_conv_first_wgrad", C, K, egz_conv_first_wgrad(F, F, F, B, H, W, C, K, F, need - 8, nullptr),
                           "egz_conv_first_wgrad: workspace too small");
                }
            }
    fclose(out);
    printf("short8\t%ld\t%ld\n", calls, wrong);
    return bad;
}
