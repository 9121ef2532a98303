// The window mean of extractLSTMw.crop_feature_var + mean (extractLSTMw.py:46-58,88-90), shared by egz_window_mean (glue.hip) and
// egz_lstm_store (lstm_pool.hip): ONE definition, so that the vector the in-memory SP -> AT hand-over stores is the vector the
// file path computes, bit for bit.
#pragma once
#include "egz_common.h"

// channel c of sample b of the channels-last (B, H, W, C) map: the sequential fp32 sum over rows [y0, y1) x columns [x0, x1) in
// (y, x) order, then one divide by the number of cells
__device__ __forceinline__ float egz_window_mean_at(const float* __restrict__ feat, int b, int H, int W, int C, int c, int y0,
                                                    int y1, int x0, int x1) {
    float s = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) s += feat[(((long)b * H + y) * W + x) * C + c];
    return s / (float)((y1 - y0) * (x1 - x0));
}
