// egz_lstm_pool_fetch (data/lstm_resident.py, `--lstm_resident`): one step of AT.trainLSTM / AT.testLSTM fed from a pool of the
// extracted fixation vectors that stays in HBM.  The step plan -- which pool row is the input, which the target, and whether the
// LSTM state is reset first -- is the file loop's own schedule run over the file names (data/lstm_resident.lstm_plan), so the launch
// takes its step number from a cursor on the device and sits at the head of the step's captured hipGraph: a replay needs nothing
// from the host.
//   pool    (rows, width) fp32
//   in_row, tgt_row (n_steps,) int32 pool rows; reset (n_steps,) uint8
//   cursor  {next step, step being run}: cursor[0] is read by every thread, then advanced by one; cursor[1] names the step to
//           the later kernels of the same replay (egz_mse_fwd_grad parks its loss in ring[cursor[1] % ring_n])
// ONE block: 2 x width floats are copied and state_n floats zeroed (6 KB at the AT geometry), the launch is latency bound, and
// a single block lets __syncthreads() order every thread's read of cursor[0] before the one store that advances it.
// Nothing is clamped.  A cursor outside the plan (status bit 0) or a plan row outside the pool (bit 1) is refused before anything
// is dereferenced with it: nothing is written but the sticky OR into *status, and the cursor stays where it is.
#include "egz_common.h"

namespace {

__device__ __forceinline__ bool lp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// dst[0 .. n) = src[0 .. n) by the whole block: float4 body where both pointers are 16-byte aligned (block-uniform), scalar tail
__device__ __forceinline__ void lp_copy(float* __restrict__ dst, const float* __restrict__ src, int n) {
    int done = 0;
    if (lp_aligned16(dst) && lp_aligned16(src)) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += blockDim.x)
            reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

__device__ __forceinline__ void lp_zero(float* __restrict__ dst, long n) {
    long done = 0;
    if (lp_aligned16(dst)) {
        const long n4 = n >> 2;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (long i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4*>(dst)[i] = z;
        done = n4 << 2;
    }
    for (long i = done + threadIdx.x; i < n; i += blockDim.x) dst[i] = 0.f;
}

__global__ __launch_bounds__(256) void lstm_pool_fetch_kernel(const float* __restrict__ pool, long rows, int width,
                                                              const int* __restrict__ in_row, const int* __restrict__ tgt_row,
                                                              const unsigned char* __restrict__ reset, long n_steps,
                                                              int* cursor, float* __restrict__ inp, float* __restrict__ tgt,
                                                              float* __restrict__ state, long state_n, unsigned int* status) {
    const int k = *static_cast<const volatile int*>(cursor);
    // bounds (block-uniform): nothing below dereferences an index that failed
    unsigned int bad = 0;
    int ri = 0, rt = 0;
    if (k < 0 || (long)k >= n_steps) {
        bad = 1;
    } else {
        ri = in_row[k];
        rt = tgt_row[k];
        if (ri < 0 || (long)ri >= rows || rt < 0 || (long)rt >= rows) bad = 2;
    }
    __syncthreads();                          // every thread holds its copy of cursor[0]: thread 0 may advance it below
    if (bad) {
        if (threadIdx.x == 0) atomicOr(status, bad);
        return;
    }
    lp_copy(inp, pool + (long)ri * width, width);
    lp_copy(tgt, pool + (long)rt * width, width);
    if (state && reset[k]) lp_zero(state, state_n);
    if (threadIdx.x == 0) {
        cursor[1] = k;
        cursor[0] = k + 1;
    }
}

}  // namespace

// state may be null (no state to reset); status is sticky: the caller zero-fills it once and reads it where it synchronises anyway.
EGZ_API int egz_lstm_pool_fetch(const float* pool, long rows, int width, const int* in_row, const int* tgt_row,
                                const unsigned char* reset, long n_steps, int* cursor, float* inp, float* tgt, float* state,
                                long state_n, unsigned int* status, hipStream_t st) {
    EGZ_CHECK_ARG(pool, "egz_lstm_pool_fetch: pool is null");
    EGZ_CHECK_ARG(in_row && tgt_row && reset, "egz_lstm_pool_fetch: a plan array (in_row / tgt_row / reset) is null");
    EGZ_CHECK_ARG(cursor, "egz_lstm_pool_fetch: cursor is null");
    EGZ_CHECK_ARG(inp && tgt, "egz_lstm_pool_fetch: inp / tgt is null");
    EGZ_CHECK_ARG(status, "egz_lstm_pool_fetch: status is null");
    EGZ_CHECK_ARG(width >= 1 && width <= 4096, "egz_lstm_pool_fetch: width = %d outside 1 .. 4096 (egz_mse_fwd_grad's limit)", width);
    EGZ_CHECK_ARG(rows >= 1 && n_steps >= 1, "egz_lstm_pool_fetch: rows = %ld, n_steps = %ld: both must be positive", rows, n_steps);
    EGZ_CHECK_ARG(state_n >= 0, "egz_lstm_pool_fetch: state_n = %ld is negative", state_n);
    hipLaunchKernelGGL(lstm_pool_fetch_kernel, dim3(1), dim3(256), 0, st, pool, rows, width, in_row, tgt_row, reset, n_steps,
                       cursor, inp, tgt, state, state_n, status);
    EGZ_CHECK_LAUNCH("egz_lstm_pool_fetch");
    return 0;
}
