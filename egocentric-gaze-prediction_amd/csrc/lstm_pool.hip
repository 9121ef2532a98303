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
//
// egz_lstm_store (extractLSTMw.extractw(into=...), `gaze_full --lstm_handover`): the other end of the same pool.  One block per
// sample of an encoder forward turns the sample's ground-truth plane (a plane of the resident ST pool) into the gaze cell, the
// cell into extractLSTMw.var_window's window, and the window of the conv5_3 map into the pool row the file path would have
// written to fix_<name>.pth.tar and read back.  The gaze cell is the FIRST arg-max of avg_pool2d(u8 / 255, cell) as ATen's CPU
// kernel computes it: per cell a sequential fp32 sum of u / 255.f in row-major order, then one divide by cell^2.  Blobs centred
// on a cell corner tie in their exact sums and differ in the last bit of these fp32 sums, so any other order (integer sums, a
// tree, row sums) picks another cell on most of them: the order is restated, not improved.  u / 255.f comes from a 256-entry
// table in LDS (the same correctly rounded divide, done once per byte value instead of once per pixel).
#include "egz_common.h"
#include "window_mean.h"

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

constexpr int LS_NT = 256;

// (score a, cell a) beats (score b, cell b): the higher score, and on equal scores the lower cell -- torch.max's first maximum
__device__ __forceinline__ bool ls_beats(float sa, int ca, float sb, int cb) { return sa > sb || (sa == sb && ca < cb); }

// s + the sixteen bytes of q in address order, one fp32 add each
__device__ __forceinline__ float ls_add16(float s, const uint4 q, const float* unit) {
    const unsigned int w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 16; ++e) s += unit[(w4[e >> 2] >> (8 * (e & 3))) & 255u];
    return s;
}

// one block per sample.  feat (B, H, H, C) channels-last; gt_pool (Q, H cell, H cell) uint8; pool (rows, C).
__global__ __launch_bounds__(LS_NT) void lstm_store_kernel(const float* __restrict__ feat, int H, int C,
                                                           const unsigned char* __restrict__ gt_pool, long Q,
                                                           const long* __restrict__ gt_src, int cell, int size,
                                                           float* __restrict__ pool, long rows, const long* __restrict__ dst,
                                                           int* __restrict__ cells, unsigned int* status) {
    __shared__ float unit[256];               // unit[u] = (float)u / 255.f
    __shared__ float red_s[LS_NT / 64];
    __shared__ int red_c[LS_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, W = H;
    // bounds (block-uniform): a skipped sample reads nothing of its own, a number that failed is never turned into an address
    const long row = dst[b];
    if (row == -1) return;
    const long src = gt_src[b];
    if (row < -1 || row >= rows || src < 0 || src >= Q) {
        if (tid == 0) atomicOr(status, 1u);
        return;
    }
    unit[tid] = (float)tid / 255.f;
    __syncthreads();

    // cell scores: one thread per feature cell, the cell's bytes in row-major order (16 at a time where the row is aligned)
    const long pw = (long)W * cell;           // bytes per row of a plane
    const unsigned char* plane = gt_pool + src * ((long)H * cell * pw);
    float best = -1.f;                        // (every score is >= 0: a thread without a cell loses to any thread with one)
    int best_c = 0x7fffffff;
    for (int k = tid; k < H * W; k += LS_NT) {
        const unsigned char* p = plane + (long)(k / W) * cell * pw + (long)(k % W) * cell;
        float s = 0.f;
        if (cell == 16 && ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)pw) & 15) == 0) {
            // the AT geometry: the cell's sixteen rows are sixteen independent 16-byte loads, all in flight before the first
            // add (one memory latency instead of sixteen); the adds keep their order
            uint4 q[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) q[r] = *reinterpret_cast<const uint4*>(p + r * pw);
#pragma unroll
            for (int r = 0; r < 16; ++r) s = ls_add16(s, q[r], unit);
        } else {
            for (int r = 0; r < cell; ++r, p += pw) {
                int x = 0;
                if (lp_aligned16(p))
                    for (; x + 16 <= cell; x += 16) s = ls_add16(s, *reinterpret_cast<const uint4*>(p + x), unit);
                for (; x < cell; ++x) s += unit[p[x]];
            }
        }
        s = s / (float)(cell * cell);
        if (ls_beats(s, k, best, best_c)) {
            best = s;
            best_c = k;
        }
    }

    // arg-max over the block: butterfly inside a wave (every lane ends with the wave's winner), then the four waves through LDS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(best, off);
        const int oc = __shfl_xor(best_c, off);
        if (ls_beats(os, oc, best, best_c)) {
            best = os;
            best_c = oc;
        }
    }
    if ((tid & 63) == 0) {
        red_s[tid >> 6] = best;
        red_c[tid >> 6] = best_c;
    }
    __syncthreads();
    best = red_s[0];
    best_c = red_c[0];
#pragma unroll
    for (int w = 1; w < LS_NT / 64; ++w)
        if (ls_beats(red_s[w], red_c[w], best, best_c)) {
            best = red_s[w];
            best_c = red_c[w];
        }

    // extractLSTMw.var_window: float clip, then truncation of both bounds; both coordinates are clipped with H.  Every value is
    // a small multiple of 0.5, exact in fp32 as in the reference's doubles; 1 <= size <= H keeps the window inside the map.
    const float half = 0.5f * (float)size;
    const int up = (size + 1) / 2;            // ceil(size / 2)
    const float fy = fminf(fmaxf((float)(best_c / W), half), (float)(H - up));
    const float fx = fminf(fmaxf((float)(best_c % W), half), (float)(H - up));
    const int y0 = (int)(fy - half), y1 = (int)(fy + (float)up), x0 = (int)(fx - half), x1 = (int)(fx + (float)up);
    if (tid == 0 && cells) cells[b] = best_c;
    for (int c = tid; c < C; c += LS_NT) pool[row * C + c] = egz_window_mean_at(feat, b, H, W, C, c, y0, y1, x0, x1);
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

// cells may be null (the chosen cells are not reported); status is sticky as above.  H == W: the reference clips both window
// coordinates with H.
EGZ_API int egz_lstm_store(const float* feat, int B, int H, int W, int C, const unsigned char* gt_pool, long Q, const long* gt_src,
                           int cell, int size, float* pool, long rows, const long* dst, int* cells, unsigned int* status,
                           hipStream_t st) {
    EGZ_CHECK_ARG(feat, "egz_lstm_store: feat is null");
    EGZ_CHECK_ARG(gt_pool && gt_src, "egz_lstm_store: gt_pool / gt_src is null");
    EGZ_CHECK_ARG(pool && dst, "egz_lstm_store: pool / dst is null");
    EGZ_CHECK_ARG(status, "egz_lstm_store: status is null");
    EGZ_CHECK_ARG(B >= 1 && B <= 65535, "egz_lstm_store: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H >= 1 && H == W, "egz_lstm_store: a %d x %d map: H == W >= 1 is needed (both window coordinates are clipped with H)", H, W);
    EGZ_CHECK_ARG(H <= 1024, "egz_lstm_store: H = %d above 1024", H);
    EGZ_CHECK_ARG(C >= 1, "egz_lstm_store: C = %d is not positive", C);
    EGZ_CHECK_ARG(cell >= 1 && cell <= 256, "egz_lstm_store: cell = %d outside 1 .. 256", cell);
    EGZ_CHECK_ARG(size >= 1 && size <= H, "egz_lstm_store: size = %d outside 1 .. H = %d", size, H);
    EGZ_CHECK_ARG(Q >= 1 && rows >= 1, "egz_lstm_store: Q = %ld, rows = %ld: both must be positive", Q, rows);
    hipLaunchKernelGGL(lstm_store_kernel, dim3(B), dim3(LS_NT), 0, st, feat, H, C, gt_pool, Q, gt_src, cell, size, pool, rows, dst,
                       cells, status);
    EGZ_CHECK_LAUNCH("egz_lstm_store");
    return 0;
}
