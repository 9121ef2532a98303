// egz_resident_gather (data/resident.py, `--gpu_resident`): a batch of the SP / AT sample layout built from a pool of decoded
// uint8 planes that stays in HBM.  One launch replaces, per batch, the file decode, the PCIe copy, three egz_u8_normalize
// launches, egz_nchw_to_nhwc_pad and egz_absmax: every gathered byte is read once (4 bytes per lane, 256 contiguous bytes per
// wave) and every output is written once as float4 per lane, contiguous across the wave.
//   pool   (P, H, W) uint8
//   table  (N, 22) int64 plane numbers per sample: column 0 the first of 3 consecutive BGR planes, 1 .. 20 the flow planes in
//          STdatas order (x_t, y_t, x_{t-1}, y_{t-1}, ...), 21 the ground truth
//   idx    (B,) int64 sample numbers
// A block owns 256 pixels of one sample.  Wave w takes channels w, w + 4, ... of the 24: it normalises with the reference's three
// fp32 operations (bit-identical with u8_normalize_kernel) and stores the NCHW outputs straight from registers.  The NHWC-32
// form of the flow stack is a 20-plane transpose: the block parks its 20 x 256 flow values in LDS ([channel][pixel], 16-byte
// groups XOR-swizzled by channel quad so that both the b128 writes and the transposed b32 reads are bank-conflict free) and
// then writes whole 128-byte pixel rows, 8 lanes per pixel, channels 20 .. 31 as zeros: a wave store covers 1 KiB contiguous.
// Nothing is clamped: a sample whose number, or one of whose used table entries, is out of range is skipped by its blocks (the
// decision is uniform per block) and a bit is raised in the status word.
//
// egz_late_gather (data/late_resident.py, `--late_resident`): the same for the late-fusion sample layout -- three one-channel
// maps per sample (SP prediction, AT map, ground truth), every value u8 / 255.  It shares the load and convert helpers below.
#include "egz_common.h"

namespace {

constexpr int RG_TILE = 256;                  // pixels per block
constexpr int RG_COLS = 22, RG_PLANES = 24, RG_FLOW = 20;

__device__ __forceinline__ int rg_lds_index(int c, int p) { return c * RG_TILE + (p ^ (((c >> 2) & 7) << 2)); }

// The two gathers' load and convert: 4 consecutive bytes of pool plane `plane` at pixel p (64-bit offset; p % 4 == 0 and
// HW % 4 == 0 keep the dword aligned), and byte e of them as (float)u8 / 255.f, the correctly rounded division (a multiply by
// the reciprocal differs from it at 126 of the 256 byte values).
__device__ __forceinline__ unsigned int rg_load4(const unsigned char* __restrict__ pool, long plane, long HW, long p) {
    return *reinterpret_cast<const unsigned int*>(pool + plane * HW + p);
}
__device__ __forceinline__ float rg_unit(unsigned int u, int e) { return (float)((u >> (8 * e)) & 255u) / 255.f; }

struct RgOut {
    float *image, *flow, *gt, *nhwc;
    unsigned int* absmax;
    unsigned char* raw;
    int raw_fields;
};

__global__ __launch_bounds__(256) void resident_gather_kernel(const unsigned char* __restrict__ pool, long P,
                                                              const long* __restrict__ table, long N,
                                                              const long* __restrict__ idx, long HW,
                                                              const float* __restrict__ mean, const float* __restrict__ stdv,
                                                              RgOut o, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float tile[RG_FLOW * RG_TILE];
    __shared__ float s_am[4];
    const int b = blockIdx.y;
    const long p0 = (long)blockIdx.x * RG_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // fields this launch reads: bit 0 image, bit 1 flow, bit 2 ground truth
    const int raw_fields = o.raw ? o.raw_fields : 0;
    const int used = (o.image ? 1 : 0) | ((o.flow || o.nhwc) ? 2 : 0) | (o.gt ? 4 : 0) | raw_fields;

    // bounds (block-uniform): nothing below dereferences an index that failed
    const long s = idx[b];
    if (s < 0 || s >= N) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const long* row = table + s * RG_COLS;
    bool ok = true;
    if (used & 1) ok = ok && row[0] >= 0 && row[0] <= P - 3;
    if (used & 2)
        for (int j = 1; j <= RG_FLOW; ++j) ok = ok && row[j] >= 0 && row[j] < P;
    if (used & 4) ok = ok && row[21] >= 0 && row[21] < P;
    if (!ok) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 2);
        return;
    }

    const long p = p0 + 4 * lane;             // this lane's 4 pixels (HW % 4 == 0: a group is inside the plane or outside)
    const bool live = p < HW;
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < RG_PLANES / 4; ++i) {
        const int c = wave + 4 * i;           // 0 .. 2 image, 3 .. 22 flow, 23 ground truth (wave-uniform)
        const int field = c < 3 ? 1 : (c < 23 ? 2 : 4);
        if (!(used & field) || !live) continue;
        const long plane = c < 3 ? row[0] + c : row[c - 2];
        const unsigned int u = rg_load4(pool, plane, HW, p);
        if (raw_fields & field) *reinterpret_cast<unsigned int*>(o.raw + ((long)b * RG_PLANES + c) * HW + p) = u;
        float* dst = c < 3 ? (o.image ? o.image + ((long)b * 3 + c) * HW : nullptr)
                   : c < 23 ? (o.flow ? o.flow + ((long)b * RG_FLOW + (c - 3)) * HW : nullptr)
                            : (o.gt ? o.gt + (long)b * HW : nullptr);
        const bool to_lds = field == 2 && o.nhwc;
        if (!dst && !to_lds) continue;
        const float m = mean[c], sd = stdv[c];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (rg_unit(u, e) - m) / sd;
        if (dst) *reinterpret_cast<f32x4*>(dst + p) = v;
        if (to_lds) {
            *reinterpret_cast<f32x4*>(&tile[rg_lds_index(c - 3, 4 * lane)]) = v;
            am = fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
    }
    if (!o.nhwc) return;                      // uniform
    for (int off = 32; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off));
    if (lane == 0) s_am[wave] = am;
    __syncthreads();
    // 8 lanes per pixel, a float4 of channels 4 q .. 4 q + 3 each: pixel rows of 128 bytes, contiguous from lane to lane
    float* out = o.nhwc + ((long)b * HW + p0) * 32;
#pragma unroll
    for (int it = 0; it < RG_TILE * 8 / 256; ++it) {
        const int t = it * 256 + threadIdx.x;
        const int q = t & 7, px = t >> 3;
        if (p0 + px >= HW) continue;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < RG_FLOW / 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = tile[rg_lds_index(4 * q + k, px)];
        }
        *reinterpret_cast<f32x4*>(out + (long)px * 32 + 4 * q) = v;
    }
    if (threadIdx.x == 0 && o.absmax)
        absmax_commit(o.absmax, blockIdx.y * gridDim.x + blockIdx.x,
                      fmaxf(fmaxf(s_am[0], s_am[1]), fmaxf(s_am[2], s_am[3])));
}

// ----------------------------------------------------------------------------- late fusion
// A block owns LG_TILE pixels of one sample, a lane 4 of them in each of the three planes: three independent 4-byte loads (a
// wave reads 256 contiguous bytes of each plane) are issued before the first store, then each output gets one float4 per lane
// (1 KiB contiguous per wave).  fused channel 0 is the AT map (table column 1), channel 1 the SP prediction (column 0): the
// order LF.py passes to late_fusion.
constexpr int LG_TILE = 1024;                 // pixels per block (256 lanes x 4)
constexpr int LG_COLS = 3;                    // table columns: pred, feat, gt

struct LgOut {
    float *fused, *gt;
    unsigned char* raw;
};

__global__ __launch_bounds__(256) void late_gather_kernel(const unsigned char* __restrict__ pool, long P,
                                                          const long* __restrict__ table, long N,
                                                          const long* __restrict__ idx, long HW, LgOut o,
                                                          int* __restrict__ status) {
    const int b = blockIdx.y;
    // columns this launch reads: bit 0 pred, bit 1 feat, bit 2 ground truth
    const int used = (o.fused ? 3 : 0) | (o.gt ? 4 : 0) | (o.raw ? 7 : 0);

    // bounds (block-uniform): nothing below dereferences an index that failed
    const long s = idx[b];
    if (s < 0 || s >= N) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const long* row = table + s * LG_COLS;
    long plane[LG_COLS];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < LG_COLS; ++c) {
        plane[c] = (used >> c) & 1 ? row[c] : 0;
        ok = ok && plane[c] >= 0 && plane[c] < P;
    }
    if (!ok) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 2);
        return;
    }

    const long p = (long)blockIdx.x * LG_TILE + 4 * threadIdx.x;      // this lane's 4 pixels (HW % 4 == 0: inside the plane or outside)
    if (p >= HW) return;
    unsigned int u[LG_COLS];
#pragma unroll
    for (int c = 0; c < LG_COLS; ++c) u[c] = (used >> c) & 1 ? rg_load4(pool, plane[c], HW, p) : 0u;
#pragma unroll
    for (int c = 0; c < LG_COLS; ++c) {
        if (!((used >> c) & 1)) continue;
        if (o.raw) *reinterpret_cast<unsigned int*>(o.raw + ((long)b * LG_COLS + c) * HW + p) = u[c];
        float* dst = c == 2 ? (o.gt ? o.gt + (long)b * HW : nullptr)
                            : (o.fused ? o.fused + ((long)b * 2 + (1 - c)) * HW : nullptr);
        if (!dst) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rg_unit(u[c], e);
        *reinterpret_cast<f32x4*>(dst + p) = v;
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// mean / std: 24 floats each on the device (image 3, flow 20, ground truth 1).  image (B,3,H,W), flow (B,20,H,W), gt (B,1,H,W),
// flow_nhwc32 (B,H,W,32) fp32 and raw (B,24,H,W) uint8 are optional (null: not produced, nothing written); raw_fields says which
// fields of raw are written (bit 0 image, 1 flow, 2 ground truth).  absmax: zero-filled egz_absmax buffer, receives max |flow|.
// status: one int on the device, zero-filled by the caller; bit 0 = an idx value, bit 1 = a table entry out of range (the
// sample was skipped).
EGZ_API int egz_resident_gather(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H,
                                int W, const float* mean, const float* stdv, float* image, float* flow, float* gt,
                                float* flow_nhwc32, unsigned int* absmax, unsigned char* raw, int raw_fields, int* status,
                                hipStream_t st) {
    EGZ_CHECK_ARG(pool, "egz_resident_gather: pool is null");
    EGZ_CHECK_ARG(table, "egz_resident_gather: table is null");
    EGZ_CHECK_ARG(idx, "egz_resident_gather: idx is null");
    EGZ_CHECK_ARG(mean && stdv, "egz_resident_gather: mean / std is null");
    EGZ_CHECK_ARG(status, "egz_resident_gather: status is null");
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "egz_resident_gather: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H > 0 && W > 0, "egz_resident_gather: H x W = %d x %d must be positive", H, W);
    const long HW = (long)H * W;
    EGZ_CHECK_ARG(HW % 4 == 0, "egz_resident_gather: H * W = %ld must be a multiple of 4", HW);
    EGZ_CHECK_ARG(P >= 1 && N >= 1, "egz_resident_gather: P = %ld planes, N = %ld samples: both must be positive", P, N);
    EGZ_CHECK_ARG(!raw || (raw_fields & 7) != 0 && (raw_fields & ~7) == 0,
                  "egz_resident_gather: raw_fields = %d must name at least one of image (1), flow (2), gt (4)", raw_fields);
    EGZ_CHECK_ARG(image || flow || gt || flow_nhwc32 || raw, "egz_resident_gather: no output (every output pointer is null)");
    EGZ_CHECK_ARG((flow_nhwc32 != nullptr) == (absmax != nullptr),
                  "egz_resident_gather: flow_nhwc32 and absmax go together (one is null, the other is not)");
    EGZ_CHECK_ARG(aligned_to(pool, 4) && aligned_to(raw, 4), "egz_resident_gather: pool / raw must be 4-byte aligned");
    EGZ_CHECK_ARG(aligned_to(image, 16) && aligned_to(flow, 16) && aligned_to(gt, 16) && aligned_to(flow_nhwc32, 16),
                  "egz_resident_gather: the fp32 outputs must be 16-byte aligned");
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    hipLaunchKernelGGL(resident_gather_kernel, dim3(egz_cdiv(HW, RG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx, HW,
                       mean, stdv, o, status);
    EGZ_CHECK_LAUNCH("egz_resident_gather");
    return 0;
}

// table (N, 3) int64: the plane numbers of the SP prediction, the AT map and the ground truth of a sample.  fused (B,2,H,W) fp32
// (channel 0 the AT map, channel 1 the SP prediction), gt (B,1,H,W) fp32 and raw (B,3,H,W) uint8 (table order) are optional
// (null: not produced, nothing written).  status: as above; bit 1 looks at the columns of the outputs asked for.
EGZ_API int egz_late_gather(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H, int W,
                            float* fused, float* gt, unsigned char* raw, int* status, hipStream_t st) {
    EGZ_CHECK_ARG(pool, "egz_late_gather: pool is null");
    EGZ_CHECK_ARG(table, "egz_late_gather: table is null");
    EGZ_CHECK_ARG(idx, "egz_late_gather: idx is null");
    EGZ_CHECK_ARG(status, "egz_late_gather: status is null");
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "egz_late_gather: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H > 0 && W > 0, "egz_late_gather: H x W = %d x %d must be positive", H, W);
    const long HW = (long)H * W;
    EGZ_CHECK_ARG(HW % 4 == 0, "egz_late_gather: H * W = %ld must be a multiple of 4", HW);
    EGZ_CHECK_ARG(P >= 1 && N >= 1, "egz_late_gather: P = %ld planes, N = %ld samples: both must be positive", P, N);
    EGZ_CHECK_ARG(fused || gt || raw, "egz_late_gather: no output (every output pointer is null)");
    EGZ_CHECK_ARG(aligned_to(pool, 4) && aligned_to(raw, 4), "egz_late_gather: pool / raw must be 4-byte aligned");
    EGZ_CHECK_ARG(aligned_to(fused, 16) && aligned_to(gt, 16), "egz_late_gather: the fp32 outputs must be 16-byte aligned");
    const LgOut o{fused, gt, raw};
    hipLaunchKernelGGL(late_gather_kernel, dim3(egz_cdiv(HW, LG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx, HW, o,
                       status);
    EGZ_CHECK_LAUNCH("egz_late_gather");
    return 0;
}
