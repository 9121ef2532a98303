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

// ----------------------------------------------------------------------------- augmented gather
// egz_resident_gather_aug: the gather above with a per-sample horizontal flip and integer translation applied consistently to the
// colour frame, the 20 flow planes and the ground truth, the x-flow negated under a flip (255 - byte), and a gain / bias on the
// colour frame.  The parameters of a sample are drawn here from a counter-based hash of (seed, epoch, sample number) -- nothing
// depends on the batch position, the batch size or the rank -- or taken from an explicit row.  resident_gather_kernel above is
// left as it is (a run without augmentation executes the code it always did); this kernel keeps its block shape, its stores and
// its LDS transpose and differs in where a lane's four bytes come from.
struct RgAug {
    unsigned long long seed, epoch, flip_thr;
    int max_shift;
    float contrast, brightness;
    const int* params_in;                     // (B, 5) flip, dy, dx, bits(gain), bits(bias): replaces the draw when non-null
    int* params_out;                          // (B, 5) the parameters used, same layout
};

__device__ __forceinline__ unsigned long long rg_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// fl(fl(a * x) + b): two fp32 roundings.  hipcc contracts a * x + b into one fma by default, and HIP's __fmul_rn / __fadd_rn
// are the plain operators, which it contracts just the same; the pragma takes the contraction off for this statement.
__device__ __forceinline__ float rg_mul_add(float a, float x, float b) {
#pragma clang fp contract(off)
    const float ax = a * x;
    return ax + b;
}
// 2 * (word >> 40) * 2^-24 - 1 in [-1, 1): 24 bits, every step exact in fp32 (fused or not)
__device__ __forceinline__ float rg_sym(unsigned long long word) {
    return rg_mul_add(2.f, (float)(unsigned int)(word >> 40) * 0x1p-24f, -1.f);
}
__device__ __forceinline__ bool rg_nonfinite(unsigned int bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(256) void resident_gather_aug_kernel(const unsigned char* __restrict__ pool, long P,
                                                                  const long* __restrict__ table, long N,
                                                                  const long* __restrict__ idx, int H, int W,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, RgOut o, RgAug g,
                                                                  int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float tile[RG_FLOW * RG_TILE];
    __shared__ float s_am[4];
    const int b = blockIdx.y;
    const unsigned int HW = (unsigned int)H * (unsigned int)W;        // the entry point keeps H * W below 2^31
    const unsigned int p0 = blockIdx.x * (unsigned int)RG_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int raw_fields = o.raw ? o.raw_fields : 0;
    const int used = (o.image ? 1 : 0) | ((o.flow || o.nhwc) ? 2 : 0) | (o.gt ? 4 : 0) | raw_fields;

    // bounds (block-uniform), as above: nothing below dereferences an index that failed
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

    // the sample's parameters (block-uniform; every block of the sample repeats the few dozen 64-bit multiplies of the draw)
    int flip, dy, dx;
    float gain, bias;
    if (g.params_in) {
        const int* q = g.params_in + 5 * b;
        flip = q[0], dy = q[1], dx = q[2];
        const unsigned int ua = (unsigned int)q[3], ub = (unsigned int)q[4];
        if ((flip & ~1) || dy < -32767 || dy > 32767 || dx < -32767 || dx > 32767 || rg_nonfinite(ua) || rg_nonfinite(ub)) {
            if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 4);
            return;
        }
        gain = __uint_as_float(ua), bias = __uint_as_float(ub);
    } else {
        constexpr unsigned long long GOLD = 0x9E3779B97F4A7C15ull;
        const unsigned long long key = rg_mix(rg_mix(rg_mix(g.seed + GOLD) ^ g.epoch) ^ (unsigned long long)s);
        const unsigned int span = 2u * (unsigned int)g.max_shift + 1u;
        flip = (rg_mix(key + GOLD) >> 32) < g.flip_thr ? 1 : 0;
        dy = (int)((unsigned int)(rg_mix(key + 2 * GOLD) >> 32) % span) - g.max_shift;
        dx = (int)((unsigned int)(rg_mix(key + 3 * GOLD) >> 32) % span) - g.max_shift;
        // one fp32 rounding per operation
        gain = rg_mul_add(g.contrast, rg_sym(rg_mix(key + 4 * GOLD)), 1.f);
        bias = g.brightness * rg_sym(rg_mix(key + 5 * GOLD));
    }
    if (g.params_out && threadIdx.x == 0 && blockIdx.x == 0) {
        int* q = g.params_out + 5 * b;
        q[0] = flip, q[1] = dy, q[2] = dx, q[3] = (int)__float_as_uint(gain), q[4] = (int)__float_as_uint(bias);
    }

    // This lane's 4 output pixels: W % 4 == 0 puts them in one row, at columns x .. x + 3 with x % 4 == 0.  They show the flipped
    // frame F at row y - dy, columns fx .. fx + 3.  A lane is INTERIOR when those four columns are in the frame: its source bytes
    // are then the four consecutive columns c0 .. c0 + 3 of one source row (c0 = fx, or W - 4 - fx in reverse order under a
    // flip), 0 <= c0 <= W - 4.  They lie in the aligned dword at a0 = c0 & ~3 and, when c0 % 4 != 0, the next one: then
    // c0 <= W - 5, so a0 <= W - 8 and a0 + 7 <= W - 1 -- both dwords are inside the source row (W % 4 == 0), which is inside a
    // plane whose number passed the bounds above, so no access leaves the row, let alone the pool.  c0 % 4 depends on dx and
    // the flip alone: the second load is a block-uniform decision.  BORDER lanes fetch byte by byte at clamped coordinates.
    const unsigned int p = p0 + 4u * lane;
    const bool live = p < HW;
    const int y = (int)(p / (unsigned int)W), x = (int)(p - (unsigned int)y * (unsigned int)W);
    const int yy = y - dy, fx = x - dx;
    const bool row_in = yy >= 0 && yy < H;
    const long rowoff = (long)min(max(yy, 0), H - 1) * W;
    const bool interior = fx >= 0 && fx <= W - 4;
    const int c0 = flip ? W - 4 - fx : fx;
    const unsigned int rot = (unsigned int)c0 & 3u;
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < RG_PLANES / 4; ++i) {
        const int c = wave + 4 * i;           // 0 .. 2 image, 3 .. 22 flow, 23 ground truth (wave-uniform)
        const int field = c < 3 ? 1 : (c < 23 ? 2 : 4);
        if (!(used & field) || !live) continue;
        const long plane = c < 3 ? row[0] + c : row[c - 2];
        const unsigned char* src = pool + plane * (long)HW + rowoff;
        unsigned int u = 0u;
        if (field == 4 && !row_in) {
            // a gaze map has no mass outside the picture
        } else if (interior) {
            const unsigned int* q = reinterpret_cast<const unsigned int*>(src + (c0 & ~3));
            u = q[0];
            if (rot) u = __builtin_amdgcn_alignbyte(q[1], u, rot);     // bytes rot .. rot + 3 of the pair
            if (flip) u = __builtin_bswap32(u);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = fx + e;
                if (field == 4 && (col < 0 || col >= W)) continue;
                const int cc = min(max(col, 0), W - 1);
                u |= (unsigned int)src[flip ? W - 1 - cc : cc] << (8 * e);
            }
        }
        if (flip && field == 2 && !((c - 3) & 1)) u = ~u;              // x-flow planes: 255 - byte
        if (raw_fields & field) *reinterpret_cast<unsigned int*>(o.raw + ((long)b * RG_PLANES + c) * HW + p) = u;
        float* dst = c < 3 ? (o.image ? o.image + ((long)b * 3 + c) * HW : nullptr)
                   : c < 23 ? (o.flow ? o.flow + ((long)b * RG_FLOW + (c - 3)) * HW : nullptr)
                            : (o.gt ? o.gt + (long)b * HW : nullptr);
        const bool to_lds = field == 2 && o.nhwc;
        if (!dst && !to_lds) continue;
        const float m = mean[c], sd = stdv[c];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = rg_unit(u, e);
            if (field == 1) t = fminf(fmaxf(rg_mul_add(gain, t, bias), 0.f), 1.f);   // gain 1, bias 0: t itself
            v[e] = (t - m) / sd;
        }
        if (dst) *reinterpret_cast<f32x4*>(dst + p) = v;
        if (to_lds) {
            *reinterpret_cast<f32x4*>(&tile[rg_lds_index(c - 3, 4 * lane)]) = v;
            am = fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
    }
    if (!o.nhwc) return;                      // uniform
    // the 20-plane transpose and the abs-max of resident_gather_kernel, on the augmented values
    for (int off = 32; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off));
    if (lane == 0) s_am[wave] = am;
    __syncthreads();
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

// egz_resident_gather with augmentation: the arguments above, then the draw's spec by value -- seed, epoch,
// flip_thr = floor(p * 2^32) in 0 .. 2^32, max_shift 0 .. 32767 pixels, contrast and brightness amplitudes in [0, 1) -- and two
// optional (B, 5) int32 tables on the device, rows of flip, dy, dx, bits(gain), bits(bias): params_in replaces the draw,
// params_out receives the parameters used (one write per sample that was not skipped).  W % 4 == 0 and H * W < 2^31.  status:
// bits 0 and 1 as above; bit 2 = an explicit row with flip outside {0, 1}, |dy| or |dx| above 32767 or a non-finite gain / bias
// (the sample was skipped).
EGZ_API int egz_resident_gather_aug(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H,
                                    int W, const float* mean, const float* stdv, float* image, float* flow, float* gt,
                                    float* flow_nhwc32, unsigned int* absmax, unsigned char* raw, int raw_fields, int* status,
                                    unsigned long long seed, unsigned long long epoch, unsigned long long flip_thr,
                                    int max_shift, float contrast, float brightness, const int* params_in, int* params_out,
                                    hipStream_t st) {
    EGZ_CHECK_ARG(pool, "egz_resident_gather_aug: pool is null");
    EGZ_CHECK_ARG(table, "egz_resident_gather_aug: table is null");
    EGZ_CHECK_ARG(idx, "egz_resident_gather_aug: idx is null");
    EGZ_CHECK_ARG(mean && stdv, "egz_resident_gather_aug: mean / std is null");
    EGZ_CHECK_ARG(status, "egz_resident_gather_aug: status is null");
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "egz_resident_gather_aug: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H > 0 && W > 0, "egz_resident_gather_aug: H x W = %d x %d must be positive", H, W);
    EGZ_CHECK_ARG(W % 4 == 0, "egz_resident_gather_aug: W = %d must be a multiple of 4 (a lane's four pixels share a row)", W);
    const long HW = (long)H * W;
    EGZ_CHECK_ARG(HW < (1l << 31), "egz_resident_gather_aug: H * W = %ld must be below 2^31", HW);
    EGZ_CHECK_ARG(P >= 1 && N >= 1, "egz_resident_gather_aug: P = %ld planes, N = %ld samples: both must be positive", P, N);
    EGZ_CHECK_ARG(!raw || (raw_fields & 7) != 0 && (raw_fields & ~7) == 0,
                  "egz_resident_gather_aug: raw_fields = %d must name at least one of image (1), flow (2), gt (4)", raw_fields);
    EGZ_CHECK_ARG(image || flow || gt || flow_nhwc32 || raw,
                  "egz_resident_gather_aug: no output (every output pointer is null)");
    EGZ_CHECK_ARG((flow_nhwc32 != nullptr) == (absmax != nullptr),
                  "egz_resident_gather_aug: flow_nhwc32 and absmax go together (one is null, the other is not)");
    EGZ_CHECK_ARG(aligned_to(pool, 4) && aligned_to(raw, 4), "egz_resident_gather_aug: pool / raw must be 4-byte aligned");
    EGZ_CHECK_ARG(aligned_to(image, 16) && aligned_to(flow, 16) && aligned_to(gt, 16) && aligned_to(flow_nhwc32, 16),
                  "egz_resident_gather_aug: the fp32 outputs must be 16-byte aligned");
    EGZ_CHECK_ARG(flip_thr <= (1ull << 32), "egz_resident_gather_aug: flip_thr = %llu outside 0 .. 2^32", flip_thr);
    EGZ_CHECK_ARG(max_shift >= 0 && max_shift <= 32767, "egz_resident_gather_aug: max_shift = %d outside 0 .. 32767", max_shift);
    EGZ_CHECK_ARG(contrast >= 0.f && contrast < 1.f, "egz_resident_gather_aug: contrast = %g outside [0, 1)", (double)contrast);
    EGZ_CHECK_ARG(brightness >= 0.f && brightness < 1.f, "egz_resident_gather_aug: brightness = %g outside [0, 1)",
                  (double)brightness);
    EGZ_CHECK_ARG(aligned_to(params_in, 4) && aligned_to(params_out, 4),
                  "egz_resident_gather_aug: params_in / params_out must be 4-byte aligned");
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    const RgAug g{seed, epoch, flip_thr, max_shift, contrast, brightness, params_in, params_out};
    hipLaunchKernelGGL(resident_gather_aug_kernel, dim3(egz_cdiv(HW, RG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx, H, W,
                       mean, stdv, o, g, status);
    EGZ_CHECK_LAUNCH("egz_resident_gather_aug");
    return 0;
}
