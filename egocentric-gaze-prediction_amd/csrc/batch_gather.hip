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

// ----------------------------------------------------------------------------- affine gather
// egz_resident_gather_affine: the augmented gather above with a per-sample magnification g and rotation theta about the frame's
// centre, p_out = c + d + g R(theta) (F(p_src) - c).  Every output pixel has a source coordinate in 1/256 pixel, computed in
// integers from a Q16 inverse matrix, and takes the bilinear mix of its four neighbours in every plane; the two planes of a flow
// pair are mixed by the same lane and then turned and scaled by the Q16 forward matrix, since the vectors move with the picture.
// Block shape, stores, LDS transpose and abs-max are those of the kernels above; what differs on the warped path is the
// assignment of planes to waves -- wave 0 takes the colour frame, the ground truth and flow pair 0, waves 1 .. 3 three flow pairs
// each, six planes per wave -- so that a pair never straddles two waves.  A sample whose matrices are the identity
// (block-uniform) runs resident_gather_aug_kernel's statements instead, planes per wave included, which the affine formulas
// reproduce bit for bit.  __launch_bounds__(256, 7) holds the kernel to the 72 VGPRs of 7 waves per SIMD, that kernel's occupancy:
// the identity path's time follows it (profiles/augment_affine.txt).
struct RgAffine {
    float scale, rotate;                      // amplitudes of the draw: g in 1 +- scale, theta in +- rotate (radians)
};

// (S, C, 1 / g) -> the four Q16 matrix entries.  The polynomial is the definition: every operation is rounded on its own.
__device__ __forceinline__ void rg_affine_matrices(float g, float theta, int& M00, int& M01, int& A00, int& A10) {
#pragma clang fp contract(off)
    const float s1 = -0x1.555546p-3f, s2 = 0x1.11073cp-7f, s3 = -0x1.9943f2p-13f;
    const float c1 = 0x1.55554ap-5f, c2 = -0x1.6c0c34p-10f, c3 = 0x1.99eb9cp-16f;
    const float z = theta * theta;
    float ps = s3 * z;
    ps = ps + s2;
    ps = ps * z;
    ps = ps + s1;
    float tz = theta * z;
    tz = tz * ps;
    const float S = theta + tz;
    float pc = c3 * z;
    pc = pc + c2;
    pc = pc * z;
    pc = pc + c1;
    float zz = z * z;
    zz = zz * pc;
    float hz = 0.5f * z;
    hz = 1.f - hz;
    const float C = hz + zz;
    const float q = __fdiv_rn(1.f, g);
    const float qc = q * C, qs = q * S, gc = g * C, gs = g * S;
    M00 = (int)rintf(qc * 65536.f), M01 = (int)rintf(qs * 65536.f);
    A00 = (int)rintf(gc * 65536.f), A10 = (int)rintf(gs * 65536.f);
}

// The bytes of one plane for a lane's 4 pixels on the integer-offset path: resident_gather_aug_kernel's fetch.
struct RgShift {
    long rowoff;
    int fx, c0, W;
    unsigned int rot;
    bool row_in, interior, flip;
};
__device__ __forceinline__ unsigned int rg_fetch_shift(const unsigned char* __restrict__ plane0, const RgShift& t, bool is_gt,
                                                       bool is_xflow) {
    const unsigned char* src = plane0 + t.rowoff;
    unsigned int u = 0u;
    if (is_gt && !t.row_in) {
        // a gaze map has no mass outside the picture
    } else if (t.interior) {
        const unsigned int* q = reinterpret_cast<const unsigned int*>(src + (t.c0 & ~3));
        u = q[0];
        if (t.rot) u = __builtin_amdgcn_alignbyte(q[1], u, t.rot);
        if (t.flip) u = __builtin_bswap32(u);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = t.fx + e;
            if (is_gt && (col < 0 || col >= t.W)) continue;
            const int cc = min(max(col, 0), t.W - 1);
            u |= (unsigned int)src[t.flip ? t.W - 1 - cc : cc] << (8 * e);
        }
    }
    if (t.flip && is_xflow) u = ~u;
    return u;
}

// The four taps of one output pixel, kept packed -- the offset of tap (y0, x0) in a plane (clamped to the frame, the flip
// applied) and a word of fx, fy, the steps to the next column (-1, 0, 1) and row (0, 1) and the mask of taps inside the frame --
// and unpacked where a plane pair is mixed: offsets, and Q16 weights that sum to 65536.  Computed once per pixel, used by every
// plane of the wave.
struct RgTap {
    int off;
    unsigned int bits;                        // fx 0..7, fy 8..15, inside 16..19, row step 20, column step + 1 in 21..22
};
struct RgTap4 {
    int off[4];
    unsigned int wgt[4], inside;
};
__device__ __forceinline__ RgTap4 rg_unpack(const RgTap& t, int W) {
    const unsigned int fx = t.bits & 255u, fy = (t.bits >> 8) & 255u;
    const int sx = (int)((t.bits >> 21) & 3u) - 1, sy = (t.bits >> 20) & 1u ? W : 0;
    RgTap4 r;
    r.off[0] = t.off, r.off[1] = t.off + sx, r.off[2] = t.off + sy, r.off[3] = t.off + sy + sx;
    r.wgt[0] = (256u - fx) * (256u - fy), r.wgt[1] = fx * (256u - fy), r.wgt[2] = (256u - fx) * fy, r.wgt[3] = fx * fy;
    r.inside = (t.bits >> 16) & 15u;
    return r;
}
__device__ __forceinline__ unsigned int rg_mix4(const unsigned char* __restrict__ src, const RgTap4& t, bool is_gt,
                                                unsigned int flipmask) {
    unsigned int acc = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int v = (unsigned int)src[t.off[k]] ^ flipmask;
        if (is_gt && !((t.inside >> k) & 1u)) v = 0u;
        acc += t.wgt[k] * v;
    }
    return acc;
}

// One plane's 4 bytes of a lane to every output that wants them: resident_gather_aug_kernel's stores.
__device__ __forceinline__ void rg_emit(const RgOut& o, int raw_fields, int b, int c, unsigned int u, unsigned int HW,
                                        unsigned int p, int lane, float gain, float bias, const float* __restrict__ mean,
                                        const float* __restrict__ stdv, float* tile, float& am) {
    const int field = c < 3 ? 1 : (c < 23 ? 2 : 4);
    if (raw_fields & field) *reinterpret_cast<unsigned int*>(o.raw + ((long)b * RG_PLANES + c) * HW + p) = u;
    float* dst = c < 3 ? (o.image ? o.image + ((long)b * 3 + c) * HW : nullptr)
               : c < 23 ? (o.flow ? o.flow + ((long)b * RG_FLOW + (c - 3)) * HW : nullptr)
                        : (o.gt ? o.gt + (long)b * HW : nullptr);
    const bool to_lds = field == 2 && o.nhwc;
    if (!dst && !to_lds) return;
    const float m = mean[c], sd = stdv[c];
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = rg_unit(u, e);
        if (field == 1) t = fminf(fmaxf(rg_mul_add(gain, t, bias), 0.f), 1.f);
        v[e] = (t - m) / sd;
    }
    if (dst) *reinterpret_cast<f32x4*>(dst + p) = v;
    if (to_lds) {
        *reinterpret_cast<f32x4*>(&tile[rg_lds_index(c - 3, 4 * lane)]) = v;
        am = fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
}

__global__ __launch_bounds__(256, 7) void resident_gather_affine_kernel(const unsigned char* __restrict__ pool, long P,
                                                                     const long* __restrict__ table, long N,
                                                                     const long* __restrict__ idx, int H, int W,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv, RgOut o, RgAug g,
                                                                     RgAffine a, int* __restrict__ status) {
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

    // the sample's parameters and matrices (block-uniform)
    int flip, dy, dx;
    float gain, bias, mag, theta;
    if (g.params_in) {
        const int* q = g.params_in + 7 * b;
        flip = q[0], dy = q[1], dx = q[2];
        const unsigned int ua = (unsigned int)q[3], ub = (unsigned int)q[4], ug = (unsigned int)q[5], ut = (unsigned int)q[6];
        gain = __uint_as_float(ua), bias = __uint_as_float(ub), mag = __uint_as_float(ug), theta = __uint_as_float(ut);
        int bad = 0;
        if ((flip & ~1) || dy < -32767 || dy > 32767 || dx < -32767 || dx > 32767 || rg_nonfinite(ua) || rg_nonfinite(ub))
            bad |= 4;
        // written so that a NaN fails: g in [0.5, 1.5], |theta| <= float32(pi / 4)
        if (!(mag >= 0.5f && mag <= 1.5f) || !(fabsf(theta) <= 0x1.921fb6p-1f)) bad |= 8;
        if (bad) {
            if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, bad);
            return;
        }
    } else {
        constexpr unsigned long long GOLD = 0x9E3779B97F4A7C15ull;
        const unsigned long long key = rg_mix(rg_mix(rg_mix(g.seed + GOLD) ^ g.epoch) ^ (unsigned long long)s);
        const unsigned int span = 2u * (unsigned int)g.max_shift + 1u;
        flip = (rg_mix(key + GOLD) >> 32) < g.flip_thr ? 1 : 0;
        dy = (int)((unsigned int)(rg_mix(key + 2 * GOLD) >> 32) % span) - g.max_shift;
        dx = (int)((unsigned int)(rg_mix(key + 3 * GOLD) >> 32) % span) - g.max_shift;
        gain = rg_mul_add(g.contrast, rg_sym(rg_mix(key + 4 * GOLD)), 1.f);
        bias = g.brightness * rg_sym(rg_mix(key + 5 * GOLD));
        mag = rg_mul_add(a.scale, rg_sym(rg_mix(key + 6 * GOLD)), 1.f);
        theta = a.rotate * rg_sym(rg_mix(key + 7 * GOLD));
    }
    if (g.params_out && threadIdx.x == 0 && blockIdx.x == 0) {
        int* q = g.params_out + 7 * b;
        q[0] = flip, q[1] = dy, q[2] = dx, q[3] = (int)__float_as_uint(gain), q[4] = (int)__float_as_uint(bias);
        q[5] = (int)__float_as_uint(mag), q[6] = (int)__float_as_uint(theta);
    }
    // g = 1 and theta = +-0 give the identity matrices by the definition: such a sample skips the polynomial and the division
    int M00 = 65536, M01 = 0, A00 = 65536, A10 = 0;
    if (!(mag == 1.f && theta == 0.f)) rg_affine_matrices(mag, theta, M00, M01, A00, A10);
    const bool identity = M00 == 65536 && M01 == 0 && A00 == 65536 && A10 == 0;

    // This lane's 4 output pixels share a row (W % 4 == 0).
    const unsigned int p = p0 + 4u * lane;
    const bool live = p < HW;
    const int y = (int)(p / (unsigned int)W), x = (int)(p - (unsigned int)y * (unsigned int)W);
    float am = 0.f;
    if (identity) {
        // resident_gather_aug_kernel's path: its planes per wave (w, w + 4, ...) and its interior / border split; see there for
        // why no access leaves the source row
        RgShift t;
        const int yy = y - dy;
        t.fx = x - dx, t.W = W, t.flip = flip != 0;
        t.row_in = yy >= 0 && yy < H;
        t.rowoff = (long)min(max(yy, 0), H - 1) * W;
        t.interior = t.fx >= 0 && t.fx <= W - 4;
        t.c0 = flip ? W - 4 - t.fx : t.fx;
        t.rot = (unsigned int)t.c0 & 3u;
#pragma unroll
        for (int i = 0; i < RG_PLANES / 4; ++i) {
            const int c = wave + 4 * i;
            const int field = c < 3 ? 1 : (c < 23 ? 2 : 4);
            if (!(used & field) || !live) continue;
            const long plane = c < 3 ? row[0] + c : row[c - 2];
            const unsigned int u = rg_fetch_shift(pool + plane * (long)HW, t, field == 4, field == 2 && !((c - 3) & 1));
            rg_emit(o, raw_fields, b, c, u, HW, p, lane, gain, bias, mean, stdv, tile, am);
        }
    } else {
        // Source coordinates (Q17, 64-bit) of the lane's first pixel; the next ones are 2 M00 and -2 M01 further.  A tap's
        // row and column are clamped to the frame before they become an offset, so every offset lies in 0 .. H W - 1 of a
        // plane whose number passed the bounds above; a pixel with all four taps inside needs no clamp.  Planes of the wave,
        // two at a time: wave 0 (0, 1), (2, 23), (3, 4); wave w > 0 the flow pairs 3 w - 2 .. 3 w, planes (3 + 2 k, 4 + 2 k).
        RgTap t[4];
        if (live) {
            const long X2 = 2l * ((long)x - dx) - (W - 1), Y2 = 2l * ((long)y - dy) - (H - 1);
            long XQ = (long)M00 * X2 + (long)M01 * Y2 + (long)(W - 1) * 65536;
            long YQ = -(long)M01 * X2 + (long)M00 * Y2 + (long)(H - 1) * 65536;
#pragma unroll
            for (int e = 0; e < 4; ++e, XQ += 2l * M00, YQ -= 2l * M01) {
                const long PX = (XQ + 256) >> 9, PY = (YQ + 256) >> 9;
                const unsigned int frac = ((unsigned int)PX & 255u) | (((unsigned int)PY & 255u) << 8);
                // clamping x0 to -2 .. W keeps both taps' clamped columns and their inside bits (W <= 2^31 - 4)
                const int x0 = (int)min(max(PX >> 8, -2l), (long)W), y0 = (int)min(max(PY >> 8, -2l), (long)H);
                if (x0 >= 0 && x0 <= W - 2 && y0 >= 0 && y0 <= H - 2) {
                    t[e].off = y0 * W + (flip ? W - 1 - x0 : x0);
                    t[e].bits = frac | (15u << 16) | (1u << 20) | ((flip ? 0u : 2u) << 21);
                } else {
                    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
                    const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
                    const int ca = flip ? W - 1 - xa : xa, cb = flip ? W - 1 - xb : xb;    // cb - ca in -1 .. 1, yb - ya in 0 .. 1
                    const unsigned int ix0 = x0 >= 0 && x0 < W, ix1 = x0 + 1 >= 0 && x0 + 1 < W;
                    const unsigned int iy0 = y0 >= 0 && y0 < H, iy1 = y0 + 1 >= 0 && y0 + 1 < H;
                    t[e].off = ya * W + ca;
                    t[e].bits = frac | (((ix0 & iy0) | ((ix1 & iy0) << 1) | ((ix0 & iy1) << 2) | ((ix1 & iy1) << 3)) << 16) |
                                ((unsigned int)(yb - ya) << 20) | ((unsigned int)(cb - ca + 1) << 21);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const bool pair = wave != 0 || i == 2;            // wave-uniform
            const int ca = wave == 0 ? (i == 0 ? 0 : i == 1 ? 2 : 3) : 6 * wave - 1 + 2 * i;
            const int cb = wave == 0 ? (i == 0 ? 1 : i == 1 ? 23 : 4) : ca + 1;
            if (!live) continue;
            if (pair) {
                if (!(used & 2)) continue;
                const unsigned char* sa = pool + row[ca - 2] * (long)HW;
                const unsigned char* sb = pool + row[cb - 2] * (long)HW;
                unsigned int ua = 0u, ub = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the x tap is 255 - byte under a flip; then the vector about 127.5 turns and scales with the picture
                    const RgTap4 t4 = rg_unpack(t[e], W);
                    const long cx = (long)rg_mix4(sa, t4, false, flip ? 255u : 0u) - 8355840l;
                    const long cy = (long)rg_mix4(sb, t4, false, 0u) - 8355840l;
                    const long ox = ((long)A00 * cx - (long)A10 * cy + 547608330240l + (1l << 31)) >> 32;
                    const long oy = ((long)A10 * cx + (long)A00 * cy + 547608330240l + (1l << 31)) >> 32;
                    ua |= (unsigned int)min(max(ox, 0l), 255l) << (8 * e);
                    ub |= (unsigned int)min(max(oy, 0l), 255l) << (8 * e);
                }
                rg_emit(o, raw_fields, b, ca, ua, HW, p, lane, gain, bias, mean, stdv, tile, am);
                rg_emit(o, raw_fields, b, cb, ub, HW, p, lane, gain, bias, mean, stdv, tile, am);
            } else {
                // two planes that do not couple: colour, or colour and ground truth
                const int fa = 1, fb = cb < 3 ? 1 : 4;
                const unsigned char* sa = pool + ((used & fa) ? row[0] + ca : 0) * (long)HW;
                const unsigned char* sb = pool + ((used & fb) ? (cb < 3 ? row[0] + cb : row[21]) : 0) * (long)HW;
                unsigned int ua = 0u, ub = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const RgTap4 t4 = rg_unpack(t[e], W);
                    if (used & fa) ua |= ((rg_mix4(sa, t4, false, 0u) + 32768u) >> 16) << (8 * e);
                    if (used & fb) ub |= ((rg_mix4(sb, t4, fb == 4, 0u) + 32768u) >> 16) << (8 * e);
                }
                if (used & fa) rg_emit(o, raw_fields, b, ca, ua, HW, p, lane, gain, bias, mean, stdv, tile, am);
                if (used & fb) rg_emit(o, raw_fields, b, cb, ub, HW, p, lane, gain, bias, mean, stdv, tile, am);
            }
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
        const int tt = it * 256 + threadIdx.x;
        const int q = tt & 7, px = tt >> 3;
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

// egz_resident_gather_aug with a magnification and a rotation about the frame's centre: the arguments
// above, then the two further amplitudes of the draw -- scale in [0, 0.5]: g in 1 +- scale; rotate_rad in [0, float32(pi / 4)]:
// theta in +- rotate_rad, positive turning the picture from +x towards +y (y down).  p_out = c + d + g R(theta) (F(p_src) - c);
// every plane is sampled bilinearly at a source coordinate in 1/256 pixel (colour and flow replicate the edge, the ground truth
// is 0 outside), and a flow pair's vector is turned and scaled with the picture.  params_in / params_out rows are (B, 7): flip,
// dy, dx, bits(gain), bits(bias), bits(g), bits(theta).  g = 1, theta = 0 reproduce egz_resident_gather_aug bit for bit.
// status: bits 0 .. 2 as above; bit 3 = an explicit row with g outside [0.5, 1.5], |theta| above float32(pi / 4) or either
// non-finite (the sample was skipped).
EGZ_API int egz_resident_gather_affine(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B,
                                       int H, int W, const float* mean, const float* stdv, float* image, float* flow, float* gt,
                                       float* flow_nhwc32, unsigned int* absmax, unsigned char* raw, int raw_fields,
                                       int* status, unsigned long long seed, unsigned long long epoch,
                                       unsigned long long flip_thr, int max_shift, float contrast, float brightness,
                                       const int* params_in, int* params_out, float scale, float rotate_rad, hipStream_t st) {
    EGZ_CHECK_ARG(pool, "egz_resident_gather_affine: pool is null");
    EGZ_CHECK_ARG(table, "egz_resident_gather_affine: table is null");
    EGZ_CHECK_ARG(idx, "egz_resident_gather_affine: idx is null");
    EGZ_CHECK_ARG(mean && stdv, "egz_resident_gather_affine: mean / std is null");
    EGZ_CHECK_ARG(status, "egz_resident_gather_affine: status is null");
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "egz_resident_gather_affine: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H > 0 && W > 0, "egz_resident_gather_affine: H x W = %d x %d must be positive", H, W);
    EGZ_CHECK_ARG(W % 4 == 0, "egz_resident_gather_affine: W = %d must be a multiple of 4 (a lane's four pixels share a row)", W);
    const long HW = (long)H * W;
    EGZ_CHECK_ARG(HW < (1l << 31), "egz_resident_gather_affine: H * W = %ld must be below 2^31", HW);
    EGZ_CHECK_ARG(P >= 1 && N >= 1, "egz_resident_gather_affine: P = %ld planes, N = %ld samples: both must be positive", P, N);
    EGZ_CHECK_ARG(!raw || (raw_fields & 7) != 0 && (raw_fields & ~7) == 0,
                  "egz_resident_gather_affine: raw_fields = %d must name at least one of image (1), flow (2), gt (4)",
                  raw_fields);
    EGZ_CHECK_ARG(image || flow || gt || flow_nhwc32 || raw,
                  "egz_resident_gather_affine: no output (every output pointer is null)");
    EGZ_CHECK_ARG((flow_nhwc32 != nullptr) == (absmax != nullptr),
                  "egz_resident_gather_affine: flow_nhwc32 and absmax go together (one is null, the other is not)");
    EGZ_CHECK_ARG(aligned_to(pool, 4) && aligned_to(raw, 4), "egz_resident_gather_affine: pool / raw must be 4-byte aligned");
    EGZ_CHECK_ARG(aligned_to(image, 16) && aligned_to(flow, 16) && aligned_to(gt, 16) && aligned_to(flow_nhwc32, 16),
                  "egz_resident_gather_affine: the fp32 outputs must be 16-byte aligned");
    EGZ_CHECK_ARG(flip_thr <= (1ull << 32), "egz_resident_gather_affine: flip_thr = %llu outside 0 .. 2^32", flip_thr);
    EGZ_CHECK_ARG(max_shift >= 0 && max_shift <= 32767, "egz_resident_gather_affine: max_shift = %d outside 0 .. 32767",
                  max_shift);
    EGZ_CHECK_ARG(contrast >= 0.f && contrast < 1.f, "egz_resident_gather_affine: contrast = %g outside [0, 1)",
                  (double)contrast);
    EGZ_CHECK_ARG(brightness >= 0.f && brightness < 1.f, "egz_resident_gather_affine: brightness = %g outside [0, 1)",
                  (double)brightness);
    EGZ_CHECK_ARG(scale >= 0.f && scale <= 0.5f, "egz_resident_gather_affine: scale = %g outside [0, 0.5]", (double)scale);
    EGZ_CHECK_ARG(rotate_rad >= 0.f && rotate_rad <= 0x1.921fb6p-1f,
                  "egz_resident_gather_affine: rotate_rad = %g outside [0, pi / 4]", (double)rotate_rad);
    EGZ_CHECK_ARG(aligned_to(params_in, 4) && aligned_to(params_out, 4),
                  "egz_resident_gather_affine: params_in / params_out must be 4-byte aligned");
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    const RgAug g{seed, epoch, flip_thr, max_shift, contrast, brightness, params_in, params_out};
    const RgAffine a{scale, rotate_rad};
    hipLaunchKernelGGL(resident_gather_affine_kernel, dim3(egz_cdiv(HW, RG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx,
                       H, W, mean, stdv, o, g, a, status);
    EGZ_CHECK_LAUNCH("egz_resident_gather_affine");
    return 0;
}
