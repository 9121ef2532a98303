// The resident gathers: a batch built from a pool of decoded uint8 planes that stays in HBM.
//
// SP / AT sample layout (data/resident.py, `--gpu_resident`; DESIGN.md sections 20, 21 and 26).  One launch replaces, per batch,
// the file decode, the PCIe copy, three egz_u8_normalize launches, egz_nchw_to_nhwc_pad and egz_absmax: every gathered byte is
// read once and every output is written once as float4 per lane, contiguous across the wave.
//   pool   (P, H, W) uint8
//   table  (N, 22) int64 plane numbers per sample: column 0 the first of 3 consecutive BGR planes, 1 .. 20 the flow planes in
//          STdatas order (x_t, y_t, x_{t-1}, y_{t-1}, ...), 21 the ground truth
//   idx    (B,) int64 sample numbers
// Three kernels share one design and differ in where a lane's four bytes of a plane come from:
//   resident_gather_kernel         the four bytes at the lane's own pixels (one aligned dword; offsets are 64-bit, a pool may
//                                  exceed 4 GiB)
//   resident_gather_aug_kernel     the bytes a per-sample flip and integer translation put there, and a gain / bias on the colour
//                                  frame; the sample's parameters are drawn in the kernel or taken from an explicit row
//   resident_gather_affine_kernel  a bilinear mix of four neighbours under a per-sample magnification and rotation on top; a
//                                  sample whose matrices are the identity takes the aug kernel's path
// They are three kernels, not one with switches, because each costs what it does: a run without augmentation launches the first.
// What the second and the third share exists once, as the rg_* pieces below; the first, the hot path of every unaugmented run, is
// written out (see there).  A block owns 256 pixels of one sample:
//   rg_used, rg_row   which fields the launch reads, and the bounds of the sample's number and of its used table entries.
//                     Nothing is clamped: a sample that fails is skipped by its blocks (the decision is uniform per block) and a
//                     bit is raised in the status word (rg_raise).
//   rg_key .. rg_row5 the aug and affine kernels' parameters of a sample, drawn from a hash or read from a row and checked
//   rg_planes         wave w takes planes w, w + 4, ... of the 24 (the affine kernel's warped path pairs the flow planes instead)
//   rg_emit           one plane's four bytes to every output that wants them: the reference's three fp32 operations
//                     (bit-identical with u8_normalize_kernel), the NCHW stores straight from registers, and for the NHWC-32
//                     form of the flow stack a park in LDS ([channel][pixel], 16-byte groups XOR-swizzled by channel quad so
//                     that both the b128 writes and the transposed b32 reads are bank-conflict free)
//   rg_finish         the 20-plane transpose out of LDS -- whole 128-byte pixel rows, 8 lanes per pixel, channels 20 .. 31 as
//                     zeros: a wave store covers 1 KiB contiguous -- and the block's abs-max
//
// Late-fusion sample layout (data/late_resident.py, `--late_resident`): late_gather_kernel, three one-channel maps per sample (SP
// prediction, AT map, ground truth), every value u8 / 255.  It shares the load and convert helpers and the host checks.
#include "egz_common.h"

namespace {

constexpr int RG_TILE = 256;                  // pixels per block
constexpr int RG_COLS = 22, RG_PLANES = 24, RG_FLOW = 20;

__device__ __forceinline__ int rg_lds_index(int c, int p) { return c * RG_TILE + (p ^ (((c >> 2) & 7) << 2)); }

// The load and convert of all gathers: 4 consecutive bytes of pool plane `plane` at pixel p (64-bit offset; p % 4 == 0 and
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

// ----------------------------------------------------------------------------- fields and bounds
// fields this launch reads: bit 0 image, bit 1 flow, bit 2 ground truth
__device__ __forceinline__ int rg_raw_fields(const RgOut& o) { return o.raw ? o.raw_fields : 0; }
__device__ __forceinline__ int rg_used(const RgOut& o) {
    return (o.image ? 1 : 0) | ((o.flow || o.nhwc) ? 2 : 0) | (o.gt ? 4 : 0) | rg_raw_fields(o);
}

// Bounds (block-uniform) of sample b -> 0 with its number s and its table row, or the status bit of what failed: bit 0, idx[b]
// outside the table; bit 1, a used entry outside the pool (the image needs three planes from row[0] on).  On a bit the caller
// raises it (rg_raise) and returns: nothing dereferences an index that failed.  The two are apart so that `row` is not merged
// behind rg_raise's one-thread branch: the compiler then keeps the row's address and the plane numbers read from it in scalar
// registers.
__device__ __forceinline__ int rg_row(const long* __restrict__ table, long N, const long* __restrict__ idx, long P, int b,
                                      int used, long& s, const long*& row) {
    s = idx[b];
    if (s < 0 || s >= N) return 1;
    row = table + s * RG_COLS;
    bool ok = true;
    if (used & 1) ok = ok && row[0] >= 0 && row[0] <= P - 3;
    if (used & 2)
        for (int j = 1; j <= RG_FLOW; ++j) ok = ok && row[j] >= 0 && row[j] < P;
    if (used & 4) ok = ok && row[21] >= 0 && row[21] < P;
    return ok ? 0 : 2;
}
// The sample is skipped: one thread of its blocks says why in the status word.
__device__ __forceinline__ void rg_raise(int* __restrict__ status, int bits) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, bits);
}

// ----------------------------------------------------------------------------- a sample's parameters
// flip, dy, dx, gain and bias of a sample are drawn from a counter-based hash of (seed, epoch, sample number) -- nothing depends
// on the batch position, the batch size or the rank -- or taken from an explicit row.  Block-uniform: every block of the sample
// repeats the few dozen 64-bit multiplies of the draw.
struct RgAug {
    unsigned long long seed, epoch, flip_thr;
    int max_shift;
    float contrast, brightness;
    const int* params_in;                     // (B, 5) flip, dy, dx, bits(gain), bits(bias): replaces the draw when non-null
    int* params_out;                          // (B, 5) the parameters used, same layout ((B, 7) in the affine gather)
};
constexpr unsigned long long RG_GOLD = 0x9E3779B97F4A7C15ull;

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

// The hash key of sample s; word k of its draw is rg_mix(key + k * RG_GOLD), k = 1 .. 5 here and 6, 7 in the affine kernel.
__device__ __forceinline__ unsigned long long rg_key(const RgAug& g, long s) {
    return rg_mix(rg_mix(rg_mix(g.seed + RG_GOLD) ^ g.epoch) ^ (unsigned long long)s);
}
__device__ __forceinline__ void rg_draw5(const RgAug& g, unsigned long long key, int& flip, int& dy, int& dx, float& gain,
                                         float& bias) {
    const unsigned int span = 2u * (unsigned int)g.max_shift + 1u;
    flip = (rg_mix(key + RG_GOLD) >> 32) < g.flip_thr ? 1 : 0;
    dy = (int)((unsigned int)(rg_mix(key + 2 * RG_GOLD) >> 32) % span) - g.max_shift;
    dx = (int)((unsigned int)(rg_mix(key + 3 * RG_GOLD) >> 32) % span) - g.max_shift;
    // one fp32 rounding per operation
    gain = rg_mul_add(g.contrast, rg_sym(rg_mix(key + 4 * RG_GOLD)), 1.f);
    bias = g.brightness * rg_sym(rg_mix(key + 5 * RG_GOLD));
}
// The first five words of an explicit row; false (status bit 2) for a flip outside {0, 1}, |dy| or |dx| above 32767 or a
// non-finite gain / bias.
__device__ __forceinline__ bool rg_row5(const int* q, int& flip, int& dy, int& dx, float& gain, float& bias) {
    flip = q[0], dy = q[1], dx = q[2];
    const unsigned int ua = (unsigned int)q[3], ub = (unsigned int)q[4];
    gain = __uint_as_float(ua), bias = __uint_as_float(ub);
    return !((flip & ~1) || dy < -32767 || dy > 32767 || dx < -32767 || dx > 32767 || rg_nonfinite(ua) || rg_nonfinite(ub));
}
__device__ __forceinline__ void rg_put5(int* q, int flip, int dy, int dx, float gain, float bias) {
    q[0] = flip, q[1] = dy, q[2] = dx, q[3] = (int)__float_as_uint(gain), q[4] = (int)__float_as_uint(bias);
}

// ----------------------------------------------------------------------------- the integer-offset fetch
// A lane's 4 output pixels: W % 4 == 0 puts them in one row, at columns x .. x + 3 with x % 4 == 0.  They show the flipped
// frame F at row y - dy, columns fx .. fx + 3.  A lane is INTERIOR when those four columns are in the frame: its source bytes
// are then the four consecutive columns c0 .. c0 + 3 of one source row (c0 = fx, or W - 4 - fx in reverse order under a
// flip), 0 <= c0 <= W - 4.  They lie in the aligned dword at a0 = c0 & ~3 and, when c0 % 4 != 0, the next one: then
// c0 <= W - 5, so a0 <= W - 8 and a0 + 7 <= W - 1 -- both dwords are inside the source row (W % 4 == 0), which is inside a
// plane whose number passed rg_row, so no access leaves the row, let alone the pool.  c0 % 4 depends on dx and the flip alone:
// the second load is a block-uniform decision.  BORDER lanes fetch byte by byte at clamped coordinates, and the source row is
// clamped to the frame: the colour frame and the flow replicate the edge, the ground truth is 0 outside.
struct RgShift {
    long rowoff;
    int fx, c0, W;
    unsigned int rot;
    bool row_in, interior, flip;
};
__device__ __forceinline__ RgShift rg_shift(int x, int y, int dx, int dy, int flip, int H, int W) {
    RgShift t;
    const int yy = y - dy;
    t.fx = x - dx, t.W = W, t.flip = flip != 0;
    t.row_in = yy >= 0 && yy < H;
    t.rowoff = (long)min(max(yy, 0), H - 1) * W;
    t.interior = t.fx >= 0 && t.fx <= W - 4;
    t.c0 = flip ? W - 4 - t.fx : t.fx;
    t.rot = (unsigned int)t.c0 & 3u;
    return t;
}
// The bytes of the plane that starts at plane0 for the lane's 4 pixels; an x-flow plane is negated under a flip (255 - byte).
__device__ __forceinline__ unsigned int rg_fetch_shift(const unsigned char* __restrict__ plane0, const RgShift& t, bool is_gt,
                                                       bool is_xflow) {
    const unsigned char* src = plane0 + t.rowoff;
    unsigned int u = 0u;
    if (is_gt && !t.row_in) {
        // a gaze map has no mass outside the picture
    } else if (t.interior) {
        const unsigned int* q = reinterpret_cast<const unsigned int*>(src + (t.c0 & ~3));
        u = q[0];
        if (t.rot) u = __builtin_amdgcn_alignbyte(q[1], u, t.rot);     // bytes rot .. rot + 3 of the pair
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

// ----------------------------------------------------------------------------- stores, plane loop, tail
// Plane c's 4 bytes of a lane, at pixels p .. p + 3 of sample b, to every output that wants them.  The colour frame takes the
// gain and the bias first, clamped to [0, 1] (gain 1, bias 0: t itself).  raw_fields (rg_raw_fields) and the lane number come
// from the kernel, which has them once: recomputed here for every plane they cost the affine kernel the registers that keep it
// at 7 waves per SIMD without scratch.
__device__ __forceinline__ void rg_emit(const RgOut& o, int raw_fields, int lane, int b, int c, unsigned int u, long HW, long p,
                                        float gain, float bias, const float* __restrict__ mean,
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

// The planes of a wave on the integer path, c = wave, wave + 4, ...: 0 .. 2 image, 3 .. 22 flow, 23 ground truth (wave-uniform).
// p % 4 == 0 and HW % 4 == 0: a lane's group is inside the plane (live) or outside.
__device__ __forceinline__ void rg_planes(const unsigned char* __restrict__ pool, const long* row, const RgOut& o, int used,
                                          int raw_fields, int lane, int b, long HW, long p, const RgShift& t, float gain,
                                          float bias, const float* __restrict__ mean, const float* __restrict__ stdv,
                                          float* tile, float& am) {
    const int wave = threadIdx.x >> 6;
    const bool live = p < HW;
#pragma unroll
    for (int i = 0; i < RG_PLANES / 4; ++i) {
        const int c = wave + 4 * i;
        const int field = c < 3 ? 1 : (c < 23 ? 2 : 4);
        if (!(used & field) || !live) continue;
        const long plane = c < 3 ? row[0] + c : row[c - 2];
        const unsigned int u = rg_fetch_shift(pool + plane * HW, t, field == 4, field == 2 && !((c - 3) & 1));
        rg_emit(o, raw_fields, lane, b, c, u, HW, p, gain, bias, mean, stdv, tile, am);
    }
}

// The tail of a block that makes the NHWC-32 form (o.nhwc, uniform): the block's abs-max, then the transpose of the 20 planes
// parked in `tile`, 8 lanes per pixel, a float4 of channels 4 q .. 4 q + 3 each: pixel rows of 128 bytes, contiguous from lane
// to lane.
__device__ __forceinline__ void rg_finish(const RgOut& o, const float* tile, float* s_am, float am, int b, long HW, long p0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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

// ----------------------------------------------------------------------------- the plain gather
// This kernel keeps a body of its own, the statements the pieces above were taken from: it is what a run without augmentation
// launches for every batch, and written through the shared pieces it came out 0.5 .. 0.7 % slower (profiles/gather_refactor.txt).
// No single piece could be held responsible -- rg_used, rg_row / rg_raise and rg_finish each change its instructions when put in
// alone -- so none is used here, and its code object is the one it had before the other two kernels were folded together.  What
// it has in common with them (the field mask, the bounds, the stores, the tail) must be changed in both places.
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

// ----------------------------------------------------------------------------- the augmented gather
// A per-sample horizontal flip and integer translation applied consistently to the colour frame, the 20 flow planes and the
// ground truth, the x-flow negated under a flip, and a gain / bias on the colour frame.  H * W < 2^31 (the entry point sees to
// it): pixel numbers fit 32 bits, which the division into row and column wants.
__global__ __launch_bounds__(256) void resident_gather_aug_kernel(const unsigned char* __restrict__ pool, long P,
                                                                  const long* __restrict__ table, long N,
                                                                  const long* __restrict__ idx, int H, int W,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, RgOut o, RgAug g,
                                                                  int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float tile[RG_FLOW * RG_TILE];
    __shared__ float s_am[4];
    const int b = blockIdx.y;
    const unsigned int HW = (unsigned int)H * (unsigned int)W;
    const unsigned int p0 = blockIdx.x * (unsigned int)RG_TILE;
    const int used = rg_used(o);
    long s;
    const long* row;
    if (const int bad = rg_row(table, N, idx, P, b, used, s, row)) {
        rg_raise(status, bad);
        return;
    }

    int flip, dy, dx;
    float gain, bias;
    if (g.params_in) {
        if (!rg_row5(g.params_in + 5 * b, flip, dy, dx, gain, bias)) {
            rg_raise(status, 4);
            return;
        }
    } else {
        rg_draw5(g, rg_key(g, s), flip, dy, dx, gain, bias);
    }
    if (g.params_out && threadIdx.x == 0 && blockIdx.x == 0) rg_put5(g.params_out + 5 * b, flip, dy, dx, gain, bias);

    const int lane = threadIdx.x & 63;
    const unsigned int p = p0 + 4u * lane;
    const int y = (int)(p / (unsigned int)W), x = (int)(p - (unsigned int)y * (unsigned int)W);
    float am = 0.f;
    rg_planes(pool, row, o, used, rg_raw_fields(o), lane, b, HW, p, rg_shift(x, y, dx, dy, flip, H, W), gain, bias, mean, stdv,
              tile, am);
    if (o.nhwc) rg_finish(o, tile, s_am, am, b, HW, p0);
}

// ----------------------------------------------------------------------------- the affine gather
// The augmented gather with a per-sample magnification g and rotation theta about the frame's centre,
// p_out = c + d + g R(theta) (F(p_src) - c).  Every output pixel has a source coordinate in 1/256 pixel, computed in integers
// from a Q16 inverse matrix, and takes the bilinear mix of its four neighbours in every plane; the two planes of a flow pair are
// mixed by the same lane and then turned and scaled by the Q16 forward matrix, since the vectors move with the picture.  On this
// warped path the planes go to the waves otherwise than in rg_planes -- wave 0 takes the colour frame, the ground truth and flow
// pair 0, waves 1 .. 3 three flow pairs each, six planes per wave -- so that a pair never straddles two waves.  A sample whose
// matrices are the identity (block-uniform) calls rg_planes as the aug kernel does, which the affine formulas reproduce bit for
// bit.  __launch_bounds__(256, 7) holds the kernel to the 72 VGPRs of 7 waves per SIMD, the aug kernel's occupancy: the identity
// path's time follows it (profiles/augment_affine.txt).
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
    const int raw_fields = rg_raw_fields(o);
    const int used = rg_used(o);
    long s;
    const long* row;
    if (const int bad = rg_row(table, N, idx, P, b, used, s, row)) {
        rg_raise(status, bad);
        return;
    }

    // the sample's parameters and matrices (block-uniform): the aug kernel's five, then the magnification and the angle as words
    // 5 and 6 of a (B, 7) row or of the draw
    int flip, dy, dx;
    float gain, bias, mag, theta;
    if (g.params_in) {
        const int* q = g.params_in + 7 * b;
        int bad = rg_row5(q, flip, dy, dx, gain, bias) ? 0 : 4;
        mag = __uint_as_float((unsigned int)q[5]), theta = __uint_as_float((unsigned int)q[6]);
        // written so that a NaN fails: g in [0.5, 1.5], |theta| <= float32(pi / 4)
        if (!(mag >= 0.5f && mag <= 1.5f) || !(fabsf(theta) <= 0x1.921fb6p-1f)) bad |= 8;
        if (bad) {
            rg_raise(status, bad);
            return;
        }
    } else {
        const unsigned long long key = rg_key(g, s);
        rg_draw5(g, key, flip, dy, dx, gain, bias);
        mag = rg_mul_add(a.scale, rg_sym(rg_mix(key + 6 * RG_GOLD)), 1.f);
        theta = a.rotate * rg_sym(rg_mix(key + 7 * RG_GOLD));
    }
    if (g.params_out && threadIdx.x == 0 && blockIdx.x == 0) {
        int* q = g.params_out + 7 * b;
        rg_put5(q, flip, dy, dx, gain, bias);
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
        rg_planes(pool, row, o, used, raw_fields, lane, b, HW, p, rg_shift(x, y, dx, dy, flip, H, W), gain, bias, mean, stdv,
                  tile, am);
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
                rg_emit(o, raw_fields, lane, b, ca, ua, HW, p, gain, bias, mean, stdv, tile, am);
                rg_emit(o, raw_fields, lane, b, cb, ub, HW, p, gain, bias, mean, stdv, tile, am);
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
                if (used & fa) rg_emit(o, raw_fields, lane, b, ca, ua, HW, p, gain, bias, mean, stdv, tile, am);
                if (used & fb) rg_emit(o, raw_fields, lane, b, cb, ub, HW, p, gain, bias, mean, stdv, tile, am);
            }
        }
    }
    if (o.nhwc) rg_finish(o, tile, s_am, am, b, HW, p0);
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

// ----------------------------------------------------------------------------- argument checks of the entry points
// EGZ_CHECK_ARG returns from the function it stands in: each check below returns the code, and an entry point passes a non-zero
// one on.  `fn` is the entry point's name, the prefix of every message.
inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// What every gather checks.  lane_in_row: the aug and affine entries, whose lanes want their four pixels in one row (W % 4 == 0)
// and pixel numbers of 32 bits; the plain and late entries want H * W % 4 == 0 alone.
int check_gather(const char* fn, const void* pool, long P, const void* table, long N, const void* idx, int B, int H, int W,
                 const void* raw, const void* status, bool lane_in_row) {
    EGZ_CHECK_ARG(pool, "%s: pool is null", fn);
    EGZ_CHECK_ARG(table, "%s: table is null", fn);
    EGZ_CHECK_ARG(idx, "%s: idx is null", fn);
    EGZ_CHECK_ARG(status, "%s: status is null", fn);
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "%s: B = %d outside 1 .. 65535", fn, B);
    EGZ_CHECK_ARG(H > 0 && W > 0, "%s: H x W = %d x %d must be positive", fn, H, W);
    const long HW = (long)H * W;
    if (lane_in_row) {
        EGZ_CHECK_ARG(W % 4 == 0, "%s: W = %d must be a multiple of 4 (a lane's four pixels share a row)", fn, W);
        EGZ_CHECK_ARG(HW < (1l << 31), "%s: H * W = %ld must be below 2^31", fn, HW);
    } else {
        EGZ_CHECK_ARG(HW % 4 == 0, "%s: H * W = %ld must be a multiple of 4", fn, HW);
    }
    EGZ_CHECK_ARG(P >= 1 && N >= 1, "%s: P = %ld planes, N = %ld samples: both must be positive", fn, P, N);
    EGZ_CHECK_ARG(aligned_to(pool, 4) && aligned_to(raw, 4), "%s: pool / raw must be 4-byte aligned", fn);
    return 0;
}

// What the three SP / AT entries check on top.
int check_resident(const char* fn, const float* mean, const float* stdv, const RgOut& o) {
    EGZ_CHECK_ARG(mean && stdv, "%s: mean / std is null", fn);
    EGZ_CHECK_ARG(!o.raw || (o.raw_fields & 7) != 0 && (o.raw_fields & ~7) == 0,
                  "%s: raw_fields = %d must name at least one of image (1), flow (2), gt (4)", fn, o.raw_fields);
    EGZ_CHECK_ARG(o.image || o.flow || o.gt || o.nhwc || o.raw, "%s: no output (every output pointer is null)", fn);
    EGZ_CHECK_ARG((o.nhwc != nullptr) == (o.absmax != nullptr),
                  "%s: flow_nhwc32 and absmax go together (one is null, the other is not)", fn);
    EGZ_CHECK_ARG(aligned_to(o.image, 16) && aligned_to(o.flow, 16) && aligned_to(o.gt, 16) && aligned_to(o.nhwc, 16),
                  "%s: the fp32 outputs must be 16-byte aligned", fn);
    return 0;
}

// The draw's spec of the aug and affine entries.
int check_draw(const char* fn, const RgAug& g) {
    EGZ_CHECK_ARG(g.flip_thr <= (1ull << 32), "%s: flip_thr = %llu outside 0 .. 2^32", fn, g.flip_thr);
    EGZ_CHECK_ARG(g.max_shift >= 0 && g.max_shift <= 32767, "%s: max_shift = %d outside 0 .. 32767", fn, g.max_shift);
    EGZ_CHECK_ARG(g.contrast >= 0.f && g.contrast < 1.f, "%s: contrast = %g outside [0, 1)", fn, (double)g.contrast);
    EGZ_CHECK_ARG(g.brightness >= 0.f && g.brightness < 1.f, "%s: brightness = %g outside [0, 1)", fn, (double)g.brightness);
    EGZ_CHECK_ARG(aligned_to(g.params_in, 4) && aligned_to(g.params_out, 4), "%s: params_in / params_out must be 4-byte aligned",
                  fn);
    return 0;
}

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
    const char* fn = "egz_resident_gather";
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    if (int rc = check_gather(fn, pool, P, table, N, idx, B, H, W, raw, status, false)) return rc;
    if (int rc = check_resident(fn, mean, stdv, o)) return rc;
    const long HW = (long)H * W;
    hipLaunchKernelGGL(resident_gather_kernel, dim3(egz_cdiv(HW, RG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx, HW,
                       mean, stdv, o, status);
    EGZ_CHECK_LAUNCH(fn);
    return 0;
}

// table (N, 3) int64: the plane numbers of the SP prediction, the AT map and the ground truth of a sample.  fused (B,2,H,W) fp32
// (channel 0 the AT map, channel 1 the SP prediction), gt (B,1,H,W) fp32 and raw (B,3,H,W) uint8 (table order) are optional
// (null: not produced, nothing written).  status: as above; bit 1 looks at the columns of the outputs asked for.
EGZ_API int egz_late_gather(const unsigned char* pool, long P, const long* table, long N, const long* idx, int B, int H, int W,
                            float* fused, float* gt, unsigned char* raw, int* status, hipStream_t st) {
    const char* fn = "egz_late_gather";
    if (int rc = check_gather(fn, pool, P, table, N, idx, B, H, W, raw, status, false)) return rc;
    EGZ_CHECK_ARG(fused || gt || raw, "%s: no output (every output pointer is null)", fn);
    EGZ_CHECK_ARG(aligned_to(fused, 16) && aligned_to(gt, 16), "%s: the fp32 outputs must be 16-byte aligned", fn);
    const long HW = (long)H * W;
    const LgOut o{fused, gt, raw};
    hipLaunchKernelGGL(late_gather_kernel, dim3(egz_cdiv(HW, LG_TILE), B), dim3(256), 0, st, pool, P, table, N, idx, HW, o,
                       status);
    EGZ_CHECK_LAUNCH(fn);
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
    const char* fn = "egz_resident_gather_aug";
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    const RgAug g{seed, epoch, flip_thr, max_shift, contrast, brightness, params_in, params_out};
    if (int rc = check_gather(fn, pool, P, table, N, idx, B, H, W, raw, status, true)) return rc;
    if (int rc = check_resident(fn, mean, stdv, o)) return rc;
    if (int rc = check_draw(fn, g)) return rc;
    hipLaunchKernelGGL(resident_gather_aug_kernel, dim3(egz_cdiv((long)H * W, RG_TILE), B), dim3(256), 0, st, pool, P, table, N,
                       idx, H, W, mean, stdv, o, g, status);
    EGZ_CHECK_LAUNCH(fn);
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
    const char* fn = "egz_resident_gather_affine";
    const RgOut o{image, flow, gt, flow_nhwc32, absmax, raw, raw_fields};
    const RgAug g{seed, epoch, flip_thr, max_shift, contrast, brightness, params_in, params_out};
    const RgAffine a{scale, rotate_rad};
    if (int rc = check_gather(fn, pool, P, table, N, idx, B, H, W, raw, status, true)) return rc;
    if (int rc = check_resident(fn, mean, stdv, o)) return rc;
    if (int rc = check_draw(fn, g)) return rc;
    EGZ_CHECK_ARG(scale >= 0.f && scale <= 0.5f, "%s: scale = %g outside [0, 0.5]", fn, (double)scale);
    EGZ_CHECK_ARG(rotate_rad >= 0.f && rotate_rad <= 0x1.921fb6p-1f, "%s: rotate_rad = %g outside [0, pi / 4]", fn,
                  (double)rotate_rad);
    hipLaunchKernelGGL(resident_gather_affine_kernel, dim3(egz_cdiv((long)H * W, RG_TILE), B), dim3(256), 0, st, pool, P, table,
                       N, idx, H, W, mean, stdv, o, g, a, status);
    EGZ_CHECK_LAUNCH(fn);
    return 0;
}
