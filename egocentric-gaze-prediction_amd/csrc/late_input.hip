// The AT -> LF hand-over on the device, and the gaze marker of the overlays (predict.py).
//
// egz_late_input: what AT.extract_late writes and data/lateDataset reads back, without the files.  Per sample: the SP map
// (B, H, W) and the AT map (B, h, w) are quantised as the stages quantise them, q = trunc(fl32(255 x)) (== (255 * x).to(uint8)
// for x in [0, 1]); the AT plane is quantised at ITS resolution and then resized to H x W with OpenCV's 8-bit INTER_LINEAR
// arithmetic (linear_u8.h, egz_resize_linear_u8's); fused (B, 2, H, W) = (AT plane, SP plane) / 255 in late_fusion's channel
// order, every value (float)u8 / 255.f as egz_late_gather makes it; planes (B, 2, H, W) holds the two uint8 planes.  Either
// input may already be uint8.  Outside [0, 1] the quantisation is defined: NaN or x < 0 -> 0 and 255 x >= 256 -> 255, with
// bit 0 (NaN) or bit 1 (out of range) raised in the status word.  HBM-bound: one lane per 4 consecutive output pixels, 16-byte
// fp32 stores and 4-byte plane stores when H W is a multiple of 4 (else the same lanes go element by element); the h x w source of
// the resize is a few hundred bytes per sample and stays in cache.
//
// egz_late_store: the training pipeline's form of the same hand-over (AT.extract_late(into=...)): the two planes of a chunk,
// quantised and resized by the same code, go straight into the planes of a ResidentLateDataset pool that a (n, 3) table of
// destinations names, and the ground-truth plane of each sample is copied there from the resident ST pool.  No fp32 output.
//
// egz_draw_ring: pixel (y, x) of image m takes the colour iff r_in^2 <= (y - cy)^2 + (x - cx)^2 <= r_out^2, in 64-bit integers;
// a centre outside the image clips the ring.
#include "egz_common.h"
#include "linear_u8.h"

namespace {

constexpr int LI_NT = 256;
constexpr int LI_TILE = 4 * LI_NT;             // output pixels per block

// trunc(fl32(255 x)) with the out-of-domain cases defined; flags: bit 0 NaN, bit 1 out of range
__device__ __forceinline__ int li_quant(float x, int& flags) {
    if (x != x) { flags |= 1; return 0; }
    if (x < 0.f) { flags |= 2; return 0; }
    const float t = 255.f * x;
    if (t >= 256.f) { flags |= 2; return 255; }
    return (int)t;
}

// element i of a map that is fp32 or already uint8
template <bool U8> __device__ __forceinline__ int li_fetch(const void* __restrict__ base, long i, int& flags) {
    if constexpr (U8) return (int)static_cast<const unsigned char*>(base)[i];
    else return li_quant(static_cast<const float*>(base)[i], flags);
}

// 4 consecutive elements from i (a multiple of 4 when VEC: one 16-byte / 4-byte load)
template <bool U8, bool VEC> __device__ __forceinline__ void li_fetch4(const void* __restrict__ base, long i, int n, int* q,
                                                                     int& flags) {
    if constexpr (VEC) {
        if constexpr (U8) {
            const unsigned int u = *reinterpret_cast<const unsigned int*>(static_cast<const unsigned char*>(base) + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = (int)((u >> (8 * e)) & 255u);
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = li_quant(v[e], flags);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = e < n ? li_fetch<U8>(base, i + e, flags) : 0;
    }
}

struct LiTables {
    const int* xofs;
    const short* xalpha;
    const int* yofs;
    const short* yalpha;       // all null: the AT map already has H x W
};

// A resized fp32 map is judged where it is quantised, at its own resolution, once per sample (by the sample's first block): an
// output pixel reads only the source elements its coefficients reach.
__device__ __forceinline__ void li_judge(const void* __restrict__ at, long src, long hw, int& flags) {
    for (long i = threadIdx.x; i < hw; i += LI_NT) (void)li_fetch<false>(at, src + i, flags);
}

// output pixels p0 .. p0 + n - 1 (n <= 4; the rest 0) of the h x w plane at element ``src`` resized to H x W
template <bool AT_U8> __device__ __forceinline__ void li_resize4(const void* __restrict__ at, long src, long p0, int n, int W,
                                                                 int h, int w, const LiTables& t, int* qa) {
    int ignore = 0;                                 // (counted by li_judge)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        qa[e] = 0;
        if (e < n) {
            const long p = p0 + e;
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const int sx = t.xofs[x], a0 = t.xalpha[2 * x], a1 = t.xalpha[2 * x + 1];
            const int sy = t.yofs[y], b0 = t.yalpha[2 * y], b1 = t.yalpha[2 * y + 1];
            const int x1 = min(sx + 1, w - 1);
            const long r0 = src + (long)min(max(sy, 0), h - 1) * w, r1 = src + (long)min(max(sy + 1, 0), h - 1) * w;
            qa[e] = linear_mix(li_fetch<AT_U8>(at, r0 + sx, ignore), li_fetch<AT_U8>(at, r0 + x1, ignore),
                               li_fetch<AT_U8>(at, r1 + sx, ignore), li_fetch<AT_U8>(at, r1 + x1, ignore), a0, a1, b0,
                               b1) & 0xff;                           // uchar(...) as OpenCV stores it
        }
    }
}

__device__ __forceinline__ unsigned int li_pack4(const int* q) {
    return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
}

// n quantised pixels (4 when VEC: one 4-byte store) into a uint8 plane
template <bool VEC> __device__ __forceinline__ void li_put4(unsigned char* __restrict__ o, const int* q, int n) {
    if constexpr (VEC) {
        *reinterpret_cast<unsigned int*>(o) = li_pack4(q);
    } else {
        for (int e = 0; e < n; ++e) o[e] = (unsigned char)q[e];
    }
}

// grid (ceil(H W / LI_TILE), B)
template <bool SP_U8, bool AT_U8, bool VEC>
__global__ __launch_bounds__(LI_NT) void late_input_kernel(const void* __restrict__ sp, const void* __restrict__ at, int H, int W,
                                                           int h, int w, LiTables t, float* __restrict__ fused,
                                                           unsigned char* __restrict__ planes, int* __restrict__ status) {
    const int b = blockIdx.y;
    const long HW = (long)H * W, hw = (long)h * w;
    const bool resize = t.xofs != nullptr;
    int flags = 0;
    if (!AT_U8 && resize && blockIdx.x == 0) li_judge(at, b * hw, hw, flags);
    const long p0 = (long)blockIdx.x * LI_TILE + 4 * threadIdx.x;
    if (p0 < HW) {
        const int n = (int)min(4L, HW - p0);
        int qs[4], qa[4];
        li_fetch4<SP_U8, VEC>(sp, b * HW + p0, n, qs, flags);
        if (!resize) li_fetch4<AT_U8, VEC>(at, b * HW + p0, n, qa, flags);
        else li_resize4<AT_U8>(at, b * hw, p0, n, W, h, w, t, qa);
        float* f_at = fused + ((long)b * 2 + 0) * HW + p0;
        float* f_sp = fused + ((long)b * 2 + 1) * HW + p0;
        if constexpr (VEC) {
            f32x4 va, vs;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                va[e] = (float)qa[e] / 255.f;
                vs[e] = (float)qs[e] / 255.f;
            }
            *reinterpret_cast<f32x4*>(f_at) = va;
            *reinterpret_cast<f32x4*>(f_sp) = vs;
        } else {
            for (int e = 0; e < n; ++e) {
                f_at[e] = (float)qa[e] / 255.f;
                f_sp[e] = (float)qs[e] / 255.f;
            }
        }
        if (planes) {
            li_put4<VEC>(planes + ((long)b * 2 + 0) * HW + p0, qa, n);
            li_put4<VEC>(planes + ((long)b * 2 + 1) * HW + p0, qs, n);
        }
    }
    if (flags) atomicOr(status, flags);
}

// egz_late_store: the same two planes written where data/late_resident keeps them, and the ground-truth plane copied beside
// them.  grid (ceil(H W / LI_TILE), n).  Every block of a sample reads the sample's four plane numbers and judges them alike: a
// number outside its pool is never turned into an address, the sample writes nothing and bit 2 goes up (once, by the sample's
// first block).  A destination of -1 skips its plane: the map behind it is neither read nor judged.
template <bool SP_U8, bool AT_U8, bool VEC>
__global__ __launch_bounds__(LI_NT) void late_store_kernel(const void* __restrict__ sp, const void* __restrict__ at, int H, int W,
                                                           int h, int w, LiTables t, unsigned char* __restrict__ late_pool, long P,
                                                           const long* __restrict__ dst, const unsigned char* __restrict__ gt_pool,
                                                           long Q, const long* __restrict__ gt_src, int* __restrict__ status) {
    const int b = blockIdx.y;
    const long HW = (long)H * W, hw = (long)h * w;
    const bool resize = t.xofs != nullptr;
    const long d_sp = dst[3 * b], d_at = dst[3 * b + 1], d_gt = gt_pool ? dst[3 * b + 2] : -1;
    const long s_gt = gt_pool ? gt_src[b] : 0;
    if (d_sp < -1 || d_sp >= P || d_at < -1 || d_at >= P || d_gt < -1 || d_gt >= P || s_gt < 0 || (gt_pool && s_gt >= Q)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 4);
        return;
    }
    int flags = 0;
    if (!AT_U8 && resize && d_at >= 0 && blockIdx.x == 0) li_judge(at, b * hw, hw, flags);
    const long p0 = (long)blockIdx.x * LI_TILE + 4 * threadIdx.x;
    if (p0 < HW) {
        const int n = (int)min(4L, HW - p0);
        int q[4];
        if (d_sp >= 0) {
            li_fetch4<SP_U8, VEC>(sp, b * HW + p0, n, q, flags);
            li_put4<VEC>(late_pool + d_sp * HW + p0, q, n);
        }
        if (d_at >= 0) {
            if (!resize) li_fetch4<AT_U8, VEC>(at, b * HW + p0, n, q, flags);
            else li_resize4<AT_U8>(at, b * hw, p0, n, W, h, w, t, q);
            li_put4<VEC>(late_pool + d_at * HW + p0, q, n);
        }
        if (d_gt >= 0) {
            int ignore = 0;                         // (bytes: nothing to flag)
            li_fetch4<true, VEC>(gt_pool, s_gt * HW + p0, n, q, ignore);
            li_put4<VEC>(late_pool + d_gt * HW + p0, q, n);
        }
    }
    if (flags) atomicOr(status, flags);
}

// grid (ceil(H W / LI_NT), M); one lane per pixel
__global__ __launch_bounds__(LI_NT) void draw_ring_kernel(unsigned char* __restrict__ images, int H, int W,
                                                          const int* __restrict__ centers, long long rin2, long long rout2,
                                                          int c0, int c1, int c2) {
    const int m = blockIdx.y;
    const long p = (long)blockIdx.x * LI_NT + threadIdx.x;
    if (p >= (long)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const long long dy = (long long)y - centers[2 * m], dx = (long long)x - centers[2 * m + 1];
    const long long d2 = dy * dy + dx * dx;
    if (d2 < rin2 || d2 > rout2) return;
    unsigned char* o = images + ((long)m * H * W + p) * 3;
    o[0] = (unsigned char)c0;
    o[1] = (unsigned char)c1;
    o[2] = (unsigned char)c2;
}

inline bool li_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// sp (B, H, W) and at (B, h, w): fp32, or uint8 where sp_u8 / at_u8 is set.  Tables (hipops.linear_table, h x w -> H x W) are all
// given or, when (h, w) == (H, W), all null.  fused (B, 2, H, W) fp32; planes (B, 2, H, W) uint8 or null; status: one int on the
// device, zero-filled by the caller (bit 0: a NaN was quantised to 0, bit 1: a value outside [0, 256 / 255) was clamped).
EGZ_API int egz_late_input(const void* sp, int sp_u8, const void* at, int at_u8, int B, int H, int W, int h, int w,
                           const int* xofs, const short* xalpha, const int* yofs, const short* yalpha, float* fused,
                           unsigned char* planes, int* status, hipStream_t st) {
    EGZ_CHECK_ARG(sp && at && fused && status, "egz_late_input: null pointer");
    EGZ_CHECK_ARG(B > 0 && B <= 65535, "egz_late_input: B = %d outside 1 .. 65535", B);
    EGZ_CHECK_ARG(H > 0 && W > 0 && h > 0 && w > 0, "egz_late_input: bad geometry (%d x %d -> %d x %d)", h, w, H, W);
    const bool tables = xofs && xalpha && yofs && yalpha;
    EGZ_CHECK_ARG(tables || (!xofs && !xalpha && !yofs && !yalpha), "egz_late_input: the four resize tables go together");
    EGZ_CHECK_ARG(tables || (h == H && w == W), "egz_late_input: %d x %d -> %d x %d needs the resize tables", h, w, H, W);
    const long HW = (long)H * W;
    EGZ_CHECK_ARG((double)B * 2.0 * (double)HW * 4.0 < 4294967296.0, "egz_late_input: fused output of 4 GiB or more (B %d, %d x %d)",
                  B, H, W);
    // one 16-byte store per lane and plane needs every plane to start on a 16-byte boundary
    const bool vec = HW % 4 == 0 && li_aligned(fused, 16) && li_aligned(planes, 4) && li_aligned(sp, sp_u8 ? 4 : 16) &&
                     (tables || li_aligned(at, at_u8 ? 4 : 16));
    const LiTables t{tables ? xofs : nullptr, tables ? xalpha : nullptr, tables ? yofs : nullptr, tables ? yalpha : nullptr};
    resolve(
        [&](auto su8, auto au8, auto v) {
            hipLaunchKernelGGL((late_input_kernel<decltype(su8)::value, decltype(au8)::value, decltype(v)::value>),
                               dim3(egz_cdiv(HW, LI_TILE), B), dim3(LI_NT), 0, st, sp, at, H, W, h, w, t, fused, planes, status);
        },
        by_bool(sp_u8 != 0), by_bool(at_u8 != 0), by_bool(vec));
    EGZ_CHECK_LAUNCH("egz_late_input");
    return 0;
}

// sp (n, H, W), at (n, h, w) and the tables as egz_late_input takes them.  late_pool (P, H, W) uint8; dst (n, 3) int64 on the
// device: the planes of late_pool that take sample i's SP plane, AT plane and ground truth (-1: that plane is skipped).  gt_pool
// (Q, H, W) uint8 with gt_src (n,) int64, both or neither: plane dst[i, 2] takes a copy of plane gt_src[i] of gt_pool; without
// them the third column of dst is not read.  A row with a number outside [-1, P) in dst, or outside [0, Q) in gt_src, writes
// nothing (bit 2 of status); the planes named within one call must be distinct (the caller's to check: the order of two
// writers of one plane is not defined).  status: bits 0 and 1 as egz_late_input's, for the maps that were stored.
EGZ_API int egz_late_store(const void* sp, int sp_u8, const void* at, int at_u8, int n, int H, int W, int h, int w,
                           const int* xofs, const short* xalpha, const int* yofs, const short* yalpha, unsigned char* late_pool,
                           long P, const long* dst, const unsigned char* gt_pool, long Q, const long* gt_src, int* status,
                           hipStream_t st) {
    EGZ_CHECK_ARG(sp && at && late_pool && dst && status, "egz_late_store: null pointer");
    EGZ_CHECK_ARG(n > 0 && n <= 65535, "egz_late_store: n = %d outside 1 .. 65535", n);
    EGZ_CHECK_ARG(H > 0 && W > 0 && h > 0 && w > 0, "egz_late_store: bad geometry (%d x %d -> %d x %d)", h, w, H, W);
    EGZ_CHECK_ARG(P > 0, "egz_late_store: a pool of %ld planes", P);
    EGZ_CHECK_ARG((gt_pool != nullptr) == (gt_src != nullptr), "egz_late_store: gt_pool and gt_src go together");
    EGZ_CHECK_ARG(!gt_pool || Q > 0, "egz_late_store: a ground-truth pool of %ld planes", Q);
    const bool tables = xofs && xalpha && yofs && yalpha;
    EGZ_CHECK_ARG(tables || (!xofs && !xalpha && !yofs && !yalpha), "egz_late_store: the four resize tables go together");
    EGZ_CHECK_ARG(tables || (h == H && w == W), "egz_late_store: %d x %d -> %d x %d needs the resize tables", h, w, H, W);
    const long HW = (long)H * W;
    // one 4-byte store per lane and plane needs every plane of both pools to start on a 4-byte boundary
    const bool vec = HW % 4 == 0 && li_aligned(late_pool, 4) && li_aligned(gt_pool, 4) && li_aligned(sp, sp_u8 ? 4 : 16) &&
                     (tables || li_aligned(at, at_u8 ? 4 : 16));
    const LiTables t{tables ? xofs : nullptr, tables ? xalpha : nullptr, tables ? yofs : nullptr, tables ? yalpha : nullptr};
    resolve(
        [&](auto su8, auto au8, auto v) {
            hipLaunchKernelGGL((late_store_kernel<decltype(su8)::value, decltype(au8)::value, decltype(v)::value>),
                               dim3(egz_cdiv(HW, LI_TILE), n), dim3(LI_NT), 0, st, sp, at, H, W, h, w, t, late_pool, P, dst,
                               gt_pool, Q, gt_src, status);
        },
        by_bool(sp_u8 != 0), by_bool(at_u8 != 0), by_bool(vec));
    EGZ_CHECK_LAUNCH("egz_late_store");
    return 0;
}

// images (M, H, W, 3) uint8, written in place; centers (M, 2) int32 (row, col), anywhere; 0 <= r_in <= r_out; colour bytes in
// the images' channel order.
EGZ_API int egz_draw_ring(unsigned char* images, int M, int H, int W, const int* centers, int r_in, int r_out, int c0, int c1,
                          int c2, hipStream_t st) {
    EGZ_CHECK_ARG(images && centers, "egz_draw_ring: null pointer");
    EGZ_CHECK_ARG(M > 0 && M <= 65535 && H > 0 && W > 0, "egz_draw_ring: bad geometry (M %d, %d x %d)", M, H, W);
    EGZ_CHECK_ARG(0 <= r_in && r_in <= r_out, "egz_draw_ring: radii %d .. %d: 0 <= r_in <= r_out is needed", r_in, r_out);
    EGZ_CHECK_ARG(((c0 | c1 | c2) & ~255) == 0, "egz_draw_ring: colour (%d, %d, %d) outside 0 .. 255", c0, c1, c2);
    hipLaunchKernelGGL(draw_ring_kernel, dim3(egz_cdiv((long)H * W, LI_NT), M), dim3(LI_NT), 0, st, images, H, W, centers,
                       (long long)r_in * r_in, (long long)r_out * r_out, c0, c1, c2);
    EGZ_CHECK_LAUNCH("egz_draw_ring");
    return 0;
}
