// Dataset preparation (data/dataset_preprocessing.py, misc/gazedataset_gt.py of the reference): the ground-truth gaze map of a
// frame is a unit impulse at (r, c) in an H x W float64 array, scipy.ndimage.gaussian_filter(sigma) of it ('reflect' boundary,
// truncate 4), min-max normalised, times 255, then cv2.resize(INTER_AREA) to oh x ow and stored as uint8.  One block renders
// one frame; the full-resolution map never exists.
//
// The filtered impulse is separable.  scipy correlates axis 0 first: row i of the intermediate is 0 except at column c, where
// it holds gy[i] = the 1-D response at i to a unit impulse at r.  The second pass along axis 1 gives
//   M[i, j] = F_j(gy[i]),   F_j(v) = fl(fl([j == c] v) w0) (+) fl(fl(m_1 v) w_k1) (+) fl(fl(m_2 v) w_k2) (+) fl(fl(m_3 v) w_k3)
// with k1 > k2 > k3 the (at most three) tap distances whose reflected index hits c and m the number of hits (1 or 2) -- the
// terms scipy adds in its own order (centre tap, then |k| = R .. 1), all others being exact zeros (metrics.hip makes the same
// construction for its AUC field).  Every term is a product of non-negative factors and rounding is monotone, so F_j is
// non-decreasing and min M = min_j F_j(min gy), max M = max_j F_j(max gy): the reference's normalisation
//   G = ((M - min M) / max(M - min M)) * 255
// is evaluated per source pixel with the same doubles numpy holds.  The area resize follows OpenCV's generic INTER_AREA path
// (ResizeArea_Invoker) with host-built tables: per output row, per source row of its y-entries, buf = sum_x S * alpha in table
// order, then sum = beta * buf for the first y-entry and sum += beta * buf after it.
//   mode 0 (GTEA Gaze+):  S = G (double), double accumulation, u8 = saturate(rint(sum))  -- cv2.imwrite of the float64 image
//   mode 1 (GTEA Gaze):   S = (float)(uint8)G (truncation, np.uint8), float accumulation, u8 = saturate(rintf(sum))
// Every operation below is a separate IEEE operation: contraction into FMA is off for this file (build.sh flags unchanged).
#include "egz_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;              // 4 waves per frame
constexpr int NWV = NT / 64;

// The <= 3 tap distances k in [1, R] (descending, scipy's order) at which the 1-D correlation at p of a line that is non-zero
// only at c picks up c, with their multiplicities, for 'reflect' with R < n (one reflection at most):
//   p + k = c (c > p),  p - k = c (p > c)     -> kd = |p - c|
//   2n - 1 - (p + k) = c                      -> ka = 2n - 1 - p - c      (p + k >= n holds for this k)
//   -(p - k) - 1 = c                          -> kb = p + c + 1           (p - k < 0 holds for this k)
// kd differs from ka and kb for every p, c; ka == kb (p + c = n - 1) is one tap hit from both sides (multiplicity 2).
__device__ __forceinline__ void tap_terms(int p, int c, int n, int R, int k[3], int m[3]) {
    int kd = p > c ? p - c : c - p, ka = 2 * n - 1 - p - c, kb = p + c + 1;
    int md = 1, ma = 1, mb = 1;
    if (ka == kb) { ma = 2; mb = 0; kb = 0; }
    if (kd > R) { kd = 0; }
    if (ka > R) { ka = 0; }
    if (kb > R) { kb = 0; }
    if (kd == 0) md = 0;
    if (ka == 0) ma = 0;
    if (kb == 0) mb = 0;
    // sort the three (k, m) pairs by k, descending (k = 0 marks an unused slot and sorts last)
    auto swap_if = [](int& k0, int& m0, int& k1, int& m1) {
        if (k1 > k0) { const int t = k0; k0 = k1; k1 = t; const int u = m0; m0 = m1; m1 = u; }
    };
    swap_if(kd, md, ka, ma);
    swap_if(ka, ma, kb, mb);
    swap_if(kd, md, ka, ma);
    k[0] = kd; m[0] = md; k[1] = ka; m[1] = ma; k[2] = kb; m[2] = mb;
}

__device__ __forceinline__ double block_reduce(double v, bool is_max, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        v = is_max ? fmax(v, o) : fmin(v, o);
    }
    __syncthreads();                 // red[] may still be read by a previous reduction
    if (lane == 0) red[wave] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) v = is_max ? fmax(v, red[w]) : fmin(v, red[w]);
    return v;
}

// LDS (dynamic): gy[H] doubles, then per source column its three tap weights ccoef[3 W] (0 when unused) and a flag word
// cmeta[W] = centre | m_1 << 1 | m_2 << 3 | m_3 << 5.
__global__ __launch_bounds__(NT) void gaze_gt_kernel(const int* __restrict__ pos, int H, int W, const double* __restrict__ gw,
                                                     int R, const int* __restrict__ xofs, const int* __restrict__ xsi,
                                                     const float* __restrict__ xalpha, int nx, const int* __restrict__ yofs,
                                                     const int* __restrict__ ysi, const float* __restrict__ yalpha, int ny,
                                                     int mode, int oh, int ow, unsigned char* __restrict__ out_u8,
                                                     double* __restrict__ out_f64, double* __restrict__ out_full) {
    extern __shared__ double lds[];
    __shared__ double red[NWV];
    double* gy = lds;
    double* ccoef = lds + H;
    int* cmeta = reinterpret_cast<int*>(ccoef + 3 * W);

    const int f = blockIdx.x, tid = threadIdx.x;
    const int r = pos[2 * f], c = pos[2 * f + 1];
    const double w0 = gw[R];

    // 1. gy[i]: axis-0 response to the unit impulse (in scipy's order; (1 + 1) w == (2 * 1) w)
    double vmin = INFINITY, vmax = -INFINITY;
    for (int i = tid; i < H; i += NT) {
        int k[3], m[3];
        tap_terms(i, r, H, R, k, m);
        double t = (i == r ? 1.0 : 0.0) * w0;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (m[q]) t = t + (double)m[q] * gw[R + k[q]];
        gy[i] = t;
        vmin = fmin(vmin, t);
        vmax = fmax(vmax, t);
    }
    // 2. per column: the axis-1 terms
    for (int j = tid; j < W; j += NT) {
        int k[3], m[3];
        tap_terms(j, c, W, R, k, m);
        int meta = j == c ? 1 : 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            ccoef[3 * j + q] = m[q] ? gw[R + k[q]] : 0.0;
            meta |= m[q] << (1 + 2 * q);
        }
        cmeta[j] = meta;
    }
    vmin = block_reduce(vmin, false, red);
    vmax = block_reduce(vmax, true, red);      // its leading __syncthreads also publishes gy / ccoef / cmeta

    auto fval = [&](double v, int j) -> double {
        const int meta = cmeta[j];
        double t = (meta & 1) ? v * w0 : 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int mq = (meta >> (1 + 2 * q)) & 3;
            if (mq) t = t + ((double)mq * v) * ccoef[3 * j + q];
        }
        return t;
    };

    // 3. min M, max M from the extreme rows
    double zmin = INFINITY, zmax = -INFINITY;
    for (int j = tid; j < W; j += NT) {
        zmin = fmin(zmin, fval(vmin, j));
        zmax = fmax(zmax, fval(vmax, j));
    }
    const double mmin = block_reduce(zmin, false, red);
    const double den = block_reduce(zmax, true, red) - mmin;      // max(M - min M): subtraction is monotone too
    auto gval = [&](double v, int j) -> double { return ((fval(v, j) - mmin) / den) * 255.0; };

    // 4. area resize, one output pixel per thread and step
    const long npix = (long)oh * ow;
    unsigned char* o8 = out_u8 + (long)f * npix;
    for (int idx = tid; idx < npix; idx += NT) {
        const int dy = idx / ow, dx = idx - dy * ow;
        const int y0 = min(max(yofs[dy], 0), ny), y1 = min(max(yofs[dy + 1], y0), ny);
        const int x0 = min(max(xofs[dx], 0), nx), x1 = min(max(xofs[dx + 1], x0), nx);
        double res;
        unsigned char u8;
        if (mode == 0) {
            double sum = 0.0;
            for (int e = y0; e < y1; ++e) {
                const double v = gy[min(max(ysi[e], 0), H - 1)];
                double buf = 0.0;
                for (int q = x0; q < x1; ++q)
                    buf = buf + gval(v, min(max(xsi[q], 0), W - 1)) * (double)xalpha[q];
                const double t = (double)yalpha[e] * buf;
                sum = e == y0 ? t : sum + t;
            }
            res = sum;
            u8 = (unsigned char)fmin(fmax(__builtin_rint(sum), 0.0), 255.0);
        } else {
            float sum = 0.f;
            for (int e = y0; e < y1; ++e) {
                const double v = gy[min(max(ysi[e], 0), H - 1)];
                float buf = 0.f;
                for (int q = x0; q < x1; ++q) {
                    const float s = (float)(unsigned char)(int)gval(v, min(max(xsi[q], 0), W - 1));
                    buf = buf + s * xalpha[q];
                }
                const float t = yalpha[e] * buf;
                sum = e == y0 ? t : sum + t;
            }
            res = (double)sum;
            u8 = (unsigned char)fminf(fmaxf(__builtin_rintf(sum), 0.f), 255.f);
        }
        o8[idx] = u8;
        if (out_f64) out_f64[(long)f * npix + idx] = res;
    }

    // 5. the normalised full-resolution map (tests)
    if (out_full) {
        double* of = out_full + (long)f * H * W;
        for (long idx = tid; idx < (long)H * W; idx += NT) {
            const int i = (int)(idx / W), j = (int)(idx - (long)i * W);
            of[idx] = gval(gy[i], j);
        }
    }
}

}  // namespace

// pos: (N, 2) ints (row, col) in [0, H) x [0, W).  gw: the 2R + 1 weights of scipy's 1-D gaussian kernel, R < min(H, W).
// x / y tables: OpenCV's INTER_AREA decimation tables, entries [ofs[d], ofs[d + 1]) of (source index si, float alpha) for output
// index d; ofs has ow + 1 (oh + 1) entries, the tables nx (ny).  out_u8: (N, oh, ow); out_f64 (nullable): (N, oh, ow) resized
// maps before the uint8 conversion; out_full (nullable): (N, H, W) normalised full-resolution maps.
EGZ_API int egz_gaze_gt_maps(const int* pos, int N, int H, int W, const double* gw, int R, const int* xofs, const int* xsi,
                             const float* xalpha, int nx, const int* yofs, const int* ysi, const float* yalpha, int ny,
                             int mode, int oh, int ow, unsigned char* out_u8, double* out_f64, double* out_full,
                             hipStream_t st) {
    EGZ_CHECK_ARG(pos && gw && xofs && xsi && xalpha && yofs && ysi && yalpha && out_u8,
                  "egz_gaze_gt_maps: null pointer");
    EGZ_CHECK_ARG(N > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, "egz_gaze_gt_maps: empty batch or map (N %d, %d x %d -> %d x %d)",
                  N, H, W, oh, ow);
    EGZ_CHECK_ARG(oh <= H && ow <= W, "egz_gaze_gt_maps: INTER_AREA here only shrinks (%d x %d -> %d x %d)", H, W, oh, ow);
    EGZ_CHECK_ARG(R >= 1 && R < H && R < W, "egz_gaze_gt_maps: kernel radius %d must be in [1, min(H, W))", R);
    EGZ_CHECK_ARG(mode == 0 || mode == 1, "egz_gaze_gt_maps: mode %d is neither 0 (double) nor 1 (uint8 source)", mode);
    EGZ_CHECK_ARG(nx >= ow && ny >= oh, "egz_gaze_gt_maps: area tables shorter than the output (%d, %d)", nx, ny);
    const size_t lds = sizeof(double) * ((size_t)H + 3 * (size_t)W) + sizeof(int) * (size_t)W;
    EGZ_CHECK_ARG(lds <= 64 * 1024, "egz_gaze_gt_maps: %d x %d source needs %zu bytes of LDS (64 KiB at most)", H, W, lds);
    hipLaunchKernelGGL(gaze_gt_kernel, dim3(N), dim3(NT), lds, st, pos, H, W, gw, R, xofs, xsi, xalpha, nx, yofs, ysi, yalpha,
                       ny, mode, oh, ow, out_u8, out_f64, out_full);
    EGZ_CHECK_LAUNCH("egz_gaze_gt_maps");
    return 0;
}
