// Baseline JPEG decode of a batch of streams on the GPU (data/STdatas.STDataset(decode='gpu')): the bytes of N files in one
// buffer, each decoded into its own uint8 (C, H, W) slot of an output tensor, bit-identical with libjpeg-turbo's default decode
// (cv2.imread).  The decode logic lives in jpeg_core.h, which the tests also build for the host under the sanitizers.
//
// Three launches on the caller's stream after a zero fill of the coefficient planes:
//   1. entropy: one wave per stream.  The stream is copied into LDS (when it fits) by the whole wave, then lane 0 parses the
//      header and Huffman-decodes the scan into int16 coefficient planes -- serial within a stream, the batch's streams in
//      parallel across the CUs.  Writes the stream's status word and an ImgInfo record for the next stages.
//   2. IDCT: one thread per 8x8 block (jpeg_idct_islow) into uint8 sample planes.
//   3. colour: one thread per output pixel: fancy upsampling + YCbCr -> BGR, or a copy of the Y plane (grayscale request /
//      one-component file, replicated for a colour request).
// Status 2 / 3 / 4 streams and invalid slots write nothing.  Streams up to SBUF bytes are read from LDS, larger ones from
// global memory; SBUF is sized so that four streams share a CU (1,024 in flight on 256 CUs).
#include "egz_common.h"
#include "jpeg_core.h"

namespace {

constexpr int SBUF = 24 * 1024;        // streams up to this size are decoded from LDS (+ ~12 KB Decoder: 4 blocks per CU)
constexpr int NT = 256;

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t info, coef, pix, total;
    long pb;                           // block capacity of one plane
};

Layout layout(int N, int H, int W, int n3) {
    Layout L;
    L.pb = (long)(2 * ((W + 15) / 16)) * (2 * ((H + 15) / 16));
    const long planes = (long)N + 2L * n3;
    L.info = 0;
    L.coef = align_up(sizeof(jpg::ImgInfo) * (size_t)N);
    L.pix = L.coef + align_up((size_t)planes * L.pb * 64 * sizeof(int16_t));
    L.total = L.pix + align_up((size_t)planes * L.pb * 64);
    return L;
}

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const uint8_t* __restrict__ data, long data_len,
                                                          const long* __restrict__ offsets, const int* __restrict__ channels,
                                                          const long* __restrict__ planes, int N, int H, int W,
                                                          long out_planes, long total_planes, long pb,
                                                          jpg::ImgInfo* __restrict__ infos, int16_t* __restrict__ coef,
                                                          int* __restrict__ status) {
    __shared__ jpg::Decoder dec;
    __shared__ uint8_t sbuf[SBUF];
    const int img = blockIdx.x, lane = threadIdx.x;
    // first workspace plane of this stream: prefix sum of the planes of the streams before it
    int acc = 0;
    for (int j = lane; j < img; j += 64) acc += channels[j] == 3 ? 3 : 1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    const long o0 = offsets[img], o1 = offsets[img + 1];
    const bool range_ok = o0 >= 0 && o1 >= o0 && o1 <= data_len;
    const long len = range_ok ? o1 - o0 : 0;
    const uint8_t* src = data + (range_ok ? o0 : 0);
    const bool in_lds = len <= SBUF;
    if (in_lds) {
#pragma unroll 8
        for (long j = lane; j < len; j += 64) sbuf[j] = src[j];
    }
    __syncthreads();
    if (lane != 0) return;
    jpg::ImgInfo& I = infos[img];
    const int want_c = channels[img];
    const long dst = planes[img];
    I.write = 0;
    I.cout = want_c;
    if (!(want_c == 1 || want_c == 3) || dst < 0 || dst + want_c > out_planes || acc + want_c > total_planes) {
        I.status = jpg::UNSUPPORTED;   // invalid request: nothing is written
        status[img] = jpg::UNSUPPORTED;
        return;
    }
    if (!range_ok) {
        I.status = jpg::FATAL;
        status[img] = jpg::FATAL;
        return;
    }
    const uint8_t* d = in_lds ? sbuf : src;
    int st = jpg::parse_header(dec, d, len, H, W, want_c);
    if (st == jpg::OK) {
        jpg::fill_info(dec, I, want_c);
        I.base_plane = acc;
        st = jpg::decode_scan(dec, I, d, len, coef + (long)acc * pb * 64, pb * 64);
        I.write = st != jpg::FATAL;
    }
    I.status = st;
    status[img] = st;
}

__global__ void __launch_bounds__(NT) jpeg_idct_kernel(const jpg::ImgInfo* __restrict__ infos,
                                                       const int16_t* __restrict__ coef, uint8_t* __restrict__ pix, long pb) {
    const jpg::ImgInfo& I = infos[blockIdx.y];
    if (I.write != 1) return;
    long t = (long)blockIdx.x * NT + threadIdx.x;
    int p = 0;
    for (; p < I.nstore; p++) {
        const long nb = (long)I.bw[p] * I.bh[p];
        if (t < nb) break;
        t -= nb;
    }
    if (p >= I.nstore) return;
    const long plane = (long)I.base_plane + p;
    const int bx = (int)(t % I.bw[p]), by = (int)(t / I.bw[p]);
    const int stride = I.bw[p] * 8;
    jpg::idct_islow(coef + (plane * pb + t) * 64, I.q[p], pix + plane * pb * 64 + (long)by * 8 * stride + bx * 8, stride);
}

__global__ void __launch_bounds__(NT) jpeg_color_kernel(const jpg::ImgInfo* __restrict__ infos, const uint8_t* __restrict__ pix,
                                                        const long* __restrict__ planes, uint8_t* __restrict__ out, int H, int W,
                                                        long pb) {
    const jpg::ImgInfo& I = infos[blockIdx.y];
    if (!I.write) return;
    const long HW = (long)H * W;
    const long px = (long)blockIdx.x * NT + threadIdx.x;
    if (px >= HW) return;
    const int y = (int)(px / W), x = (int)(px % W);
    uint8_t* o = out + planes[blockIdx.y] * HW + px;
    const int C = I.cout;
    const uint8_t* p0 = pix + (long)I.base_plane * pb * 64;
    const int s0 = I.bw[0] * 8;
    const int Y = p0[(long)y * s0 + x];
    if (C == 1 || I.nstore == 1) {
        for (int c = 0; c < C; c++) o[c * HW] = (uint8_t)Y;
        return;
    }
    const int s1 = I.bw[1] * 8;
    const int cb = jpg::chroma(p0 + pb * 64, s1, I.up, I.dw[1], I.dh[1], x, y);
    const int cr = jpg::chroma(p0 + 2 * pb * 64, s1, I.up, I.dw[2], I.dh[2], x, y);
    uint8_t bgr[3];
    jpg::ycc_bgr(Y, cb, cr, bgr);
    o[0] = bgr[0];
    o[HW] = bgr[1];
    o[2 * HW] = bgr[2];
}

}  // namespace

EGZ_API size_t egz_jpeg_decode_ws_bytes(int N, int H, int W, int n3) {
    if (N <= 0 || H <= 0 || W <= 0 || H > jpg::MAX_DIM || W > jpg::MAX_DIM || n3 < 0 || n3 > N) return 0;
    return layout(N, H, W, n3).total;
}

EGZ_API int egz_jpeg_decode(const unsigned char* data, long data_len, const long* offsets, const int* channels,
                            const long* planes, int N, int H, int W, unsigned char* out, long out_planes, int* status,
                            void* ws, size_t ws_bytes, int n3, int stages, hipStream_t stream) {
    EGZ_CHECK_ARG(N > 0 && H > 0 && W > 0 && H <= jpg::MAX_DIM && W <= jpg::MAX_DIM,
                  "egz_jpeg_decode: bad geometry N=%d H=%d W=%d (1 <= H, W <= %d)", N, H, W, jpg::MAX_DIM);
    EGZ_CHECK_ARG(n3 >= 0 && n3 <= N, "egz_jpeg_decode: n3=%d outside [0, N=%d]", n3, N);
    EGZ_CHECK_ARG(data && offsets && channels && planes && out && status && ws && data_len >= 0 && out_planes > 0,
                  "egz_jpeg_decode: null pointer or empty buffer");
    EGZ_CHECK_ARG(stages == 1 || stages == 2, "egz_jpeg_decode: stages=%d (1: entropy only, 2: all)", stages);
    const Layout L = layout(N, H, W, n3);
    EGZ_CHECK_ARG(ws_bytes >= L.total, "egz_jpeg_decode: workspace %zu bytes < %zu", ws_bytes, L.total);
    uint8_t* w = (uint8_t*)ws;
    jpg::ImgInfo* infos = (jpg::ImgInfo*)(w + L.info);
    int16_t* coef = (int16_t*)(w + L.coef);
    uint8_t* pix = w + L.pix;
    const long total_planes = (long)N + 2L * n3;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)total_planes * L.pb * 64 * sizeof(int16_t), stream);
    if (e != hipSuccess) { egz_set_error("egz_jpeg_decode: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    jpeg_entropy_kernel<<<N, 64, 0, stream>>>(data, data_len, offsets, channels, planes, N, H, W, out_planes, total_planes,
                                              L.pb, infos, coef, status);
    EGZ_CHECK_LAUNCH("egz_jpeg_decode (entropy)");
    if (stages == 1) return 0;
    jpeg_idct_kernel<<<dim3(egz_cdiv(3 * L.pb, NT), N), NT, 0, stream>>>(infos, coef, pix, L.pb);
    EGZ_CHECK_LAUNCH("egz_jpeg_decode (idct)");
    jpeg_color_kernel<<<dim3(egz_cdiv((long)H * W, NT), N), NT, 0, stream>>>(infos, pix, planes, out, H, W, L.pb);
    EGZ_CHECK_LAUNCH("egz_jpeg_decode (colour)");
    return 0;
}
