// Baseline JPEG encode of a batch of images of one geometry on the GPU: uint8 grey (N, H, W) or BGR (N, H, W, 3) in,
// N complete files out, byte-identical with libjpeg-turbo's default encoder (Pillow's Image.save, cv2.imwrite).  The
// arithmetic lives in jpeg_enc_core.h, which the tests also build for the host under the sanitizers.
//
// egz_jpeg_encode runs, on the caller's stream,
//   1. setup: one thread writes the call's header bytes, quantisation and Huffman code tables (jpge::Setup) to the workspace;
//   2. transform: one thread per 8x8 block of the scan -- colour conversion, edge replication, chroma down-sampling, FDCT,
//      quantisation -> int16 coefficients in zigzag order, the block's DC and the scan bits of its AC part;
//   3. count: one thread per block adds the bits of its DC difference (the predecessor's index is a closed form) and a
//      workgroup sums SCAN_CHUNK blocks; 4. an exclusive scan of the chunk sums per image (any number of chunks);
//   5. zero fill of the words of the bit buffer the image will use; 6. pack: one thread per block, its bit position from
//      the chunk offset plus a workgroup scan, Huffman tables in LDS, codes OR-ed into the bit buffer with 32-bit atomics
//      (neighbouring blocks share boundary words);
//   7. 0xFF count per BYTE_CHUNK bytes of the padded bit buffer; 8. exclusive scan of those per image, which also gives the
//      length the file needs.
// egz_jpeg_encode_write then scatters header, stuffed scan and EOI into each image's slot of the output -- or nothing at all,
// with status 1, where the slot is smaller than the length needed.  Between the two calls the caller may read the N lengths
// back to allocate the exact output; nothing else happens on the host.
#include "egz_common.h"
#include "jpeg_enc_core.h"

namespace {

constexpr int NT = 256;
constexpr int SCAN_CHUNK = NT;         // blocks per workgroup of the count / pack stages
constexpr int BYTE_CHUNK = NT * 16;    // scan bytes per workgroup of the stuffing stages: four 32-bit words per thread

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t setup, coef, dc, acb, csum, words, fsum, tot, total;
    long nblk, nchunk, wpi, nbchunk;   // per image: blocks, block chunks, bit-buffer words, byte chunks
};

Layout layout(int N, const jpge::Geo& g) {
    Layout L;
    L.nblk = g.nblk;
    L.nchunk = (L.nblk + SCAN_CHUNK - 1) / SCAN_CHUNK;
    L.wpi = (L.nblk * (long)jpge::MAX_BLOCK_BITS + 31) / 32 + 1;
    L.nbchunk = (L.wpi * 4 + BYTE_CHUNK - 1) / BYTE_CHUNK;
    size_t o = 0;
    L.setup = o; o += align_up(sizeof(jpge::Setup));
    L.coef = o; o += align_up((size_t)N * L.nblk * 64 * sizeof(int16_t));
    L.dc = o; o += align_up((size_t)N * L.nblk * sizeof(int16_t));
    L.acb = o; o += align_up((size_t)N * L.nblk * sizeof(uint16_t));
    L.csum = o; o += align_up((size_t)N * L.nchunk * sizeof(uint32_t));
    L.words = o; o += align_up((size_t)N * L.wpi * sizeof(uint32_t));
    L.fsum = o; o += align_up((size_t)N * L.nbchunk * sizeof(uint32_t));
    L.tot = o; o += align_up((size_t)N * 2 * sizeof(unsigned long long));     // per image: scan bits, 0xFF bytes
    L.total = o;
    return L;
}

__global__ void setup_kernel(jpge::Setup* s, jpge::Geo g, int quality) {
    if (blockIdx.x == 0 && threadIdx.x == 0) jpge::setup(*s, g, quality);
}

__global__ void __launch_bounds__(NT) transform_kernel(const uint8_t* __restrict__ img, jpge::Geo g, long img_bytes,
                                                       const jpge::Setup* __restrict__ setup, int16_t* __restrict__ coef,
                                                       int16_t* __restrict__ dc, uint16_t* __restrict__ acb) {
    __shared__ jpge::Setup s;          // only q and ac_size are read; the copy is a few hundred words
    for (int i = threadIdx.x; i < (int)(sizeof(jpge::Setup) / 4); i += NT) ((uint32_t*)&s)[i] = ((const uint32_t*)setup)[i];
    __syncthreads();
    const long b = (long)blockIdx.x * NT + threadIdx.x;
    if (b >= g.nblk) return;
    const long n = blockIdx.y;
    int16_t zz[64];
    jpge::block_coefs(g, s, img + n * img_bytes, (int)b, zz);
    const long gb = n * g.nblk + b;
    uint4* o = (uint4*)(coef + gb * 64);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint4 v;
        v.x = (uint16_t)zz[8 * i + 0] | ((uint32_t)(uint16_t)zz[8 * i + 1] << 16);
        v.y = (uint16_t)zz[8 * i + 2] | ((uint32_t)(uint16_t)zz[8 * i + 3] << 16);
        v.z = (uint16_t)zz[8 * i + 4] | ((uint32_t)(uint16_t)zz[8 * i + 5] << 16);
        v.w = (uint16_t)zz[8 * i + 6] | ((uint32_t)(uint16_t)zz[8 * i + 7] << 16);
        o[i] = v;
    }
    dc[gb] = zz[0];
    acb[gb] = (uint16_t)jpge::ac_bits(zz, s.ac_size[jpge::block_comp(g, (int)b) ? 1 : 0]);
}

// Scan bits of block b of image n: AC bits + the bits of its DC difference
__device__ __forceinline__ uint32_t block_bits(const jpge::Geo& g, const jpge::Setup* __restrict__ setup,
                                               const int16_t* __restrict__ dc, const uint16_t* __restrict__ acb, long n,
                                               long b, int* prev_dc) {
    const long base = n * g.nblk;
    const int pb = jpge::prev_block(g, (int)b);
    const int pd = pb < 0 ? 0 : dc[base + pb];
    *prev_dc = pd;
    const int t = jpge::block_comp(g, (int)b) ? 1 : 0;
    return (uint32_t)acb[base + b] + (uint32_t)jpge::dc_bits(dc[base + b] - pd, setup->dc_size[t]);
}

// Exclusive scan of one value per thread over the workgroup; *total: the sum.  `sh` holds NT / 64 words.
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();                   // sh may still be read from an earlier call
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        if (w < wave) before += sh[w];
        all += sh[w];
    }
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(NT) count_kernel(jpge::Geo g, const jpge::Setup* __restrict__ setup,
                                                   const int16_t* __restrict__ dc, const uint16_t* __restrict__ acb,
                                                   uint32_t* __restrict__ csum, long nchunk) {
    __shared__ uint32_t sh[NT / 64];
    const long b = (long)blockIdx.x * SCAN_CHUNK + threadIdx.x, n = blockIdx.y;
    int pd;
    const uint32_t bits = b < g.nblk ? block_bits(g, setup, dc, acb, n, b, &pd) : 0;
    uint32_t total;
    wg_exclusive_scan(bits, sh, &total);
    if (threadIdx.x == 0) csum[n * nchunk + blockIdx.x] = total;
}

// In-place exclusive scan of each image's `count` values (one workgroup per image, tiles of NT with a carry); the sum goes
// to tot[2 * n + slot].  count_of: per-image number of valid values (tot-derived) or the fixed `count`.
__global__ void __launch_bounds__(NT) chunk_scan_kernel(uint32_t* __restrict__ vals, long stride, long count,
                                                        unsigned long long* __restrict__ tot, int slot) {
    __shared__ uint32_t sh[NT / 64];
    const long n = blockIdx.x;
    if (slot == 1) {                   // byte chunks in use: from the scan bits of this image
        const unsigned long long nbytes = (tot[2 * n] + 7) / 8;
        count = (long)((nbytes + BYTE_CHUNK - 1) / BYTE_CHUNK);
    }
    uint32_t* v = vals + n * stride;
    unsigned long long carry = 0;
    for (long t0 = 0; t0 < count; t0 += NT) {
        const long i = t0 + threadIdx.x;
        const uint32_t x = i < count ? v[i] : 0;
        uint32_t total;
        const uint32_t ex = wg_exclusive_scan(x, sh, &total);
        if (i < count) v[i] = (uint32_t)carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tot[2 * n + slot] = carry;
}

__global__ void __launch_bounds__(NT) zero_kernel(uint32_t* __restrict__ words, long wpi,
                                                  const unsigned long long* __restrict__ tot) {
    const long n = blockIdx.y;
    long need = (long)((tot[2 * n] + 31) / 32) + 1;
    if (need > wpi) need = wpi;
    uint32_t* w = words + n * wpi;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < need; i += (long)gridDim.x * NT) w[i] = 0;
}

// Bit sink of the pack stage: codes are OR-ed into big-endian 32-bit words of a zero-filled buffer
struct WordSink {
    uint32_t* w;                       // next word
    long left;                         // words that may still be written
    uint64_t acc;
    int nacc;
    __device__ __forceinline__ void flush_word(uint32_t v) {
        if (left > 0) {
            if (v) atomicOr(w, v);
            w++;
            left--;
        }
    }
    __device__ __forceinline__ void put(uint32_t v, int len) {
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            flush_word((uint32_t)(acc >> (nacc - 32)));
            nacc -= 32;
            acc &= ((uint64_t)1 << nacc) - 1;
        }
    }
};

__global__ void __launch_bounds__(NT) pack_kernel(jpge::Geo g, const jpge::Setup* __restrict__ setup,
                                                  const int16_t* __restrict__ coef, const int16_t* __restrict__ dc,
                                                  const uint16_t* __restrict__ acb, const uint32_t* __restrict__ csum,
                                                  long nchunk, uint32_t* __restrict__ words, long wpi) {
    __shared__ uint32_t sh[NT / 64];
    __shared__ uint16_t dc_code[2][16], ac_code[2][256];
    __shared__ uint8_t dc_size[2][16], ac_size[2][256];
    for (int i = threadIdx.x; i < 32; i += NT) {
        (&dc_code[0][0])[i] = (&setup->dc_code[0][0])[i];
        (&dc_size[0][0])[i] = (&setup->dc_size[0][0])[i];
    }
    for (int i = threadIdx.x; i < 512; i += NT) {
        (&ac_code[0][0])[i] = (&setup->ac_code[0][0])[i];
        (&ac_size[0][0])[i] = (&setup->ac_size[0][0])[i];
    }
    const long b = (long)blockIdx.x * SCAN_CHUNK + threadIdx.x, n = blockIdx.y;
    int pd = 0;
    const uint32_t bits = b < g.nblk ? block_bits(g, setup, dc, acb, n, b, &pd) : 0;
    uint32_t total;
    const uint32_t ex = wg_exclusive_scan(bits, sh, &total);       // its barriers also publish the tables
    if (b >= g.nblk) return;
    const uint64_t pos = (uint64_t)csum[n * nchunk + blockIdx.x] + ex;
    int16_t zz[64];
    const uint4* src = (const uint4*)(coef + (n * g.nblk + b) * 64);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 v = src[i];
        zz[8 * i + 0] = (int16_t)(v.x & 0xFFFF); zz[8 * i + 1] = (int16_t)(v.x >> 16);
        zz[8 * i + 2] = (int16_t)(v.y & 0xFFFF); zz[8 * i + 3] = (int16_t)(v.y >> 16);
        zz[8 * i + 4] = (int16_t)(v.z & 0xFFFF); zz[8 * i + 5] = (int16_t)(v.z >> 16);
        zz[8 * i + 6] = (int16_t)(v.w & 0xFFFF); zz[8 * i + 7] = (int16_t)(v.w >> 16);
    }
    const long w0 = (long)(pos >> 5);
    WordSink sink;
    sink.w = words + n * wpi + w0;
    sink.left = wpi - w0;
    sink.acc = 0;
    sink.nacc = (int)(pos & 31);       // the bits before this block in its first word are another block's: zeros here
    const int t = jpge::block_comp(g, (int)b) ? 1 : 0;
    jpge::emit_block(zz, pd, dc_code[t], dc_size[t], ac_code[t], ac_size[t], sink);
    if (sink.nacc) sink.flush_word((uint32_t)(sink.acc << (32 - sink.nacc)));
}

// Word i of an image's scan with the last byte padded with 1-bits; words past the scan read as 0
__device__ __forceinline__ uint32_t scan_word(const uint32_t* __restrict__ w, long i, unsigned long long bits) {
    const long nw = (long)((bits + 31) / 32);
    if (i >= nw) return 0;
    uint32_t v = w[i];
    if (i == nw - 1) {
        const int used = (int)(bits - (unsigned long long)i * 32);   // 1 .. 32
        const int padded = (used + 7) & ~7;
        if (padded > used) v |= ((1u << (padded - used)) - 1) << (32 - padded);
    }
    return v;
}

__device__ __forceinline__ int count_ff(uint32_t v, int nbytes) {   // among the first nbytes (big-endian) bytes of v
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) c += (k < nbytes && ((v >> (24 - 8 * k)) & 0xFF) == 0xFF) ? 1 : 0;
    return c;
}

// 0xFF bytes among this thread's four words (bytes [16 t, 16 t + 16) of the chunk, cut at the scan's length)
__device__ __forceinline__ uint32_t thread_ff(const uint32_t* __restrict__ w, unsigned long long bits, long byte0,
                                              uint32_t* v) {
    const long nbytes = (long)((bits + 7) / 8);
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long b0 = byte0 + 4 * k;
        v[k] = b0 < nbytes ? scan_word(w, b0 >> 2, bits) : 0;
        const long left = nbytes - b0;
        c += count_ff(v[k], left >= 4 ? 4 : (left > 0 ? (int)left : 0));
    }
    return c;
}

__global__ void __launch_bounds__(NT) ff_count_kernel(const uint32_t* __restrict__ words, long wpi,
                                                      const unsigned long long* __restrict__ tot,
                                                      uint32_t* __restrict__ fsum, long nbchunk) {
    __shared__ uint32_t sh[NT / 64];
    const long n = blockIdx.y;
    const unsigned long long bits = tot[2 * n];
    const long chunk0 = (long)blockIdx.x * BYTE_CHUNK;
    if (chunk0 >= (long)((bits + 7) / 8)) return;                   // whole workgroup
    uint32_t v[4], total;
    const uint32_t c = thread_ff(words + n * wpi, bits, chunk0 + 16 * threadIdx.x, v);
    wg_exclusive_scan(c, sh, &total);
    if (threadIdx.x == 0) fsum[n * nbchunk + blockIdx.x] = total;
}

__global__ void needed_kernel(const jpge::Setup* __restrict__ setup, const unsigned long long* __restrict__ tot,
                              long* __restrict__ needed, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) needed[n] = setup->hdr_len + (long)((tot[2 * n] + 7) / 8) + (long)tot[2 * n + 1] + 2;
}

__global__ void __launch_bounds__(NT) write_kernel(const jpge::Setup* __restrict__ setup, const uint32_t* __restrict__ words,
                                                   long wpi, const unsigned long long* __restrict__ tot,
                                                   const uint32_t* __restrict__ fsum, long nbchunk,
                                                   uint8_t* __restrict__ out, long out_bytes,
                                                   const long* __restrict__ slot_off, const long* __restrict__ slot_cap,
                                                   long* __restrict__ lengths, int* __restrict__ status) {
    __shared__ uint32_t sh[NT / 64];
    const long n = blockIdx.y;
    const unsigned long long bits = tot[2 * n];
    const long nbytes = (long)((bits + 7) / 8);
    const int hdr = setup->hdr_len;
    const long need = hdr + nbytes + (long)tot[2 * n + 1] + 2;
    const long off = slot_off[n], cap = slot_cap[n];
    const bool fits = off >= 0 && cap >= need && off <= out_bytes - need;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lengths[n] = need;
        status[n] = fits ? jpge::OK : jpge::TOO_SMALL;
    }
    const long chunk0 = (long)blockIdx.x * BYTE_CHUNK;
    if (!fits || chunk0 >= nbytes) return;                          // whole workgroup
    uint8_t* o = out + off;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < hdr; i += NT) o[i] = setup->hdr[i];
    const long byte0 = chunk0 + 16 * threadIdx.x;
    uint32_t v[4], total;
    const uint32_t c = thread_ff(words + n * wpi, bits, byte0, v);
    const uint32_t ex = wg_exclusive_scan(c, sh, &total);
    long p = hdr + byte0 + (long)fsum[n * nbchunk + blockIdx.x] + ex;   // < need - 2 for every byte below
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (byte0 + k < nbytes) {
            const uint8_t by = (uint8_t)(v[k >> 2] >> (24 - 8 * (k & 3)));
            o[p++] = by;
            if (by == 0xFF) o[p++] = 0;
        }
    }
    if (byte0 < nbytes && byte0 + 16 >= nbytes) {                   // the thread that holds the last byte
        o[need - 2] = 0xFF;
        o[need - 1] = 0xD9;
    }
}

int check_args(const char* who, int N, int H, int W, int C, int quality, int subsampling, jpge::Geo& g) {
    EGZ_CHECK_ARG(N > 0 && N <= 65535, "%s: N=%d outside 1 .. 65535", who, N);
    EGZ_CHECK_ARG(H > 0 && W > 0 && H <= jpge::MAX_DIM && W <= jpge::MAX_DIM, "%s: bad geometry H=%d W=%d (1 <= H, W <= %d)", who,
                  H, W, jpge::MAX_DIM);
    EGZ_CHECK_ARG(C == 1 || C == 3, "%s: channels=%d (1: grey, 3: interleaved BGR)", who, C);
    EGZ_CHECK_ARG(quality >= 1 && quality <= 100, "%s: quality=%d outside 1 .. 100", who, quality);
    EGZ_CHECK_ARG(subsampling == 420, "%s: subsampling=%d: only 4:2:0 (420) is built; 4:4:4 and 4:2:2 are not", who, subsampling);
    jpge::make_geo(g, H, W, C);
    return 0;
}

}  // namespace

EGZ_API size_t egz_jpeg_encode_ws_bytes(int N, int H, int W, int C) {
    jpge::Geo g;
    if (N <= 0 || N > 65535 || !jpge::make_geo(g, H, W, C)) return 0;
    return layout(N, g).total;
}

EGZ_API int egz_jpeg_encode(const unsigned char* images, int N, int H, int W, int C, int quality, int subsampling,
                            void* ws, size_t ws_bytes, long* needed, int stages, hipStream_t stream) {
    jpge::Geo g;
    if (int rc = check_args("egz_jpeg_encode", N, H, W, C, quality, subsampling, g)) return rc;
    EGZ_CHECK_ARG(images && ws && needed, "egz_jpeg_encode: null pointer");
    EGZ_CHECK_ARG(stages >= 1 && stages <= 4, "egz_jpeg_encode: stages=%d (1: transform, 2: + scan, 3: + pack, 4: all)", stages);
    const Layout L = layout(N, g);
    EGZ_CHECK_ARG(ws_bytes >= L.total, "egz_jpeg_encode: workspace %zu bytes < %zu", ws_bytes, L.total);
    uint8_t* w = (uint8_t*)ws;
    jpge::Setup* setup = (jpge::Setup*)(w + L.setup);
    int16_t* coef = (int16_t*)(w + L.coef);
    int16_t* dc = (int16_t*)(w + L.dc);
    uint16_t* acb = (uint16_t*)(w + L.acb);
    uint32_t* csum = (uint32_t*)(w + L.csum);
    uint32_t* words = (uint32_t*)(w + L.words);
    uint32_t* fsum = (uint32_t*)(w + L.fsum);
    unsigned long long* tot = (unsigned long long*)(w + L.tot);
    setup_kernel<<<1, 64, 0, stream>>>(setup, g, quality);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (setup)");
    transform_kernel<<<dim3(egz_cdiv(L.nblk, NT), N), NT, 0, stream>>>(images, g, (long)H * W * C, setup, coef, dc, acb);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (transform)");
    if (stages == 1) return 0;
    count_kernel<<<dim3((unsigned)L.nchunk, N), NT, 0, stream>>>(g, setup, dc, acb, csum, L.nchunk);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (count)");
    chunk_scan_kernel<<<N, NT, 0, stream>>>(csum, L.nchunk, L.nchunk, tot, 0);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (scan)");
    if (stages == 2) return 0;
    const long zgrid = L.wpi / (NT * 8) + 1;
    zero_kernel<<<dim3((unsigned)(zgrid > 64 ? 64 : zgrid), N), NT, 0, stream>>>(words, L.wpi, tot);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (zero)");
    pack_kernel<<<dim3((unsigned)L.nchunk, N), NT, 0, stream>>>(g, setup, coef, dc, acb, csum, L.nchunk, words, L.wpi);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (pack)");
    if (stages == 3) return 0;
    ff_count_kernel<<<dim3((unsigned)L.nbchunk, N), NT, 0, stream>>>(words, L.wpi, tot, fsum, L.nbchunk);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (0xFF count)");
    chunk_scan_kernel<<<N, NT, 0, stream>>>(fsum, L.nbchunk, 0, tot, 1);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (0xFF scan)");
    needed_kernel<<<egz_cdiv(N, NT), NT, 0, stream>>>(setup, tot, needed, N);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode (lengths)");
    return 0;
}

EGZ_API int egz_jpeg_encode_write(const void* ws, size_t ws_bytes, int N, int H, int W, int C, unsigned char* out,
                                  long out_bytes, const long* slot_off, const long* slot_cap, long* lengths, int* status,
                                  hipStream_t stream) {
    jpge::Geo g;
    if (int rc = check_args("egz_jpeg_encode_write", N, H, W, C, 95, 420, g)) return rc;
    EGZ_CHECK_ARG(ws && out && slot_off && slot_cap && lengths && status && out_bytes > 0,
                  "egz_jpeg_encode_write: null pointer or empty output");
    const Layout L = layout(N, g);
    EGZ_CHECK_ARG(ws_bytes >= L.total, "egz_jpeg_encode_write: workspace %zu bytes < %zu", ws_bytes, L.total);
    const uint8_t* w = (const uint8_t*)ws;
    write_kernel<<<dim3((unsigned)L.nbchunk, N), NT, 0, stream>>>(
        (const jpge::Setup*)(w + L.setup), (const uint32_t*)(w + L.words), L.wpi, (const unsigned long long*)(w + L.tot),
        (const uint32_t*)(w + L.fsum), L.nbchunk, out, out_bytes, slot_off, slot_cap, lengths, status);
    EGZ_CHECK_LAUNCH("egz_jpeg_encode_write");
    return 0;
}
