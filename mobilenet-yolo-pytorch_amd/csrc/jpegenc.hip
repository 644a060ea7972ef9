// Baseline JPEG encode (include/mnyolo.h: mny_jpeg_enc_layout, mny_jpeg_coef_batch, mny_jpeg_huffman_batch): the mirror image of
// csrc/jpeg.hip.  The host half, the item records and the Huffman coding of the coefficients into streams, is csrc/jpegenc_host.h
// and is only exported here; this file is the device half, everything per pixel, as one launch over the whole batch:
//   jpeg_fdct_kernel : one 256-thread workgroup takes 32 consecutive 8x8 blocks of one image's padded grids, eight lanes per
//                      block.  Lane r forms row r of the block's samples straight from the packed RGB (colour conversion, edge
//                      repeats and chroma down-sampling are per sample, so no intermediate plane exists), transforms the row
//                      and parks it in LDS; lane c then transforms column c and quantises it in place; lane r stores row r
//                      as 8 int16 in one 16-byte word (the 32 blocks are 4 KiB contiguous).  A block is 72 dwords apart from
//                      the next in LDS, as in jpeg_idct_kernel.  Blocks of the padded grid outside the component's own grid
//                      are skipped: the host stage codes them without reading them.
// The job list is jpeg.hip's (csrc/jpeg_jobs.h); the grid is capped and strides over it.  Integer arithmetic only; no atomics.
#include "common.h"
#include "jpeg_jobs.h"
#include "jpegenc_host.h"

namespace mny {
namespace {

using namespace jpeg_jobs;

constexpr int kMaxSide = 16383;
constexpr size_t kWsBytes = 256;         // the status word
constexpr int kJobBlocks = 32;           // 8x8 blocks per job
constexpr int kBlkDw = 72;               // LDS dwords from one block to the next: 64 + 8

typedef short short8 __attribute__((ext_vector_type(8)));

__device__ bool enc_sound(const mny_jpeg_item* it, const mny_image_desc& d, int max_h, int max_w) {
    if (it->status != MNY_JPEG_OK || it->ncomp != 3) return false;
    const int h = it->h, w = it->w, hs = it->hs, vs = it->vs;
    if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return false;
    if (!((hs == 1 || hs == 2) && vs >= 1 && vs <= hs)) return false;
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        const int bw = mcux * (c == 0 ? hs : 1), bh = mcuy * (c == 0 ? vs : 1);
        if (it->bw[c] != bw || it->bh[c] != bh || it->plane_off[c] != off) return false;
        off += (int64_t)bw * bh * 64;
    }
    if (it->n_coef != off) return false;
    if (it->coef_off < 0 || (it->coef_off & 7)) return false;
    if (d.offset < 0 || (d.offset & 15)) return false;
    if (d.h != h || d.w != w || h > max_h || w > max_w) return false;
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k)
            if (it->q[c][k] < 1 || it->q[c][k] > 255) return false;
    return true;
}

// one sample of component c of the pixel at (y, x), both inside the image
__device__ __forceinline__ int ycc(const uint8_t* __restrict__ img, int w, int c, int y, int x) {
    const uint8_t* p = img + ((int64_t)y * w + x) * 3;
    const int r = p[0], g = p[1], b = p[2];
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// sample (y, x) of component c's plane over its own block grid: edge repeats and down-sampling as the header states them
__device__ __forceinline__ int sample(const uint8_t* __restrict__ img, int h, int w, int hs, int vs, int c, int y, int x) {
    if (c == 0 || hs == 1) return ycc(img, w, c, min(y, h - 1), min(x, w - 1));
    const int xa = min(2 * x, w - 1), xb = min(2 * x + 1, w - 1);
    if (vs == 1) {
        const int yy = min(y, h - 1);
        return (ycc(img, w, c, yy, xa) + ycc(img, w, c, yy, xb) + (x & 1)) >> 1;
    }
    const int yd = min(y, ((h + 1) >> 1) - 1);                                   // the last down-sampled row is what repeats
    const int ya = min(2 * yd, h - 1), yb = min(2 * yd + 1, h - 1);
    return (ycc(img, w, c, ya, xa) + ycc(img, w, c, ya, xb) + ycc(img, w, c, yb, xa) + ycc(img, w, c, yb, xb) + 1 + (x & 1)) >> 2;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's accurate integer forward DCT on (v0..v7), in place.  kFirst: the row pass (even terms << 2, the others rounded >> 11);
// else the column pass (>> 2 and >> 15).  Samples are -128..127, so every intermediate fits int32.
template <bool kFirst>
__device__ __forceinline__ void fdct8(int* v) {
    constexpr int n = kFirst ? 11 : 15;
    const int t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
    const int t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    v[0] = kFirst ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    v[4] = kFirst ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    v[2] = descale(z1 + t13 * 6270, n);
    v[6] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    v[7] = descale(a4 + z1 + z3, n);
    v[5] = descale(a5 + z2 + z4, n);
    v[3] = descale(a6 + z2 + z3, n);
    v[1] = descale(a7 + z1 + z4, n);
}

struct fdct_lds {
    int v[kJobBlocks * kBlkDw];   // first: the rows are moved as 16-byte words
    job_lds J;
};

// grid: capped
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const uint8_t* __restrict__ src, const mny_image_desc* __restrict__ desc,
                                                        const mny_jpeg_item* __restrict__ items, int n, int max_h, int max_w, int16_t* __restrict__ coef,
                                                        int* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) fdct_lds S;
    const int tid = threadIdx.x;
    const uint32_t total = build_jobs(S.J, n, [&](int i) {
        return enc_sound(items + i, desc[i], max_h, max_w) ? (uint32_t)((items[i].n_coef / 64 + kJobBlocks - 1) / kJobBlocks) : 0u;
    });
    if (blockIdx.x == 0) {                                                       // the status word: the lowest item that is not sound
        const int per = (n + 255) / 256;
        const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
        uint32_t bad = 0xffffffffu;
        for (int i = i1 - 1; i >= i0; --i)
            if (!enc_sound(items + i, desc[i], max_h, max_w)) bad = (uint32_t)i;
        S.J.part[tid] = bad;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) S.J.part[tid] = min(S.J.part[tid], S.J.part[tid + s]);
            __syncthreads();
        }
        if (tid == 0) *ws = S.J.part[0] == 0xffffffffu ? 0 : (int)S.J.part[0] + 1;
        __syncthreads();
    }
    const int b = tid >> 3, r = tid & 7;
    int* blk = S.v + b * kBlkDw;
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        const int img = find_item(S.J, n, job);
        const mny_jpeg_item* it = items + img;
        const int h = it->h, w = it->w, hs = it->hs, vs = it->vs;
        const int64_t g = (int64_t)(job - S.J.pref[img]) * kJobBlocks + b;      // this lane's block of the image's padded grids
        const int c = g * 64 >= it->plane_off[2] ? 2 : (g * 64 >= it->plane_off[1] ? 1 : 0);
        const int64_t local = g - it->plane_off[c] / 64;
        const int bw = it->bw[c];
        const int by = (int)(local / bw), bx = (int)(local - (int64_t)by * bw);
        const int cw = c == 0 ? w : (w + hs - 1) / hs, ch = c == 0 ? h : (h + vs - 1) / vs;
        const bool live = g * 64 < it->n_coef && bx < (cw + 7) / 8 && by < (ch + 7) / 8;   // a block of the component's own grid
        int v[8];
        if (live) {                                                              // rows: lane r owns row r
            const uint8_t* pix = src + desc[img].offset;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = sample(pix, h, w, hs, vs, c, by * 8 + r, bx * 8 + k) - 128;
            fdct8<true>(v);
            *(int4*)(blk + r * 8) = make_int4(v[0], v[1], v[2], v[3]);
            *(int4*)(blk + r * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (live) {                                                              // columns, then quantise: lane r owns column r
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = blk[k * 8 + r];
            fdct8<false>(v);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t d = 8u * it->q[c][k * 8 + r];
                const uint32_t m = ((uint32_t)abs(v[k]) + (d >> 1)) / d;
                blk[k * 8 + r] = v[k] < 0 ? -(int)m : (int)m;
            }
        }
        __syncthreads();
        if (live) {
            const int4 lo = *(const int4*)(blk + r * 8), hi = *(const int4*)(blk + r * 8 + 4);
            short8 o;
            o[0] = (short)lo.x; o[1] = (short)lo.y; o[2] = (short)lo.z; o[3] = (short)lo.w;
            o[4] = (short)hi.x; o[5] = (short)hi.y; o[6] = (short)hi.z; o[7] = (short)hi.w;
            *(short8*)(coef + it->coef_off + g * 64 + r * 8) = o;
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" int mny_jpeg_enc_layout(const mny_image_desc* desc, int n, int quality, int hs, int vs, mny_jpeg_item* items, int64_t* coef_elems) {
    MNY_REQUIRE(desc && items && coef_elems, "mny_jpeg_enc_layout: null pointer");
    MNY_REQUIRE(n >= 1 && n <= kMaxItems, "mny_jpeg_enc_layout: bad batch size %d (1..%d)", n, kMaxItems);
    MNY_REQUIRE(quality >= 1 && quality <= 100, "mny_jpeg_enc_layout: quality %d outside 1..100", quality);
    MNY_REQUIRE((hs == 1 || hs == 2) && vs >= 1 && vs <= hs, "mny_jpeg_enc_layout: sampling %dx%d is not 1x1, 2x1 or 2x2", hs, vs);
    *coef_elems = mny_jpegenc_host::enc_layout(desc, n, quality, hs, vs, items);
    return MNY_OK;
}

extern "C" size_t mny_jpeg_enc_ws_bytes(int n) { return n >= 1 && n <= kMaxItems ? kWsBytes : 0; }

extern "C" int mny_jpeg_coef_batch(const uint8_t* src, const mny_image_desc* desc, const mny_jpeg_item* items, int n, int max_h, int max_w,
                                   int16_t* coef, void* ws, void* stream) {
    MNY_REQUIRE(src && desc && items && coef && ws, "mny_jpeg_coef_batch: null pointer");
    MNY_REQUIRE((((uintptr_t)src | (uintptr_t)coef | (uintptr_t)ws | (uintptr_t)items) & 15) == 0, "mny_jpeg_coef_batch: src, items, coef and ws must be 16-byte aligned");
    MNY_REQUIRE(n >= 1 && n <= kMaxItems && max_h >= 1 && max_w >= 1 && max_h <= kMaxSide && max_w <= kMaxSide,
                "mny_jpeg_coef_batch: bad sizes items=%d (1..%d) max %dx%d (sides up to %d)", n, kMaxItems, max_h, max_w, kMaxSide);
    const int64_t blocks = 3 * 4 * cdiv(max_h, 16) * cdiv(max_w, 16);            // 4:4:4 on the padded grid bounds every mode
    const int64_t bound = (int64_t)n * cdiv(blocks, kJobBlocks);
    jpeg_fdct_kernel<<<(unsigned)(bound < 2048 ? bound : 2048), 256, 0, (hipStream_t)stream>>>(src, desc, items, n, max_h, max_w, coef, (int*)ws);
    return check_launch("mny_jpeg_coef_batch");
}

extern "C" int mny_jpeg_huffman_batch(const int16_t* coef, int64_t coef_elems, const mny_jpeg_item* items, int n, uint8_t* out, const int64_t* out_off,
                                      const int64_t* out_cap, int64_t* out_len, int32_t* status, int n_threads) {
    MNY_REQUIRE(coef && items && out && out_off && out_cap && out_len && status, "mny_jpeg_huffman_batch: null pointer");
    MNY_REQUIRE(n >= 1 && n <= kMaxItems && coef_elems >= 0, "mny_jpeg_huffman_batch: bad batch size %d (1..%d) or negative coef_elems", n, kMaxItems);
    mny_jpegenc_host::batch(coef, coef_elems, items, n, out, out_off, out_cap, out_len, status, n_threads);
    return MNY_OK;
}
