// Baseline JPEG decode (include/mnyolo.h: mny_jpeg_*).  The host half, marker parsing and Huffman decoding into quantised
// coefficients, is csrc/jpeg_host.h and is only exported here; this file is the device half, everything per pixel, as two
// launches over the whole batch:
//   (a) jpeg_idct_kernel  : one 256-thread workgroup takes 32 consecutive 8x8 blocks of one image, eight lanes per block.
//                           Lane r loads row r of the block (8 int16 = one 16-byte load; the 32 blocks are 4 KiB contiguous),
//                           dequantises it and parks it in LDS; lane c then transforms column c in place, lane r transforms
//                           row r and stores its 8 samples as one 8-byte word into the uint8 plane in ws.  A block is 72 dwords
//                           apart from the next in LDS, so the four blocks of a 32-lane group read their columns from 32
//                           different banks.
//   (b) jpeg_rgb_kernel   : one workgroup takes 1024 consecutive pixels of one image (rows are contiguous in the packed
//                           layout, so pixels are counted through the row ends), four per thread: chroma upsampling from
//                           the planes, YCbCr -> RGB, 12 bytes per thread into LDS, then 192 threads store the 3072 bytes
//                           as 16-byte words.  1024 pixels are 3072 bytes, so every job starts 16-byte aligned and only the
//                           last word of an image can be partial; that one goes out by bytes.
// Both kernels rebuild the job list (the prefix sum of the per-image job counts) in LDS from the item records, as
// augseq.hip does; the grid is capped and strides over it.  Integer arithmetic only; no atomics, no scratch.
#include "common.h"
#include "jpeg_host.h"
#include "jpeg_jobs.h"

static_assert(sizeof(mny_jpeg_item) == 512, "mny_jpeg_item layout (jpeg.py ITEM)");
static_assert(sizeof(mny_jpeg_info) == 56, "mny_jpeg_info layout (jpeg.py INFO)");
static_assert(offsetof(mny_jpeg_item, q) == 96, "the quantisation rows are read as 16-byte words");
static_assert(sizeof(mny_image_desc) == 16, "mny_image_desc layout");

namespace mny {
namespace {

using namespace jpeg_jobs;
constexpr int kMaxSide = 16383;
constexpr size_t kWsHead = 256;          // status word, then the uint8 planes at the coefficients' element offsets
constexpr int kJobBlocks = 32;           // 8x8 blocks per job of launch (a)
constexpr int kBlkDw = 72;               // LDS dwords from one block to the next: 64 + 8
constexpr int kJobPix = 1024;            // pixels per job of launch (b): 3072 bytes, a multiple of 16

typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

__device__ bool sound(const mny_jpeg_item* it, const mny_image_desc& d, int max_h, int max_w) {
    if (it->status != MNY_JPEG_OK) return false;
    const int nc = it->ncomp, h = it->h, w = it->w, hs = it->hs, vs = it->vs;
    if (nc != 1 && nc != 3) return false;
    if (h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return false;
    if (nc == 1 ? (hs != 1 || vs != 1) : !((hs == 1 || hs == 2) && vs >= 1 && vs <= hs)) return false;
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        const int bw = c < nc ? mcux * (c == 0 ? hs : 1) : 0, bh = c < nc ? mcuy * (c == 0 ? vs : 1) : 0;
        if (it->bw[c] != bw || it->bh[c] != bh || it->plane_off[c] != off) return false;
        off += (int64_t)bw * bh * 64;
    }
    if (it->n_coef != off) return false;
    if (it->coef_off < 0 || (it->coef_off & 7)) return false;
    if (d.offset < 0 || (d.offset & 15)) return false;
    if (d.h != h || d.w != w || h > max_h || w > max_w) return false;
    return true;
}

// The 1-D inverse DCT of the header, in place.  The sums run in uint32 so that coefficients no encoder writes wrap
// instead of overflowing; for a real stream every intermediate fits int32 and the result is the header's.
__device__ __forceinline__ void idct8(int* v) {
    typedef uint32_t u;
    const u v0 = (u)v[0], v1 = (u)v[1], v2 = (u)v[2], v3 = (u)v[3], v4 = (u)v[4], v5 = (u)v[5], v6 = (u)v[6], v7 = (u)v[7];
    u z1 = (v2 + v6) * 4433u;
    const u t2 = z1 - v6 * 15137u, t3 = z1 + v2 * 6270u;
    const u t0 = (v0 + v4) * 8192u, t1 = (v0 - v4) * 8192u;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u a0 = v7, a1 = v5, a2 = v3, a3 = v1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5;
    z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    v[0] = (int)(t10 + a3); v[7] = (int)(t10 - a3);
    v[1] = (int)(t11 + a2); v[6] = (int)(t11 - a2);
    v[2] = (int)(t12 + a1); v[5] = (int)(t12 - a1);
    v[3] = (int)(t13 + a0); v[4] = (int)(t13 - a0);
}
__device__ __forceinline__ int round_shift(int x, int add, int sh) { return (int)((uint32_t)x + (uint32_t)add) >> sh; }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

struct idct_lds {
    int v[kJobBlocks * kBlkDw];   // first: the rows are moved as 16-byte words
    job_lds J;
};

// launch (a).  grid: capped
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const mny_jpeg_item* __restrict__ items,
                                                        const mny_image_desc* __restrict__ desc, int n, int max_h, int max_w, uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) idct_lds S;
    const int tid = threadIdx.x;
    const uint32_t total = build_jobs(S.J, n, [&](int i) {
        return sound(items + i, desc[i], max_h, max_w) ? (uint32_t)((items[i].n_coef / 64 + kJobBlocks - 1) / kJobBlocks) : 0u;
    });
    if (blockIdx.x == 0) {                                                       // the status word: the lowest item that is not sound
        const int per = (n + 255) / 256;
        const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
        uint32_t bad = 0xffffffffu;
        for (int i = i1 - 1; i >= i0; --i)
            if (!sound(items + i, desc[i], max_h, max_w)) bad = (uint32_t)i;
        S.J.part[tid] = bad;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) S.J.part[tid] = min(S.J.part[tid], S.J.part[tid + s]);
            __syncthreads();
        }
        if (tid == 0) *(int*)ws = S.J.part[0] == 0xffffffffu ? 0 : (int)S.J.part[0] + 1;
        __syncthreads();
    }
    const int b = tid >> 3, r = tid & 7;
    int* blk = S.v + b * kBlkDw;
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        const int img = find_item(S.J, n, job);
        const mny_jpeg_item* it = items + img;
        const int64_t g = (int64_t)(job - S.J.pref[img]) * kJobBlocks + b;      // this lane's block of the image
        const bool live = g * 64 < it->n_coef;
        int c = 0;
        if (it->ncomp == 3) c = g * 64 >= it->plane_off[2] ? 2 : (g * 64 >= it->plane_off[1] ? 1 : 0);
        int v[8];
        if (live) {
            const short8 cf = *(const short8*)(coef + it->coef_off + g * 64 + r * 8);
            const ushort8 q = *(const ushort8*)(&it->q[c][r * 8]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (int)cf[k] * (int)q[k];
            *(int4*)(blk + r * 8) = make_int4(v[0], v[1], v[2], v[3]);
            *(int4*)(blk + r * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (live) {                                                              // columns: lane r owns column r
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = blk[k * 8 + r];
            idct8(v);
#pragma unroll
            for (int k = 0; k < 8; ++k) blk[k * 8 + r] = round_shift(v[k], 1024, 11);
        }
        __syncthreads();
        if (live) {                                                              // rows
            const int4 lo = *(const int4*)(blk + r * 8), hi = *(const int4*)(blk + r * 8 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            idct8(v);
            uint32_t w0 = 0, w1 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w0 |= (uint32_t)clamp255(round_shift(v[k], 131072, 18) + 128) << (8 * k);
                w1 |= (uint32_t)clamp255(round_shift(v[k + 4], 131072, 18) + 128) << (8 * k);
            }
            const int64_t local = g - it->plane_off[c] / 64;
            const int bw = it->bw[c];
            const int64_t by = local / bw, bx = local - by * bw;
            uint8_t* plane = ws + kWsHead + it->coef_off + it->plane_off[c];
            *(uint2*)(plane + (by * 8 + r) * ((int64_t)bw * 8) + bx * 8) = make_uint2(w0, w1);
        }
        __syncthreads();
    }
}

// one chroma sample of output pixel (x, y): p = the plane, `stride` bytes per row, cw x ch real samples
__device__ __forceinline__ int chroma(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(int64_t)y * stride + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * stride + i];        // libjpeg replicates a plane this narrow
    const int in = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (vs == 1) {
        const uint8_t* row = p + (int64_t)y * stride;
        return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int j = y >> 1;
    const int jn = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const uint8_t* r0 = p + (int64_t)j * stride;
    const uint8_t* r1 = p + (int64_t)jn * stride;
    const int si = 3 * r0[i] + r1[i], sn = 3 * r0[in] + r1[in];
    return (3 * si + sn + ((x & 1) ? 7 : 8)) >> 4;
}

struct rgb_lds {
    uint32_t px[kJobPix * 3 / 4];   // first: read back as 16-byte words
    job_lds J;
};

// launch (b).  grid: capped
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const mny_jpeg_item* __restrict__ items, const mny_image_desc* __restrict__ desc, int n, int max_h,
                                                       int max_w, const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) rgb_lds S;
    const int tid = threadIdx.x;
    const uint32_t total = build_jobs(S.J, n, [&](int i) {
        return sound(items + i, desc[i], max_h, max_w) ? (uint32_t)(((int64_t)items[i].h * items[i].w + kJobPix - 1) / kJobPix) : 0u;
    });
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        const int img = find_item(S.J, n, job);
        const mny_jpeg_item* it = items + img;
        const int h = it->h, w = it->w, hs = it->hs, vs = it->vs;
        const bool colour = it->ncomp == 3;
        const int64_t npix = (int64_t)h * w;
        const int64_t p0 = (int64_t)(job - S.J.pref[img]) * kJobPix;
        const uint8_t* base = ws + kWsHead + it->coef_off;
        const uint8_t* Y = base;
        const uint8_t* Cb = base + it->plane_off[1];
        const uint8_t* Cr = base + it->plane_off[2];
        const int ys = it->bw[0] * 8, cs = it->bw[1] * 8;
        const int cw = hs == 2 ? (w + 1) >> 1 : w, ch = vs == 2 ? (h + 1) >> 1 : h;
        uint32_t o[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t p = p0 + 4 * tid + k;
            int rr = 0, gg = 0, bb = 0;
            if (p < npix) {
                const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
                const int lum = Y[(int64_t)y * ys + x];
                rr = gg = bb = lum;
                if (colour) {
                    const int cb = chroma(Cb, cs, cw, ch, hs, vs, x, y) - 128, cr = chroma(Cr, cs, cw, ch, hs, vs, x, y) - 128;
                    rr = clamp255(lum + ((91881 * cr + 32768) >> 16));
                    gg = clamp255(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    bb = clamp255(lum + ((116130 * cb + 32768) >> 16));
                }
            }
            const int vals[3] = {rr, gg, bb};
#pragma unroll
            for (int ch3 = 0; ch3 < 3; ++ch3) {
                const int byte = 3 * k + ch3;
                o[byte >> 2] |= (uint32_t)vals[ch3] << (8 * (byte & 3));
            }
        }
        S.px[3 * tid] = o[0]; S.px[3 * tid + 1] = o[1]; S.px[3 * tid + 2] = o[2];
        __syncthreads();
        if (tid < kJobPix * 3 / 16) {
            const int64_t B = p0 * 3 + 16 * tid, end = npix * 3;                 // bytes from the image's first
            uint8_t* out = dst + desc[img].offset + B;
            if (B + 16 <= end) {
                *(uint4*)out = *(const uint4*)(S.px + 4 * tid);
            } else {
                const uint8_t* sb = (const uint8_t*)(S.px + 4 * tid);
                for (int k = 0; k < 16; ++k)
                    if (B + k < end) out[k] = sb[k];
            }
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" int mny_jpeg_probe(const uint8_t* data, int64_t len, mny_jpeg_info* info) {
    MNY_REQUIRE(data && info && len >= 0, "mny_jpeg_probe: null pointer or negative length");
    mny_jpeg_host::probe(data, len, info);
    return MNY_OK;
}

extern "C" int mny_jpeg_entropy_batch(const uint8_t* const* data, const int64_t* len, int n, int16_t* coef, const int64_t* coef_off,
                                      const int64_t* coef_cap, mny_jpeg_item* items, int n_threads) {
    MNY_REQUIRE(data && len && coef && coef_off && coef_cap && items, "mny_jpeg_entropy_batch: null pointer");
    MNY_REQUIRE(n >= 1 && n <= kMaxItems, "mny_jpeg_entropy_batch: bad batch size %d (1..%d)", n, kMaxItems);
    mny_jpeg_host::batch(data, len, n, coef, coef_off, coef_cap, items, n_threads);
    return MNY_OK;
}

extern "C" size_t mny_jpeg_ws_bytes(int n, int64_t coef_elems) {
    if (n < 1 || n > kMaxItems || coef_elems < 1) return 0;
    return kWsHead + (((size_t)coef_elems + 255) & ~(size_t)255);
}

extern "C" int mny_jpeg_pixels_batch(const int16_t* coef, const mny_jpeg_item* items, int n, uint8_t* dst, const mny_image_desc* desc, int max_h,
                                     int max_w, void* ws, void* stream) {
    MNY_REQUIRE(coef && items && dst && desc && ws, "mny_jpeg_pixels_batch: null pointer");
    MNY_REQUIRE((((uintptr_t)coef | (uintptr_t)dst | (uintptr_t)ws | (uintptr_t)items) & 15) == 0, "mny_jpeg_pixels_batch: coef, items, dst and ws must be 16-byte aligned");
    MNY_REQUIRE(n >= 1 && n <= kMaxItems && max_h >= 1 && max_w >= 1 && max_h <= kMaxSide && max_w <= kMaxSide,
                "mny_jpeg_pixels_batch: bad sizes items=%d (1..%d) max %dx%d (sides up to %d)", n, kMaxItems, max_h, max_w, kMaxSide);
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = 3 * 4 * cdiv(max_h, 16) * cdiv(max_w, 16);            // 4:4:4 on the padded grid bounds every mode
    const int64_t bound_a = (int64_t)n * cdiv(blocks, kJobBlocks), bound_b = (int64_t)n * cdiv((int64_t)max_h * max_w, kJobPix);
    jpeg_idct_kernel<<<(unsigned)(bound_a < 2048 ? bound_a : 2048), 256, 0, st>>>(coef, items, desc, n, max_h, max_w, (uint8_t*)ws);
    jpeg_rgb_kernel<<<(unsigned)(bound_b < 2048 ? bound_b : 2048), 256, 0, st>>>(items, desc, n, max_h, max_w, (const uint8_t*)ws, dst);
    return check_launch("mny_jpeg_pixels_batch");
}
