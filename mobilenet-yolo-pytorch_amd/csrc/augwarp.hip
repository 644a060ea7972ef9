// YOLOv5-style random perspective on the device (include/mnyolo.h: mny_aug_warp_batch): one inverse projective map per image,
// output pixel -> source coordinate, Pillow's Image.transform(PERSPECTIVE) restated uint8 -> uint8 on the packed batch; RGB images
// are sampled BILINEAR (bilinear_filter32RGB), one-channel id maps NEAREST (nearest_filter8).  The host made every draw and
// inverted every matrix.
// An image is a flat string of h*w pixels from a 4-byte-aligned offset.  A lane owns four consecutive pixels of that order (a
// quad): 12 bytes = three aligned dwords for RGB, one dword for an id map, whatever 3*w is; the image's last 1..3 pixels go out in
// byte stores.  A 256-thread workgroup takes one (image, chunk of 1024 pixels) job at a time.  The job list is the prefix sum of
// the per-image chunk counts, which every workgroup rebuilds in LDS from the descriptors (as aug_seq_kernel does); the grid is
// capped and walks the list with a grid stride, so there is no launch per image.  A chunk is about two rows of a VOC image: at
// the default draws (scale and translation only) rows map to rows and the wave's taps stream; under rotation the footprint is a
// thin slanted strip and reuse between neighbouring chunks is left to L2.
// The coordinate arithmetic and the interpolation are fp64 without contraction (-ffp-contract=off): an fp64 a / b compiles to
// v_div_scale / v_div_fmas / v_div_fixup, the correctly rounded quotient, so the bytes are Pillow's.  An item with c6 == c7 == 0
// skips the division (den is exactly 1); the branch is per item, uniform over the workgroup.  Within a path the samplers do not
// branch, so that the 48 byte loads of a lane's four pixels overlap (measured 1.4 x against early returns).  The three channels
// of a tap share one address.  No atomics, no LDS beyond the job list, no scratch.
#include "common.h"

static_assert(sizeof(mny_aug_warp_item) == 72, "mny_aug_warp_item layout (augment.py WARP)");
static_assert(sizeof(mny_image_desc) == 16, "mny_image_desc layout");

namespace mny {
namespace {

constexpr int kMaxItems = 4096;
constexpr int kMaxSide = 16383;                                // pixels per image < 2^28, chunks per batch < 2^30
constexpr int kChunkPx = 1024;                                 // 256 lanes x 4 pixels
constexpr size_t kWsBytes = 256;                               // the status word

enum { kOk = 0, kZero = 1, kSkip = 2 };

__device__ __forceinline__ bool finite_d(double x) { return ((uint32_t)__double2hiint(x) & 0x7ff00000u) != 0x7ff00000u; }

__device__ __forceinline__ bool addressable(const mny_image_desc& d) {
    return d.offset >= 0 && d.h >= 1 && d.w >= 1 && d.h <= kMaxSide && d.w <= kMaxSide;
}

__device__ __forceinline__ uint32_t chunks_of(const mny_image_desc& d) { return (uint32_t)((d.h * d.w + kChunkPx - 1) / kChunkPx); }

// kOk: warp or copy; kZero: a malformed item whose bytes can be addressed, written as zeros; kSkip: no bytes to address
__device__ int classify(const mny_image_desc& d, const mny_aug_warp_item& q, int max_h, int max_w) {
    if (!addressable(d)) return kSkip;
    if ((d.offset & 3) || d.h > max_h || d.w > max_w) return kZero;
    for (int k = 0; k < 8; ++k)
        if (!finite_d(q.c[k])) return kZero;
    return kOk;
}

struct coef {
    double c0, c1, c2, c3, c4, c5, c6, c7;
};

// output pixel (x, y) -> source coordinate; false = the fill (den <= 0 or a non-finite coordinate: Pillow defines neither)
template <bool kAffine>
__device__ __forceinline__ bool source_of(const coef& c, int x, int y, double& xin, double& yin) {
    const double xi = (double)x + 0.5, yi = (double)y + 0.5;
    xin = c.c0 * xi + c.c1 * yi + c.c2;
    yin = c.c3 * xi + c.c4 * yi + c.c5;
    if (!kAffine) {
        const double den = c.c6 * xi + c.c7 * yi + 1.0;
        if (!(den > 0.0)) return false;
        xin = xin / den;
        yin = yin / den;
    }
    return finite_d(xin) && finite_d(yin);
}

// bilinear_filter32RGB: three bytes of one output pixel into o[0..3)
template <bool kAffine>
__device__ __forceinline__ void sample_rgb(const uint8_t* __restrict__ in, const coef& c, int h, int w, int x, int y, uint32_t fill, uint32_t* o) {
    double xin, yin;
    bool ok = source_of<kAffine>(c, x, y, xin, yin);
    ok = ok && !(xin < 0.0 || xin >= (double)w || yin < 0.0 || yin >= (double)h);
    // no branch from here on, so that the taps of a lane's four pixels can be in flight together: a pixel that takes the fill
    // reads pixel (0, 0) and drops the result
    const double xs = ok ? xin - 0.5 : 0.0, ys = ok ? yin - 0.5 : 0.0;
    const double fx = floor(xs), fy = floor(ys);
    const int X = (int)fx, Y = (int)fy;                          // -1 .. side - 1
    const double dx = xs - fx, dy = ys - fy;
    const int x0 = max(X, 0), x1 = min(X + 1, w - 1), y0 = max(Y, 0);
    const int y1 = Y + 1 < h ? Y + 1 : y0;                       // Y + 1 >= 0 always; past the last row v2 repeats v1's operations: v2 = v1
    const uint8_t* r0 = in + (int64_t)y0 * w * 3;
    const uint8_t* r1 = in + (int64_t)y1 * w * 3;
    const uint8_t *p00 = r0 + 3 * x0, *p01 = r0 + 3 * x1, *p10 = r1 + 3 * x0, *p11 = r1 + 3 * x1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double a = (double)p00[ch], b = (double)p01[ch], e = (double)p10[ch], f = (double)p11[ch];
        const double v1 = a + (b - a) * dx;
        const double v2 = e + (f - e) * dx;
        const uint32_t v = (uint32_t)(int)(v1 + (v2 - v1) * dy);  // (UINT8)v: 0 <= v <= 255, truncated
        o[ch] = ok ? v : (fill >> (8 * ch)) & 255u;
    }
}

// nearest_filter8
template <bool kAffine>
__device__ __forceinline__ uint32_t sample_id(const uint8_t* __restrict__ in, const coef& c, int h, int w, int x, int y, uint32_t fill) {
    double xin, yin;
    bool ok = source_of<kAffine>(c, x, y, xin, yin);
    ok = ok && !(xin < 0.0 || yin < 0.0 || xin >= (double)w || yin >= (double)h);
    const uint32_t v = in[ok ? (int64_t)(int)yin * w + (int)xin : 0];
    return ok ? v : fill;
}

// one chunk of one image: pixels [p0, min(p0 + 1024, h*w)) of the flat order
template <int kCh, bool kAffine>
__device__ void warp_chunk(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const mny_aug_warp_item& q, int h, int w, int p0) {
    const coef c = {q.c[0], q.c[1], q.c[2], q.c[3], q.c[4], q.c[5], q.c[6], q.c[7]};
    const int npx = h * w;
    const int p = p0 + 4 * threadIdx.x;
    if (p >= npx) return;
    const int n = min(4, npx - p);
    int y = p / w, x = p - y * w;
    if (kCh == 3) {
        const uint32_t fill = (uint32_t)q.fill[0] | ((uint32_t)q.fill[1] << 8) | ((uint32_t)q.fill[2] << 16);
        uint32_t b[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sample_rgb<kAffine>(in, c, h, w, x, y, fill, b + 3 * k);      // past the image's last pixel (k >= n): computed, not stored
            if (++x == w) { x = 0; ++y; }
        }
        uint8_t* o = out + (int64_t)p * 3;                        // 12 * (p / 4) from a 4-aligned base
        if (n == 4) {
#pragma unroll
            for (int d = 0; d < 3; ++d) ((uint32_t*)o)[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (k < 3 * n) o[k] = (uint8_t)b[k];
        }
    } else {
        const uint32_t fill = q.fill[0];
        uint32_t b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = sample_id<kAffine>(in, c, h, w, x, y, fill);
            if (++x == w) { x = 0; ++y; }
        }
        uint8_t* o = out + p;
        if (n == 4) {
            *(uint32_t*)o = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < n) o[k] = (uint8_t)b[k];
        }
    }
}

// an identity item: its bytes [b0, b0 + nb) of the chunk, whole dwords, then the image's last 1..3 bytes
__device__ void copy_chunk(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t nbytes, int64_t b0, int64_t nb) {
    const int64_t e = min(b0 + nb, nbytes);                       // b0 and nb are multiples of 4
    for (int64_t i = b0 + 4 * threadIdx.x; i + 4 <= e; i += 1024) *(uint32_t*)(out + i) = *(const uint32_t*)(in + i);
    if (e == nbytes) {
        const int64_t tail = (nbytes & ~(int64_t)3) + threadIdx.x;
        if (tail < nbytes) out[tail] = in[tail];
    }
}

// a malformed item: byte stores, the offset may be odd
__device__ void zero_chunk(uint8_t* __restrict__ out, int64_t nbytes, int64_t b0, int64_t nb) {
    const int64_t e = min(b0 + nb, nbytes);
    for (int64_t i = b0 + threadIdx.x; i < e; i += 256) out[i] = 0;
}

struct warp_lds {
    uint32_t pref[kMaxItems + 1];
    uint32_t part[256];
};

template <int kCh>
__global__ __launch_bounds__(256) void aug_warp_kernel(const uint8_t* __restrict__ src, const mny_image_desc* __restrict__ desc,
                                                       const mny_aug_warp_item* __restrict__ warp, int n_items, int max_h, int max_w,
                                                       uint8_t* __restrict__ dst, int* __restrict__ status) {
    __shared__ warp_lds S;
    const int tid = threadIdx.x;
    // ---- the job list: exclusive prefix sum of the per-image chunk counts
    const int per = (n_items + 255) / 256;
    const int i0 = min(tid * per, n_items), i1 = min(i0 + per, n_items);
    uint32_t local = 0;
    for (int i = i0; i < i1; ++i) {
        const mny_image_desc d = desc[i];
        const uint32_t c = addressable(d) ? chunks_of(d) : 0u;
        S.pref[i] = c;
        local += c;
    }
    S.part[tid] = local;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                                          // inclusive scan of the 256 partial sums
        const uint32_t add = tid >= s ? S.part[tid - s] : 0u;
        __syncthreads();
        S.part[tid] += add;
        __syncthreads();
    }
    uint32_t run = S.part[tid] - local;
    for (int i = i0; i < i1; ++i) {
        const uint32_t c = S.pref[i];
        S.pref[i] = run;
        run += c;
    }
    const uint32_t total = S.part[255];
    if (tid == 0) S.pref[n_items] = total;
    __syncthreads();
    // ---- status word: the lowest malformed index, by block 0 alone
    if (blockIdx.x == 0) {
        uint32_t bad = 0xffffffffu;
        for (int i = i1 - 1; i >= i0; --i)
            if (classify(desc[i], warp[i], max_h, max_w) != kOk) bad = (uint32_t)i;
        S.part[tid] = bad;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) S.part[tid] = min(S.part[tid], S.part[tid + s]);
            __syncthreads();
        }
        if (tid == 0) *status = S.part[0] == 0xffffffffu ? 0 : (int)S.part[0] + 1;
    }
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        int lo = 0, hi = n_items;                                                // the last image with pref <= job
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (S.pref[mid] <= job) lo = mid; else hi = mid;
        }
        const mny_image_desc d = desc[lo];
        const mny_aug_warp_item& q = warp[lo];
        const int p0 = (int)(job - S.pref[lo]) * kChunkPx;
        const int cls = classify(d, q, max_h, max_w);
        if (cls == kSkip) continue;
        const int64_t nbytes = (int64_t)kCh * d.h * d.w;
        if (cls == kZero)
            zero_chunk(dst + d.offset, nbytes, (int64_t)kCh * p0, (int64_t)kCh * kChunkPx);
        else if (q.identity)
            copy_chunk(src + d.offset, dst + d.offset, nbytes, (int64_t)kCh * p0, (int64_t)kCh * kChunkPx);
        else if (q.c[6] == 0.0 && q.c[7] == 0.0)
            warp_chunk<kCh, true>(src + d.offset, dst + d.offset, q, d.h, d.w, p0);
        else
            warp_chunk<kCh, false>(src + d.offset, dst + d.offset, q, d.h, d.w, p0);
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_aug_warp_ws_bytes(int n_items, int channels, int max_in_h, int max_in_w) {
    if (n_items < 1 || n_items > kMaxItems || (channels != 1 && channels != 3) || max_in_h < 1 || max_in_w < 1 || max_in_h > kMaxSide || max_in_w > kMaxSide)
        return 0;
    return kWsBytes;
}

extern "C" int mny_aug_warp_batch(const uint8_t* src, const mny_image_desc* desc, const mny_aug_warp_item* warp, int n_items, int channels, int max_in_h,
                                  int max_in_w, uint8_t* dst, void* ws, void* stream) {
    MNY_REQUIRE(src && desc && warp && dst && ws, "mny_aug_warp_batch: null pointer");
    MNY_REQUIRE(src != dst, "mny_aug_warp_batch: dst must not be src");
    MNY_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)ws) & 3) == 0, "mny_aug_warp_batch: src, dst and ws must be 4-byte aligned");
    MNY_REQUIRE((((uintptr_t)desc | (uintptr_t)warp) & 7) == 0, "mny_aug_warp_batch: desc and warp must be 8-byte aligned");
    MNY_REQUIRE(channels == 1 || channels == 3, "mny_aug_warp_batch: channels must be 3 (RGB, bilinear) or 1 (id map, nearest), got %d", channels);
    MNY_REQUIRE(n_items >= 1 && n_items <= kMaxItems && max_in_h >= 1 && max_in_w >= 1 && max_in_h <= kMaxSide && max_in_w <= kMaxSide,
                "mny_aug_warp_batch: bad sizes items=%d (1..%d) max %dx%d (sides up to %d)", n_items, kMaxItems, max_in_h, max_in_w, kMaxSide);
    hipStream_t st = (hipStream_t)stream;
    const int64_t bound = (int64_t)n_items * cdiv((int64_t)max_in_h * max_in_w, kChunkPx);
    const unsigned grid = (unsigned)(bound < 4096 ? bound : 4096);
    if (channels == 3)
        aug_warp_kernel<3><<<grid, 256, 0, st>>>(src, desc, warp, n_items, max_in_h, max_in_w, dst, (int*)ws);
    else
        aug_warp_kernel<1><<<grid, 256, 0, st>>>(src, desc, warp, n_items, max_in_h, max_in_w, dst, (int*)ws);
    return check_launch("mny_aug_warp_batch");
}
