// Annotation of image batches on the device (include/mnyolo.h: mny_viz_boxes, mny_viz_compose): draw records from detection or
// target rows, then one uint8 HWC image per item: source pixels, box outlines, seg overlay, in the reference's order
// (inference.py:70-103).  Built with -ffp-contract=off: the header states the arithmetic operation by operation and
// tests/viz_ref.py restates it in numpy.  No atomics, no host sync; every output byte has one writer.
//   viz_boxes_kernel   : one thread per row of a segment; record i belongs to row i, nothing is compacted.
//   viz_compose_kernel : one 256-thread workgroup owns a tile of kTileW x kTileH pixels of one item, a thread four pixels of
//                        one column (rows ty, ty + 4, ...), so a wave reads 64 consecutive floats of a plane.  The item's draw
//                        records are taken kList at a time: every thread tests one record against the TILE (its outline meets
//                        the tile), the survivors are appended in record order to a list in LDS by the wave scan of
//                        postproc.hip (shuffle scan + the four wave totals), and each pixel walks that list from its end, so
//                        the first hit is the latest record.  A pixel never meets a record whose outline misses its tile.
//                        The job list (item, tile) is csrc/jpeg_jobs.h; the grid is capped and strides over it.
#include "common.h"
#include "jpeg_jobs.h"

static_assert(sizeof(mny_viz_box) == 20, "mny_viz_box layout (viz.py BOX)");
static_assert(sizeof(mny_viz_item) == 32, "mny_viz_item layout (viz.py ITEM)");

namespace mny {
namespace {

using namespace jpeg_jobs;

constexpr int kTileW = 64, kTileH = 16;
constexpr int kList = 256;               // draw records per pass of the LDS list: one candidate per thread, so it cannot overflow
constexpr int kMaxSide = 16383;
constexpr int kMaxSeg = 8;               // seg classes
constexpr float kCorner = 1073741824.f;  // corners are clamped to +-2^30 before the conversion

// floor(v * size + 0.5) in fp32, one operation each; false for a NaN
__device__ __forceinline__ bool corner(float v, int size, int& out) {
    const float p = v * (float)size;
    const float f = floorf(p + 0.5f);
    if (!(f == f)) return false;
    out = (int)(f < -kCorner ? -kCorner : (f > kCorner ? kCorner : f));
    return true;
}

// grid: (S, trips).  mode 0: detection rows [.,7]; mode 1: target rows [.,5]
__global__ __launch_bounds__(256) void viz_boxes_kernel(const float* __restrict__ rows, int mode, const int32_t* __restrict__ seg_begin,
                                                        const int32_t* __restrict__ seg_count, int capacity, const mny_image_desc* __restrict__ dims,
                                                        float thr, const uint8_t* __restrict__ palette, int P, int thickness,
                                                        mny_viz_box* __restrict__ out) {
    const int s = blockIdx.x;
    const int begin = seg_begin[s];
    if (begin < 0 || begin >= capacity) return;
    const int count = min(max(seg_count[s], 0), capacity - begin);
    const int W = dims[s].w, H = dims[s].h;
    for (int r = blockIdx.y * 256 + threadIdx.x; r < count; r += gridDim.y * 256) {
        const int i = begin + r;
        mny_viz_box b = {0, 0, 0, 0, {0, 0, 0}, 0};
        float x1, y1, x2, y2, cls;
        bool draw;
        if (mode == 0) {
            const float* p = rows + (int64_t)i * 7;
            x1 = p[0]; y1 = p[1]; x2 = p[2]; y2 = p[3]; cls = p[6];
            draw = p[4] * p[5] > thr;
        } else {
            const float* p = rows + (int64_t)i * 5;
            const float hw = 0.5f * p[3], hh = 0.5f * p[4];
            cls = p[0];
            x1 = p[1] - hw; x2 = p[1] + hw; y1 = p[2] - hh; y2 = p[2] + hh;
            draw = true;
        }
        int xa, ya, xb, yb;
        draw = draw && W >= 1 && H >= 1 && cls >= 0.f && cls < 16777216.f;
        draw = draw && corner(x1, W, xa) && corner(y1, H, ya) && corner(x2, W, xb) && corner(y2, H, yb);
        if (draw) {
            const int c = (int)cls % P;
            b.x0 = min(xa, xb); b.x1 = max(xa, xb); b.y0 = min(ya, yb); b.y1 = max(ya, yb);
            b.rgb[0] = palette[3 * c]; b.rgb[1] = palette[3 * c + 1]; b.rgb[2] = palette[3 * c + 2];
            b.t = (uint8_t)thickness;
        }
        out[i] = b;
    }
}

struct compose_args {
    const float* batch;          // [N,3,H,W] or NULL
    int H, W;
    float mean[3], std[3];
    const uint8_t* src;          // packed uint8 HWC when batch == NULL
    const mny_image_desc* desc;
    const mny_viz_item* items;
    int N;
    const mny_viz_box* boxes;    // NULL: no boxes
    const int32_t* seg_begin;
    const int32_t* seg_count;
    int capacity;
    const float* seg;
    int C;
    int seg_channel[kMaxSeg];
    uint8_t* dst;
    int* ws;
};

__device__ bool item_sound(const compose_args& a, int i) {
    const mny_viz_item& it = a.items[i];
    if (it.h < 1 || it.w < 1 || it.h > kMaxSide || it.w > kMaxSide) return false;
    if (it.dst_offset < 0 || it.dst_stride < 3 * (int64_t)it.w) return false;
    if (a.C > 0 && it.seg_offset < 0) return false;
    if (a.batch) return it.h == a.H && it.w == a.W;
    return a.desc[i].offset >= 0 && a.desc[i].h == it.h && a.desc[i].w == it.w;
}

__device__ __forceinline__ uint32_t item_tiles(const compose_args& a, int i) {
    return item_sound(a, i) ? (uint32_t)(((a.items[i].w + kTileW - 1) / kTileW) * ((a.items[i].h + kTileH - 1) / kTileH)) : 0u;
}

// clamp(floor((x * std + mean) * 255 + 0.5), 0, 255), one fp32 operation each; a NaN gives 0
__device__ __forceinline__ int denorm(float x, float mean, float std) {
    const float v = floorf((x * std + mean) * 255.f + 0.5f);
    return v > 0.f ? (v < 255.f ? (int)v : 255) : 0;
}

struct compose_lds {
    job_lds J;
    mny_viz_box list[kList];
    int wsum[4];
};

// grid: capped
__global__ __launch_bounds__(256) void viz_compose_kernel(const compose_args a) {
    __shared__ compose_lds S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.N;
    const uint32_t total = build_jobs(S.J, n, [&](int i) { return item_tiles(a, i); });
    if (blockIdx.x == 0) {                                                       // the status word: the lowest item that is not sound
        const int per = (n + 255) / 256;
        const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
        uint32_t bad = 0xffffffffu;
        for (int i = i1 - 1; i >= i0; --i)
            if (!item_sound(a, i)) bad = (uint32_t)i;
        S.J.part[tid] = bad;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) S.J.part[tid] = min(S.J.part[tid], S.J.part[tid + s]);
            __syncthreads();
        }
        if (tid == 0) *a.ws = S.J.part[0] == 0xffffffffu ? 0 : (int)S.J.part[0] + 1;
        __syncthreads();
    }
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        const int img = find_item(S.J, n, job);
        const mny_viz_item it = a.items[img];
        const int h = it.h, w = it.w;
        const int tiles_x = (w + kTileW - 1) / kTileW;
        const int t = (int)(job - S.J.pref[img]);
        const int tx0 = (t % tiles_x) * kTileW, ty0 = (t / tiles_x) * kTileH;
        const int tx1 = min(tx0 + kTileW, w) - 1, ty1 = min(ty0 + kTileH, h) - 1; // the tile's last column and row
        const int x = tx0 + lane;
        const bool col = x < w;
        int px[4][3];
        // 1. source
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = ty0 + wave + 4 * k;
            px[k][0] = px[k][1] = px[k][2] = 0;
            if (col && y < h) {
                if (a.batch) {
                    const float* p = a.batch + ((int64_t)img * 3 * h + y) * w + x;
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[k][c] = denorm(p[(int64_t)c * h * w], a.mean[c], a.std[c]);
                } else {
                    const uint8_t* p = a.src + a.desc[img].offset + ((int64_t)y * w + x) * 3;
                    px[k][0] = p[0]; px[k][1] = p[1]; px[k][2] = p[2];
                }
            }
        }
        // 2. boxes: record order, later over earlier
        int begin = 0, count = 0;
        if (a.boxes) {
            begin = a.seg_begin[img];
            count = (begin < 0 || begin >= a.capacity) ? 0 : min(max(a.seg_count[img], 0), a.capacity - begin);
        }
        for (int r0 = 0; r0 < count; r0 += kList) {
            const int r = r0 + tid;
            mny_viz_box b = {0, 0, 0, 0, {0, 0, 0}, 0};
            int m = 0;
            if (r < count) {
                b = a.boxes[begin + r];
                const int th = b.t;
                const bool meets = th > 0 && b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= ty1 && b.y1 >= ty0;
                const bool inside = tx0 >= b.x0 + th && tx1 <= b.x1 - th && ty0 >= b.y0 + th && ty1 <= b.y1 - th;   // only interior pixels
                m = meets && !inside ? 1 : 0;
            }
            int inc = m;                                                         // inclusive scan over the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(inc, d);
                if (lane >= d) inc += up;
            }
            if (lane == 63) S.wsum[wave] = inc;
            __syncthreads();
            int woff = 0;
            for (int q = 0; q < wave; ++q) woff += S.wsum[q];
            const int listed = S.wsum[0] + S.wsum[1] + S.wsum[2] + S.wsum[3];
            if (m) S.list[woff + inc - 1] = b;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = ty0 + wave + 4 * k;
                for (int j = listed - 1; j >= 0; --j) {
                    const mny_viz_box& q = S.list[j];
                    const int th = q.t;
                    if (x >= q.x0 && x <= q.x1 && y >= q.y0 && y <= q.y1 && (x < q.x0 + th || x > q.x1 - th || y < q.y0 + th || y > q.y1 - th)) {
                        px[k][0] = q.rgb[0]; px[k][1] = q.rgb[1]; px[k][2] = q.rgb[2];
                        break;
                    }
                }
            }
            __syncthreads();                                                     // the list and wsum are rewritten by the next pass
        }
        // 3. seg overlay, class order; 4. store
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = ty0 + wave + 4 * k;
            if (!(col && y < h)) continue;
            for (int c = 0; c < a.C; ++c) {
                const float p = a.seg[it.seg_offset + ((int64_t)c * h + y) * w + x];
                if (p > 0.5f) {
                    const int ch = a.seg_channel[c];
                    const float v = (float)px[k][ch] * (1.0f - p);
                    px[k][ch] = v > 0.f ? (int)v : 0;                            // truncation; p above 1 gives 0
                }
            }
            uint8_t* o = a.dst + it.dst_offset + (int64_t)y * it.dst_stride + (int64_t)x * 3;
            o[0] = (uint8_t)px[k][0]; o[1] = (uint8_t)px[k][1]; o[2] = (uint8_t)px[k][2];
        }
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" int mny_viz_boxes(const float* rows, int mode, const int32_t* seg_begin, const int32_t* seg_count, int S, int capacity,
                             const mny_image_desc* dims, float thr, const uint8_t* palette, int P, int thickness, mny_viz_box* out, void* stream) {
    MNY_REQUIRE(S >= 0 && S <= kMaxItems, "mny_viz_boxes: bad segment count %d (0..%d)", S, kMaxItems);
    MNY_REQUIRE(mode == 0 || mode == 1, "mny_viz_boxes: mode %d is neither 0 (detections) nor 1 (targets)", mode);
    MNY_REQUIRE(P >= 1 && thickness >= 1 && thickness <= 8, "mny_viz_boxes: palette of %d colours, thickness %d (1..8)", P, thickness);
    MNY_REQUIRE(capacity >= 0, "mny_viz_boxes: negative capacity");
    if (S == 0 || capacity == 0) return MNY_OK;
    MNY_REQUIRE(rows && seg_begin && seg_count && dims && palette && out, "mny_viz_boxes: null pointer");
    const int64_t need = cdiv(capacity, 256);
    const int trips = (int)(need < 32 ? need : 32);
    viz_boxes_kernel<<<dim3(S, trips), 256, 0, (hipStream_t)stream>>>(rows, mode, seg_begin, seg_count, capacity, dims, thr, palette, P, thickness, out);
    return check_launch("mny_viz_boxes");
}

extern "C" size_t mny_viz_ws_bytes(int N) { return N >= 1 && N <= kMaxItems ? 256 : 0; }

extern "C" int mny_viz_compose(const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                               const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes,
                               const int32_t* seg_begin, const int32_t* seg_count, int capacity, const float* seg, int C,
                               const int32_t* seg_channel, uint8_t* dst, void* ws, void* stream) {
    MNY_REQUIRE(items && dst && ws, "mny_viz_compose: null pointer");
    MNY_REQUIRE(N >= 1 && N <= kMaxItems, "mny_viz_compose: bad batch size %d (1..%d)", N, kMaxItems);
    MNY_REQUIRE((batch != nullptr) != (src != nullptr), "mny_viz_compose: exactly one of batch and src");
    int max_h = kMaxSide, max_w = kMaxSide;
    compose_args a{};
    if (batch) {
        MNY_REQUIRE(mean3 && std3, "mny_viz_compose: null pointer (mean3, std3)");
        MNY_REQUIRE(H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide, "mny_viz_compose: bad batch size %dx%d (sides 1..%d)", H, W, kMaxSide);
        for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.std[c] = std3[c]; }
        max_h = H;
        max_w = W;
    } else {
        MNY_REQUIRE(desc, "mny_viz_compose: null pointer (desc)");
    }
    MNY_REQUIRE(!boxes || (seg_begin && seg_count && capacity >= 0), "mny_viz_compose: boxes without their segments");
    MNY_REQUIRE(C >= 0 && C <= kMaxSeg && (C == 0 || (seg && seg_channel)), "mny_viz_compose: %d seg classes (0..%d) or null planes", C, kMaxSeg);
    for (int c = 0; c < C; ++c) {
        MNY_REQUIRE(seg_channel[c] >= 0 && seg_channel[c] <= 2, "mny_viz_compose: seg_channel[%d] = %d is no RGB channel", c, seg_channel[c]);
        a.seg_channel[c] = seg_channel[c];
    }
    a.batch = batch; a.H = H; a.W = W; a.src = src; a.desc = desc; a.items = items; a.N = N;
    a.boxes = boxes; a.seg_begin = seg_begin; a.seg_count = seg_count; a.capacity = capacity;
    a.seg = seg; a.C = C; a.dst = dst; a.ws = (int*)ws;
    const int64_t bound = (int64_t)N * cdiv(max_w, kTileW) * cdiv(max_h, kTileH);
    viz_compose_kernel<<<(unsigned)(bound < 4096 ? bound : 4096), 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("mny_viz_compose");
}
