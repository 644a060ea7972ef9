// Annotation of image batches on the device (include/mnyolo.h: mny_viz_boxes, mny_viz_labels, mny_viz_compose,
// mny_viz_compose_labels): draw and label records from detection or target rows, then one uint8 HWC image per item: source
// pixels, box outlines with their class-name labels, seg overlay, in the reference's order (inference.py:70-103).  Built with
// -ffp-contract=off: the header states the arithmetic operation by operation and tests/viz_ref.py, tests/vizlabel_ref.py restate
// it in numpy.  No atomics, no host sync; every output byte has one writer.
//   viz_boxes_kernel   : one thread per row of a segment; record i belongs to row i, nothing is compacted.
//   viz_labels_kernel  : one thread per row again; label record i sits beside box record i and is empty where that one is.
//   viz_compose_kernel : one 256-thread workgroup owns a tile of kTileW x kTileH pixels of one item, a thread four pixels of
//                        one column (rows ty, ty + 4, ...), so a wave reads 64 consecutive floats of a plane.  The item's draw
//                        records are taken kList at a time: every thread tests one record against the TILE (its outline meets
//                        the tile), the survivors are appended in record order to a list in LDS by the wave scan of
//                        postproc.hip (shuffle scan + the four wave totals), and each pixel walks that list from its end, so
//                        the first hit is the latest record.  A pixel never meets a record whose outline misses its tile.
//                        The job list (item, tile) is csrc/jpeg_jobs.h; the grid is capped and strides over it.
//                        The instantiation with labels lists a record when its outline OR its label rectangle meets the tile and
//                        walks the list forwards, outline then label per record: a label that is not filled, or whose coverage
//                        is partial, blends with what the earlier records left.  The instantiation without them is the kernel
//                        as it was.
#include "common.h"
#include "jpeg_jobs.h"

static_assert(sizeof(mny_viz_box) == 20, "mny_viz_box layout (viz.py BOX)");
static_assert(sizeof(mny_viz_item) == 32, "mny_viz_item layout (viz.py ITEM)");
static_assert(sizeof(mny_viz_label) == 48 && alignof(mny_viz_label) == 4, "mny_viz_label layout (viz.py LABEL)");
static_assert(MNY_VIZ_LABEL_STRIPS == 8 + 5, "a class index of 8 digits, then space, digit, point, two digits");

namespace mny {
namespace {

using namespace jpeg_jobs;

constexpr int kTileW = 64, kTileH = 16;
constexpr int kList = 256;               // draw records per pass of the LDS list: one candidate per thread, so it cannot overflow
constexpr int kMaxSide = 16383;
constexpr int kMaxSeg = 8;               // seg classes
constexpr float kCorner = 1073741824.f;  // corners are clamped to +-2^30 before the conversion
constexpr int kPad = 2;                  // columns of background left and right of a label's text
constexpr int kDot = 10, kSpace = 11;    // the strips after the names: "0123456789. "

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

// grid: (S, trips), as viz_boxes_kernel.  strips: (offset, w) per strip, the names first, then "0123456789. "
__global__ __launch_bounds__(256) void viz_labels_kernel(const float* __restrict__ rows, int mode, const int32_t* __restrict__ seg_begin,
                                                         const int32_t* __restrict__ seg_count, int capacity, const mny_image_desc* __restrict__ dims,
                                                         const mny_viz_box* __restrict__ boxes, const int32_t* __restrict__ strips, int n_names, int h,
                                                         int with_score, int filled, int label_targets, uint32_t fg, mny_viz_label* __restrict__ out) {
    const int s = blockIdx.x;
    const int begin = seg_begin[s];
    if (begin < 0 || begin >= capacity) return;
    const int count = min(max(seg_count[s], 0), capacity - begin);
    const int W = dims[s].w;
    for (int r = blockIdx.y * 256 + threadIdx.x; r < count; r += gridDim.y * 256) {
        const int i = begin + r;
        mny_viz_label* o = out + i;
        *o = mny_viz_label{};
        const mny_viz_box b = boxes[i];
        if (b.t == 0 || (mode == 1 && !label_targets)) continue;                // the gate was decided by mny_viz_boxes
        const float* p = rows + (int64_t)i * (mode == 0 ? 7 : 5);
        const float cls = p[mode == 0 ? 6 : 0];
        if (!(cls >= 0.f && cls < 16777216.f)) continue;                        // no drawn record has such a class: these are not its rows
        const int c = (int)cls;
        int n = 0, tw = 0;
        auto append = [&](int strip) {
            o->seq[n++] = (uint16_t)strip;
            tw += strips[2 * strip + 1];
        };
        if (c < n_names) {
            append(c);
        } else {                                                                // the class index in decimal, at most 8 digits
            int div = 1;
            while (c / div >= 10) div *= 10;
            for (; div > 0; div /= 10) append(n_names + c / div % 10);
        }
        if (mode == 0 && with_score) {
            const float prod = p[4] * p[5];                                      // the product of the gate
            const double v = rint((double)prod * 100.0);
            const int k = v > 0.0 ? (v < 999.0 ? (int)v : 999) : 0;
            append(n_names + kSpace);
            append(n_names + k / 100);
            append(n_names + kDot);
            append(n_names + k / 10 % 10);
            append(n_names + k % 10);
        }
        const int lw = tw + 2 * kPad;
        o->lx = max(min(b.x0, W - lw), 0);
        o->ly = b.y0 - h >= 0 ? b.y0 - h : b.y0;
        o->lw = lw;
        o->n = (uint8_t)n;
        o->lh = (uint8_t)h;
        o->filled = (uint8_t)(filled ? 1 : 0);
        o->bg[0] = b.rgb[0]; o->bg[1] = b.rgb[1]; o->bg[2] = b.rgb[2];
        o->fg[0] = (uint8_t)fg; o->fg[1] = (uint8_t)(fg >> 8); o->fg[2] = (uint8_t)(fg >> 16);
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
    static constexpr bool kLabels = false;
};

struct compose_label_args : compose_args {
    const mny_viz_label* labels;  // beside boxes
    const uint8_t* atlas;
    const int32_t* strips;
    static constexpr bool kLabels = true;
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

template <bool L>
struct compose_lds {
    job_lds J;
    mny_viz_box list[kList];
    int wsum[4];
};
template <>
struct compose_lds<true> : compose_lds<false> {
    mny_viz_label labs[kList];
};

// coverage of a label at text column c, row `row`: through the strip sequence; 0 outside 0 .. tw - 1
__device__ __forceinline__ int coverage(const mny_viz_label& l, int c, int row, const int32_t* __restrict__ strips, const uint8_t* __restrict__ atlas) {
    if (c < 0) return 0;
    for (int s = 0; s < l.n; ++s) {
        const int32_t* e = strips + 2 * (int)l.seq[s];
        const int w = e[1];
        if (c < w) return atlas[(int64_t)e[0] + (int64_t)row * w + c];
        c -= w;
    }
    return 0;
}

// Pillow's blend of an 8-bit mask: m * ink + (255 - m) * under, divided by 255 with rounding
__device__ __forceinline__ int blend(int m, int under, int ink) {
    const int tmp = m * ink + (255 - m) * under + 128;
    return ((tmp >> 8) + tmp) >> 8;
}

// grid: capped.  A: compose_args (the kernel without labels) or compose_label_args
template <class A>
__global__ __launch_bounds__(256) void viz_compose_kernel(const A a) {
    constexpr bool L = A::kLabels;
    __shared__ compose_lds<L> S;
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
                if constexpr (L) {
                    const mny_viz_label& l = a.labels[begin + r];
                    if (l.n > 0 && l.lx <= tx1 && l.lx + l.lw > tx0 && l.ly <= ty1 && l.ly + (int)l.lh > ty0) m = 1;
                }
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
            if constexpr (L) {
                if (m) S.labs[woff + inc - 1] = a.labels[begin + r];
            }
            __syncthreads();
            if constexpr (L) {                                                   // forwards: a record's outline, then its label, which may blend
                for (int j = 0; j < listed; ++j) {
                    const mny_viz_box& q = S.list[j];
                    const mny_viz_label& l = S.labs[j];
                    const int th = q.t;
                    const bool xin = x >= q.x0 && x <= q.x1, xedge = x < q.x0 + th || x > q.x1 - th;
                    const bool lxin = l.n > 0 && x >= l.lx && x < l.lx + l.lw;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int y = ty0 + wave + 4 * k;
                        if (th > 0 && xin && y >= q.y0 && y <= q.y1 && (xedge || y < q.y0 + th || y > q.y1 - th)) {
                            px[k][0] = q.rgb[0]; px[k][1] = q.rgb[1]; px[k][2] = q.rgb[2];
                        }
                        if (lxin && y >= l.ly && y < l.ly + (int)l.lh) {
                            const int cov = coverage(l, x - l.lx - kPad, y - l.ly, a.strips, a.atlas);
#pragma unroll
                            for (int c = 0; c < 3; ++c) px[k][c] = blend(cov, l.filled ? (int)l.bg[c] : px[k][c], l.fg[c]);
                        }
                    }
                }
            } else {
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

extern "C" int mny_viz_labels(const float* rows, int mode, const int32_t* seg_begin, const int32_t* seg_count, int S, int capacity,
                              const mny_image_desc* dims, const mny_viz_box* boxes, const int32_t* strips, int n_names, int h, int with_score,
                              int filled, int label_targets, const uint8_t* text_rgb, mny_viz_label* out, void* stream) {
    MNY_REQUIRE(S >= 0 && S <= kMaxItems, "mny_viz_labels: bad segment count %d (0..%d)", S, kMaxItems);
    MNY_REQUIRE(mode == 0 || mode == 1, "mny_viz_labels: mode %d is neither 0 (detections) nor 1 (targets)", mode);
    MNY_REQUIRE(n_names >= 0 && n_names <= MNY_VIZ_MAX_NAMES, "mny_viz_labels: %d names (0..%d)", n_names, MNY_VIZ_MAX_NAMES);
    MNY_REQUIRE(h >= 1 && h <= MNY_VIZ_MAX_TEXT_H, "mny_viz_labels: a line height of %d (1..%d)", h, MNY_VIZ_MAX_TEXT_H);
    MNY_REQUIRE(capacity >= 0, "mny_viz_labels: negative capacity");
    if (S == 0 || capacity == 0) return MNY_OK;
    MNY_REQUIRE(rows && seg_begin && seg_count && dims && boxes && strips && text_rgb && out, "mny_viz_labels: null pointer");
    const int64_t need = cdiv(capacity, 256);
    const int trips = (int)(need < 32 ? need : 32);
    const uint32_t fg = (uint32_t)text_rgb[0] | (uint32_t)text_rgb[1] << 8 | (uint32_t)text_rgb[2] << 16;
    viz_labels_kernel<<<dim3(S, trips), 256, 0, (hipStream_t)stream>>>(rows, mode, seg_begin, seg_count, capacity, dims, boxes, strips, n_names, h,
                                                                       with_score, filled, label_targets, fg, out);
    return check_launch("mny_viz_labels");
}

extern "C" size_t mny_viz_ws_bytes(int N) { return N >= 1 && N <= kMaxItems ? 256 : 0; }

// both compose entry points; `who` names the caller in messages
static int compose(const char* who, const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                   const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes, const int32_t* seg_begin,
                   const int32_t* seg_count, int capacity, const float* seg, int C, const int32_t* seg_channel, uint8_t* dst, void* ws,
                   const mny_viz_label* labels, const uint8_t* atlas, const int32_t* strips, void* stream) {
    MNY_REQUIRE(items && dst && ws, "%s: null pointer", who);
    MNY_REQUIRE(N >= 1 && N <= kMaxItems, "%s: bad batch size %d (1..%d)", who, N, kMaxItems);
    MNY_REQUIRE((batch != nullptr) != (src != nullptr), "%s: exactly one of batch and src", who);
    int max_h = kMaxSide, max_w = kMaxSide;
    compose_label_args a{};
    if (batch) {
        MNY_REQUIRE(mean3 && std3, "%s: null pointer (mean3, std3)", who);
        MNY_REQUIRE(H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide, "%s: bad batch size %dx%d (sides 1..%d)", who, H, W, kMaxSide);
        for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.std[c] = std3[c]; }
        max_h = H;
        max_w = W;
    } else {
        MNY_REQUIRE(desc, "%s: null pointer (desc)", who);
    }
    MNY_REQUIRE(!boxes || (seg_begin && seg_count && capacity >= 0), "%s: boxes without their segments", who);
    MNY_REQUIRE(!labels || (boxes && atlas && strips), "%s: labels without their boxes, atlas or strip table", who);
    MNY_REQUIRE(C >= 0 && C <= kMaxSeg && (C == 0 || (seg && seg_channel)), "%s: %d seg classes (0..%d) or null planes", who, C, kMaxSeg);
    for (int c = 0; c < C; ++c) {
        MNY_REQUIRE(seg_channel[c] >= 0 && seg_channel[c] <= 2, "%s: seg_channel[%d] = %d is no RGB channel", who, c, seg_channel[c]);
        a.seg_channel[c] = seg_channel[c];
    }
    a.batch = batch; a.H = H; a.W = W; a.src = src; a.desc = desc; a.items = items; a.N = N;
    a.boxes = boxes; a.seg_begin = seg_begin; a.seg_count = seg_count; a.capacity = capacity;
    a.seg = seg; a.C = C; a.dst = dst; a.ws = (int*)ws;
    a.labels = labels; a.atlas = atlas; a.strips = strips;
    const int64_t bound = (int64_t)N * cdiv(max_w, kTileW) * cdiv(max_h, kTileH);
    const unsigned grid = (unsigned)(bound < 4096 ? bound : 4096);
    if (labels)
        viz_compose_kernel<compose_label_args><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else
        viz_compose_kernel<compose_args><<<grid, 256, 0, (hipStream_t)stream>>>(a);  // the kernel without labels, on the base of `a`
    return check_launch(who);
}

extern "C" int mny_viz_compose(const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                               const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes,
                               const int32_t* seg_begin, const int32_t* seg_count, int capacity, const float* seg, int C,
                               const int32_t* seg_channel, uint8_t* dst, void* ws, void* stream) {
    return compose("mny_viz_compose", batch, H, W, mean3, std3, src, desc, items, N, boxes, seg_begin, seg_count, capacity, seg, C, seg_channel, dst,
                   ws, nullptr, nullptr, nullptr, stream);
}

extern "C" int mny_viz_compose_labels(const float* batch, int H, int W, const float* mean3, const float* std3, const uint8_t* src,
                                      const mny_image_desc* desc, const mny_viz_item* items, int N, const mny_viz_box* boxes,
                                      const int32_t* seg_begin, const int32_t* seg_count, int capacity, const float* seg, int C,
                                      const int32_t* seg_channel, uint8_t* dst, void* ws, const mny_viz_label* labels, const uint8_t* atlas,
                                      const int32_t* strips, void* stream) {
    return compose("mny_viz_compose_labels", batch, H, W, mean3, std3, src, desc, items, N, boxes, seg_begin, seg_count, capacity, seg, C,
                   seg_channel, dst, ws, labels, atlas, strips, stream);
}
