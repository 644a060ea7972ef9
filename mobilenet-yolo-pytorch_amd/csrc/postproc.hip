// Opt-in post-processing of the detection path (include/mnyolo.h "post-processing options"): the decode with a score threshold, a
// candidate per (cell, class) pair (`multi_label`), a class filter and a capacity that is reported instead of required, and the
// per-segment top-k (`max_det`) behind either NMS.  The class-agnostic NMS itself is a flag on the bucket kernels of detect.hip.
// Built with -ffp-contract=off: the header states the arithmetic operation by operation, tests/post_ref.py restates it in numpy.
// No atomics anywhere: every position is a scan, the results are bit-reproducible.
#include "common.h"
#include "detshare.h" // the cell decode of yolo_decode_kernel, desc_key, scan / gather

namespace mny {

// ---- mny_yolo_decode_ex ------------------------------------------------------------------------------------------------
// One workgroup per image, 256 cells per trip like yolo_decode_kernel; a cell contributes m = 0..C rows, so the ballot of that kernel
// becomes an inclusive integer scan over the wave (6 shuffle steps) plus the four wave totals through LDS.  `total` (the rows of the
// trips so far) is the same value in every thread.  Multi-label cells evaluate their classes twice (count, then write): the second
// pass runs only in cells that emit, and stops at the end of the segment.
__device__ __forceinline__ bool class_allowed(const uint32_t* __restrict__ class_mask, int c) {
    return !class_mask || ((class_mask[c >> 5] >> (c & 31)) & 1u);
}

__global__ __launch_bounds__(256) void yolo_decode_ex_kernel(const float* __restrict__ head, const float* __restrict__ anchors,
                                                             const int32_t* __restrict__ mask, mny_yolo_head hp, float obj_thr, float score_thr,
                                                             int multi_label, const uint32_t* __restrict__ class_mask, float* __restrict__ rows,
                                                             int row_stride, const int32_t* __restrict__ base_counts, int32_t* __restrict__ counts,
                                                             int32_t* __restrict__ dropped) {
    __shared__ int wsum[4];
    const int n = blockIdx.x, g = hp.g, A = hp.A, C = hp.C, T = 5 + hp.C;
    const int cells = A * g * g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base0 = base_counts ? base_counts[n] : 0;
    const int room = (base0 >= 0 && base0 <= row_stride) ? row_stride - base0 : 0;     // rows this image may still write
    const bool score_on = !(score_thr < 0.f);
    float* seg = rows + ((int64_t)n * row_stride + (room > 0 ? base0 : 0)) * 7;
    int total = 0;
    for (int c0 = 0; c0 < cells; c0 += 256) {
        const int cell = c0 + threadIdx.x;       // (a, gy, gx) order: yolo_loss.py:201-203
        const float* p = head;
        Box b{0.f, 0.f, 0.f, 0.f};
        float conf = 0.f, best = 0.f;
        int bi = 0, m = 0;
        if (cell < cells) {
            const int gx = cell % g, gy = (cell / g) % g, a = cell / (g * g);
            p = head + (((int64_t)n * g + gy) * g + gx) * (A * T) + a * T;
            const int am = mask[a];
            b = decode_cell_box(p, gx, gy, g, anchors[am * 2], anchors[am * 2 + 1], conf);
            if (!multi_label) {
                bi = decode_cell_best(p, C, best);
                m = (conf > obj_thr && (!score_on || conf * best > score_thr) && class_allowed(class_mask, bi)) ? 1 : 0;
            } else if (conf > obj_thr) {
                for (int c = 0; c < C; ++c) {
                    const float cls = sigmoid_ref(p[5 + c]);
                    if ((!score_on || conf * cls > score_thr) && class_allowed(class_mask, c)) ++m;
                }
            }
        }
        int inc = m;                              // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int trip = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        int pos = total + woff + inc - m;
        if (m && pos < room) {
            if (!multi_label) {
                float* dst = seg + (int64_t)pos * 7;
                dst[0] = b.x1; dst[1] = b.y1; dst[2] = b.x2; dst[3] = b.y2; dst[4] = conf; dst[5] = best; dst[6] = (float)bi;
            } else {
                for (int c = 0; c < C && pos < room; ++c) {
                    const float cls = sigmoid_ref(p[5 + c]);
                    if ((!score_on || conf * cls > score_thr) && class_allowed(class_mask, c)) {
                        float* dst = seg + (int64_t)pos * 7;
                        dst[0] = b.x1; dst[1] = b.y1; dst[2] = b.x2; dst[3] = b.y2; dst[4] = conf; dst[5] = cls; dst[6] = (float)c;
                        ++pos;
                    }
                }
            }
        }
        total += trip;
        __syncthreads();                          // wsum is rewritten by the next trip
    }
    if (threadIdx.x == 0) {
        const int written = total < room ? total : room;
        counts[n] = base0 + written;
        dropped[n] = total - written;
    }
}

// ---- mny_det_topk ------------------------------------------------------------------------------------------------------
// One workgroup per segment: keys (desc_key(score) << 32 | position in the NMS output) of the segment's kept entries, a bitonic sort
// (ascending key == descending score, ties by position: the order inside an NMS bucket), the first min(k, max_det) entries' row
// indices staged through `tmp` and written back over out_idx.  Up to TOPK_LDS entries the keys sit in LDS; a longer list (only a
// segment that keeps more than 4096 boxes) is sorted in global scratch at gkeys + 2 * seg_begin, padded to a power of two < 2k: the
// regions of different segments stay disjoint, and __syncthreads orders the one workgroup's own global accesses.
constexpr int TOPK_LDS = 4096;

__global__ __launch_bounds__(256) void det_topk_kernel(const float* __restrict__ rows, const int32_t* __restrict__ seg_begin, int capacity,
                                                       int max_det, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_counts,
                                                       unsigned long long* __restrict__ gkeys, int32_t* __restrict__ tmp) {
    __shared__ unsigned long long skeys[TOPK_LDS];
    const int s = blockIdx.x;
    const int begin = seg_begin[s];
    int k = out_counts[s];
    if (k < 0 || begin < 0 || begin > capacity) k = 0;
    else if (k > capacity - begin) k = capacity - begin;                  // never read or write outside out_idx[capacity]
    if (k == 0) { if (threadIdx.x == 0) out_counts[s] = 0; return; }
    int n2 = 1; while (n2 < k) n2 <<= 1;
    unsigned long long* keys = n2 <= TOPK_LDS ? skeys : gkeys + 2 * (int64_t)begin;
    for (int r = threadIdx.x; r < n2; r += 256) {
        unsigned long long key = ~0ull;                                    // pad: sorts last
        if (r < k) {
            const int i = out_idx[begin + r];
            float score = 0.f;                                             // (not a row of `rows`: score 0, nothing is read)
            if (i >= 0 && i < capacity) { const float* q = rows + (int64_t)i * 7; score = q[5] * q[4]; }
            key = ((unsigned long long)desc_key(score) << 32) | (unsigned)r;
        }
        keys[r] = key;
    }
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    const bool up = (i & kk) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    const int kept = k < max_det ? k : max_det;
    for (int j = threadIdx.x; j < kept; j += 256) tmp[begin + j] = out_idx[begin + (int)(unsigned)(keys[j] & 0xFFFFFFFFull)];
    __syncthreads();                                                       // every old entry has been read
    for (int j = threadIdx.x; j < kept; j += 256) out_idx[begin + j] = tmp[begin + j];
    if (threadIdx.x == 0) out_counts[s] = kept;
}

}  // namespace mny

using namespace mny;

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int mny_yolo_decode_ex(const float* head, const float* anchors_all, const int32_t* mask, const mny_yolo_head* hp, float obj_thr,
                                  float score_thr, int multi_label, const uint32_t* class_mask, float* rows, int row_stride,
                                  const int32_t* base_counts, int32_t* counts, int32_t* dropped, void* stream) {
    MNY_REQUIRE(head && anchors_all && mask && hp && rows && counts && dropped, "yolo_decode_ex: null pointer");
    MNY_REQUIRE(hp->N > 0 && hp->g > 0 && hp->A > 0 && hp->C > 0, "yolo_decode_ex: bad head spec");
    MNY_REQUIRE(row_stride >= 1, "yolo_decode_ex: row_stride %d must be >= 1", row_stride);
    MNY_REQUIRE(obj_thr == obj_thr && score_thr == score_thr, "yolo_decode_ex: a threshold is NaN");
    MNY_REQUIRE((int64_t)hp->A * hp->g * hp->g * hp->C < ((int64_t)1 << 30) && (int64_t)hp->N * row_stride < ((int64_t)1 << 40),
                "yolo_decode_ex: head or row buffer too large");
    hipLaunchKernelGGL(yolo_decode_ex_kernel, dim3(hp->N), dim3(256), 0, (hipStream_t)stream, head, anchors_all, mask, *hp, obj_thr, score_thr,
                       multi_label ? 1 : 0, class_mask, rows, row_stride, base_counts, counts, dropped);
    return check_launch("yolo_decode_ex_kernel");
}

extern "C" size_t mny_det_topk_ws_bytes(int S, int capacity) {
    if (S < 0 || capacity < 0) return 0;
    const size_t cap = capacity > 0 ? capacity : 1;
    return align256(cap * 4) + align256(2 * cap * 8);                      // tmp int32[capacity] + sort keys u64[2 * capacity]
}

extern "C" int mny_det_topk(const float* rows, const int32_t* seg_begin, int S, int capacity, int max_det, int32_t* out_idx, int32_t* out_counts,
                            float* out_rows, int32_t* out_prefix, void* wsp, void* stream) {
    MNY_REQUIRE(max_det > 0, "det_topk: max_det must be >= 1, got %d", max_det);
    MNY_REQUIRE(S >= 0 && capacity >= 0, "det_topk: bad sizes (S %d, capacity %d)", S, capacity);
    if (S == 0 && !out_prefix) return MNY_OK;
    MNY_REQUIRE(out_prefix, "det_topk: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (S > 0) {
        MNY_REQUIRE(seg_begin && out_idx && out_counts && wsp && (rows || capacity == 0), "det_topk: null pointer");
        int32_t* tmp = (int32_t*)wsp;
        unsigned long long* gkeys = (unsigned long long*)((char*)wsp + align256((size_t)(capacity > 0 ? capacity : 1) * 4));
        hipLaunchKernelGGL(det_topk_kernel, dim3(S), dim3(256), 0, st, rows, seg_begin, capacity, max_det, out_idx, out_counts, gkeys, tmp);
    }
    hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(256), 0, st, out_counts, S, out_prefix);
    if (S > 0 && out_rows)
        hipLaunchKernelGGL(nms_gather_kernel, dim3(S, 1), dim3(256), 0, st, rows, seg_begin, out_idx, out_counts, out_prefix, out_rows);
    return check_launch("det_topk kernels");
}
