// Detection arithmetic with one definition for every file that must agree on its bits (detect.hip, postproc.hip): the cell decode of
// mny_yolo_decode / mny_yolo_decode_ex, the sort key of the NMS buckets, and the scan / gather tail of an NMS-shaped result.  Files that
// include this are compiled with -ffp-contract=off.  The kernels sit in an unnamed namespace: every translation unit gets its own copy.
#pragma once
#include "common.h"
#include "iou.h"      // Box

namespace mny {

// decode one cell; order of operations follows yolo_loss.py:89-92,243-247 (Q6, Q13)
__device__ __forceinline__ Box decode_box(float sx, float sy, float ew, float eh, int gx, int gy, float gf, float aw, float ah) {
    const float cx = (sx + (float)gx) / gf;
    const float cy = (sy + (float)gy) / gf;
    const float w = ew * aw, h = eh * ah;
    Box b;
    b.x1 = cx - w / 2; b.y1 = cy - h / 2;
    b.x2 = w + b.x1; b.y2 = h + b.y1;
    return b;
}

// the eval decode of one cell (yolo_loss.py:180-204): p = the cell's 5 + C logits, (aw, ah) its anchor
__device__ __forceinline__ Box decode_cell_box(const float* __restrict__ p, int gx, int gy, int g, float aw, float ah, float& conf) {
    const Box b = decode_box(sigmoid_ref(p[0]), sigmoid_ref(p[1]), expf(p[2]), expf(p[3]), gx, gy, (float)g, aw, ah);
    conf = sigmoid_ref(p[4]);
    return b;
}

// best class of a cell: first maximum of the per-class sigmoid, like torch.max (a NaN never wins)
__device__ __forceinline__ int decode_cell_best(const float* __restrict__ p, int C, float& best) {
    best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < C; ++c) {
        const float s = sigmoid_ref(p[5 + c]);
        if (s > best) { best = s; bi = c; }
    }
    return bi;
}

// sort key of a score: larger score -> smaller key (NMS buckets, mny_det_topk)
__device__ __forceinline__ uint32_t desc_key(float s) {
    uint32_t b = __float_as_uint(s);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // ascending-orderable
    return ~b;
}

namespace {

// single block: exclusive scan of out_counts -> out_prefix[S+1]
__global__ __launch_bounds__(256) void nms_scan_kernel(const int32_t* __restrict__ counts, int S, int32_t* __restrict__ prefix) {
    __shared__ int32_t tot[256];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < S; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const int v = i < S ? counts[i] : 0;
        tot[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int t = threadIdx.x >= d ? tot[threadIdx.x - d] : 0;
            __syncthreads();
            tot[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < S) prefix[i] = carry + tot[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += tot[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) prefix[S] = carry;
}

// grid S: gather the kept rows densely, segment after segment
__global__ __launch_bounds__(256) void nms_gather_kernel(const float* __restrict__ rows, const int32_t* __restrict__ seg_begin,
                                                         const int32_t* __restrict__ out_idx, const int32_t* __restrict__ out_counts,
                                                         const int32_t* __restrict__ prefix, float* __restrict__ out_rows) {
    const int s = blockIdx.x;
    const int k = out_counts[s], b = seg_begin[s], o = prefix[s];
    for (int i = blockIdx.y * 256 + threadIdx.x; i < k * 7; i += gridDim.y * 256) {
        const int r = i / 7, f = i % 7;
        out_rows[(int64_t)(o + r) * 7 + f] = rows[(int64_t)out_idx[b + r] * 7 + f];
    }
}

}  // namespace
}  // namespace mny
