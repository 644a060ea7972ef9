// Test-time augmentation of the detection path (include/mnyolo.h "test-time augmentation"): the mirrored / resized view of the
// input batch, the per-image append of one view's candidates behind the earlier views' (un-mirrored), and the score-weighted box
// merge behind the per-class NMS.  Built with -ffp-contract=off: the header states the arithmetic operation by operation, and
// tests/tta_ref.py restates it in numpy bit for bit.
#include "common.h"

namespace mny {

// ---- mny_tta_view ----------------------------------------------------------------------------------------------------
// a thread per output element, columns fastest: coalesced stores, and the two source rows a wave reads are contiguous spans
// (reversed under `flip`).  fp64 throughout, one rounding at the end.

// w0 * p + w1 * q without the term whose weight is exactly 0 (a non-finite neighbour cannot poison an exact sample)
__device__ __forceinline__ double mix2(double w0, double p, double w1, double q) {
    if (w1 == 0.0) return w0 * p;
    if (w0 == 0.0) return w1 * q;
    return w0 * p + w1 * q;
}

__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int Hs, int Ws, int Hd,
                                                       int Wd, double ry, double rx, int flip) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int x = (int)(e % Wd);
        const int64_t t = e / Wd;
        const int y = (int)(t % Hd);
        const int64_t plane = t / Hd;                                      // n * C + c
        double sy = ((double)y + 0.5) * ry - 0.5; if (!(sy > 0.0)) sy = 0.0;
        double sx = ((double)x + 0.5) * rx - 0.5; if (!(sx > 0.0)) sx = 0.0;
        int y0 = (int)sy; if (y0 > Hs - 1) y0 = Hs - 1;                    // (never taken: sy < Hs - 0.5; the bound is for the loads)
        int x0 = (int)sx; if (x0 > Ws - 1) x0 = Ws - 1;
        const int y1 = y0 + 1 < Hs - 1 ? y0 + 1 : Hs - 1;
        const int x1 = x0 + 1 < Ws - 1 ? x0 + 1 : Ws - 1;
        const double ly = sy - (double)y0, lx = sx - (double)x0;
        const double wy0 = 1.0 - ly, wx0 = 1.0 - lx;
        const int c0 = flip ? Ws - 1 - x0 : x0, c1 = flip ? Ws - 1 - x1 : x1;
        const float* p0 = src + (plane * Hs + y0) * (int64_t)Ws;
        const float* p1 = src + (plane * Hs + y1) * (int64_t)Ws;
        const double top = mix2(wx0, (double)p0[c0], lx, (double)p0[c1]);
        double v;
        if (ly == 0.0) {
            v = wy0 * top;
        } else {
            const double bot = mix2(wx0, (double)p1[c0], lx, (double)p1[c1]);
            v = mix2(wy0, top, ly, bot);
        }
        dst[e] = (float)v;
    }
}

// ---- mny_det_append ----------------------------------------------------------------------------------------------------
// a workgroup per image: every thread reads the image's base count, the copy runs over the 7 * copied floats, and thread 0 moves
// the count behind a barrier (no other workgroup reads or writes this image's count)
__global__ __launch_bounds__(256) void det_append_kernel(const float* __restrict__ src_rows, int src_stride, const int32_t* __restrict__ src_counts,
                                                         int flip, float* __restrict__ dst_rows, int dst_stride, int32_t* __restrict__ counts) {
    const int n = blockIdx.x;
    const int base = counts[n];
    int m = src_counts[n];
    if (m > src_stride) m = src_stride;
    if (base < 0 || base > dst_stride) m = 0;                              // a count outside its segment: nothing is appended
    else if (m > dst_stride - base) m = dst_stride - base;                  // clamp: never write outside the image's segment
    if (m < 0) m = 0;
    const float* s = src_rows + (int64_t)n * src_stride * 7;
    float* d = dst_rows + ((int64_t)n * dst_stride + base) * 7;
    for (int e = threadIdx.x; e < m * 7; e += 256) {
        const int col = e % 7;
        float v;
        if (flip && col == 0) v = 1.0f - s[e + 2];                          // x1' = 1 - x2
        else if (flip && col == 2) v = 1.0f - s[e - 2];                     // x2' = 1 - x1
        else v = s[e];
        d[e] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[n] = base + m;
}

// ---- mny_nms_merge -----------------------------------------------------------------------------------------------------
// grid (S, MERGE_SLICES), 256 threads: a lane per kept box of the segment; the segment's rows pass through LDS in chunks of 256
// (box, weight, class: every lane reads the same LDS address per step, a broadcast) and each lane adds its members in ascending
// row order in fp64: the order of every sum is fixed, no sum is split across lanes.
constexpr int MERGE_SLICES = 8;

__global__ __launch_bounds__(256) void nms_merge_kernel(const float* __restrict__ rows, const int32_t* __restrict__ seg_begin,
                                                        const int32_t* __restrict__ seg_count, const int32_t* __restrict__ out_idx,
                                                        const int32_t* __restrict__ out_counts, const int32_t* __restrict__ out_prefix, double thr,
                                                        float* __restrict__ out_rows) {
    __shared__ float4 cbox[256];
    __shared__ float cw[256], ccls[256];
    const int s = blockIdx.x;
    const int begin = seg_begin[s];
    const int n = max(seg_count[s], 0);
    const int K = min(max(out_counts[s], 0), n);                           // (a segment keeps at most its own rows)
    const int o = out_prefix[s];
    for (int p0 = blockIdx.y * 256; p0 < K; p0 += MERGE_SLICES * 256) {    // workgroup-uniform trip counts: the barriers below are safe
        const int p = p0 + threadIdx.x;
        int i = -1;
        if (p < K) {
            i = out_idx[begin + p];
            if (i < begin || i >= begin + n) i = -1;                       // not a row of this segment: the output row stays as it is
        }
        float4 kb = make_float4(0.f, 0.f, 0.f, 0.f);
        float c = 0.f;
        if (i >= 0) {
            const float* r = rows + (int64_t)i * 7;
            kb = make_float4(r[0], r[1], r[2], r[3]);
            c = r[6];
        }
        const float ia = (kb.z - kb.x) * (kb.w - kb.y);
        double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int j0 = 0; j0 < n; j0 += 256) {
            const int lim = min(256, n - j0);
            __syncthreads();                                               // the previous chunk has been read by every lane
            if ((int)threadIdx.x < lim) {
                const float* r = rows + (int64_t)(begin + j0 + threadIdx.x) * 7;
                cbox[threadIdx.x] = make_float4(r[0], r[1], r[2], r[3]);
                cw[threadIdx.x] = r[5] * r[4];                             // the NMS score (utils/box.py:27), one fp32 product
                ccls[threadIdx.x] = r[6];
            }
            __syncthreads();
            if (i < 0) continue;
            for (int q = 0; q < lim; ++q) {
                if (!(ccls[q] == c)) continue;
                const float4 bx = cbox[q];
                bool member = (begin + j0 + q == i);
                if (!member) {                                             // the IoU of nms_bucket_kernel (detect.hip), kept box first
                    const float aj = (bx.z - bx.x) * (bx.w - bx.y);
                    const float xx1 = kb.x > bx.x ? kb.x : bx.x, yy1 = kb.y > bx.y ? kb.y : bx.y;
                    const float xx2 = kb.z < bx.z ? kb.z : bx.z, yy2 = kb.w < bx.w ? kb.w : bx.w;
                    float w = xx2 - xx1; if (!(w > 0.f)) w = 0.f;
                    float h = yy2 - yy1; if (!(h > 0.f)) h = 0.f;
                    const float inter = w * h;
                    const float ovr = inter / (ia + aj - inter);
                    member = (double)ovr > thr;
                }
                if (member) {
                    const double wj = (double)cw[q];
                    sw += wj;
                    s0 += wj * (double)bx.x;
                    s1 += wj * (double)bx.y;
                    s2 += wj * (double)bx.z;
                    s3 += wj * (double)bx.w;
                }
            }
        }
        if (i >= 0) {
            float* d = out_rows + (int64_t)(o + p) * 7;
            const bool ok = sw > 0.0 && sw < INFINITY;                     // finite and positive (a NaN fails both compares)
            d[0] = ok ? (float)(s0 / sw) : kb.x;
            d[1] = ok ? (float)(s1 / sw) : kb.y;
            d[2] = ok ? (float)(s2 / sw) : kb.z;
            d[3] = ok ? (float)(s3 / sw) : kb.w;
        }
    }
}

}  // namespace mny

using namespace mny;

extern "C" int mny_tta_view(const float* src, float* dst, int N, int C, int Hs, int Ws, int Hd, int Wd, int flip, void* stream) {
    MNY_REQUIRE(src && dst, "tta_view: null pointer");
    MNY_REQUIRE(N > 0 && C > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "tta_view: sizes must be >= 1 (N %d C %d, %dx%d -> %dx%d)", N, C, Hs, Ws, Hd, Wd);
    MNY_REQUIRE(src != dst, "tta_view: in-place views are not supported");
    const int64_t total = (int64_t)N * C * Hd * Wd;
    MNY_REQUIRE((int64_t)N * C * Hs * Ws < ((int64_t)1 << 40) && total < ((int64_t)1 << 40), "tta_view: tensor too large");
    const double ry = (double)Hs / (double)Hd, rx = (double)Ws / (double)Wd;
    const int64_t blocks = cdiv(total, 256);
    hipLaunchKernelGGL(tta_view_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, src, dst, total, Hs, Ws, Hd,
                       Wd, ry, rx, flip ? 1 : 0);
    return check_launch("tta_view_kernel");
}

extern "C" int mny_det_append(const float* src_rows, int src_stride, const int32_t* src_counts, int flip, float* dst_rows, int dst_stride,
                              int32_t* counts, int N, void* stream) {
    MNY_REQUIRE(N >= 0 && src_stride >= 0 && dst_stride >= 0, "det_append: bad sizes (N %d, strides %d -> %d)", N, src_stride, dst_stride);
    if (N == 0) return MNY_OK;
    MNY_REQUIRE(src_counts && counts, "det_append: null pointer");
    MNY_REQUIRE((src_rows || src_stride == 0) && (dst_rows || dst_stride == 0), "det_append: null rows with a non-zero stride");
    MNY_REQUIRE(src_stride <= (1 << 28) / 7 && dst_stride <= (1 << 28) / 7, "det_append: stride too large");
    hipLaunchKernelGGL(det_append_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, src_rows, src_stride, src_counts, flip ? 1 : 0, dst_rows,
                       dst_stride, counts);
    return check_launch("det_append_kernel");
}

extern "C" int mny_nms_merge(const float* rows, const int32_t* seg_begin, const int32_t* seg_count, int S, const int32_t* out_idx,
                             const int32_t* out_counts, const int32_t* out_prefix, double thr, float* out_rows, void* stream) {
    MNY_REQUIRE(S >= 0, "nms_merge: bad segment count %d", S);
    if (S == 0) return MNY_OK;
    MNY_REQUIRE(seg_begin && seg_count && out_idx && out_counts && out_prefix && out_rows, "nms_merge: null pointer");
    MNY_REQUIRE(thr == thr, "nms_merge: thr is NaN");
    hipLaunchKernelGGL(nms_merge_kernel, dim3(S, MERGE_SLICES), dim3(256), 0, (hipStream_t)stream, rows, seg_begin, seg_count, out_idx, out_counts,
                       out_prefix, thr, out_rows);
    return check_launch("nms_merge_kernel");
}
