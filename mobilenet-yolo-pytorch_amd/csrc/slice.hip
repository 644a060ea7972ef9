// Sliced (tiled) inference of the detection path (include/mnyolo.h "sliced inference"): the batch prep that reads crop windows of
// larger source images (one network input per tile, at native resolution) and the append that moves every tile's candidates
// through the tile's affine map into the joint per-image segment, dropping the boxes that an interior tile edge cuts.
// Built with -ffp-contract=off: the header states the arithmetic operation by operation, tests/slice_ref.py restates it in numpy.
// No atomics on row positions: every position is an ordered scan, the results are bit-reproducible.
#include "prep_kernels.h"

namespace mny {

// ---- mny_det_append_tiles ----------------------------------------------------------------------------------------------
// One workgroup per destination image.  It walks the B slots in ascending order and takes the ones whose map names its image (the
// test is workgroup-uniform), so the rows of one image are written by one workgroup, slot after slot, in source order: no other
// workgroup reads or writes this image's count.  Within a slot the rows pass in trips of 256; a row survives (0 / 1), the inclusive
// scan over the wave plus the four wave totals through LDS give its position, as in yolo_decode_ex_kernel (postproc.hip).
__global__ __launch_bounds__(256) void det_append_tiles_kernel(const float* __restrict__ src_rows, int src_stride, const int32_t* __restrict__ src_counts,
                                                               const mny_tile_map* __restrict__ maps, int B, float* __restrict__ dst_rows, int dst_stride,
                                                               int32_t* __restrict__ counts, int32_t* __restrict__ dropped) {
    __shared__ int wsum[4];
    const int n = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base0 = counts[n];
    const int room = (base0 >= 0 && base0 <= dst_stride) ? dst_stride - base0 : 0;     // rows this image may still write
    float* seg = dst_rows + ((int64_t)n * dst_stride + (room > 0 ? base0 : 0)) * 7;
    int total = 0;                                                                      // survivors so far: the same value in every thread
    for (int b = 0; b < B; ++b) {
        if (maps[b].image != n) continue;
        const mny_tile_map mp = maps[b];
        int m = src_counts[b];
        if (m > src_stride) m = src_stride;
        const float* s = src_rows + (int64_t)b * src_stride * 7;
        for (int r0 = 0; r0 < m; r0 += 256) {                                          // (m < 0: no trip)
            const int r = r0 + threadIdx.x;
            float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int keep = 0;
            if (r < m) {
#pragma unroll
                for (int c = 0; c < 7; ++c) v[c] = s[(int64_t)r * 7 + c];
                const bool cut = ((mp.interior & 1u) && v[0] < mp.ex) || ((mp.interior & 4u) && v[2] > 1.0f - mp.ex) ||
                                 ((mp.interior & 2u) && v[1] < mp.ey) || ((mp.interior & 8u) && v[3] > 1.0f - mp.ey);
                keep = cut ? 0 : 1;
            }
            int inc = keep;                                                             // inclusive scan over the wave
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
            const int pos = total + woff + inc - keep;
            if (keep && pos < room) {
                float* d = seg + (int64_t)pos * 7;
                d[0] = (float)(mp.ax + mp.bx * (double)v[0]);                           // two fp64 operations, one rounding
                d[1] = (float)(mp.ay + mp.by * (double)v[1]);
                d[2] = (float)(mp.ax + mp.bx * (double)v[2]);
                d[3] = (float)(mp.ay + mp.by * (double)v[3]);
                d[4] = v[4]; d[5] = v[5]; d[6] = v[6];
            }
            total += trip;
            __syncthreads();                                                            // wsum is rewritten by the next trip
        }
    }
    if (threadIdx.x == 0 && total > 0) {
        const int written = total < room ? total : room;
        counts[n] = base0 + written;
        dropped[n] += total - written;
    }
}

}  // namespace mny

using namespace mny;

extern "C" size_t mny_prep_tiles_ws_bytes(int B, int max_h, int max_w, int out_h, int out_w) {
    if (B < 1 || max_h < 1 || max_w < 1 || out_h < 1 || out_w < 1) return 0;
    return make_layout(B, max_h, max_w, out_h, out_w).total;
}

extern "C" int mny_prep_tiles(const uint8_t* src, const mny_tile_desc* tiles, int B, int max_h, int max_w, int out_h, int out_w, const float* mean3,
                              const float* std3, float* out, void* ws, void* stream) {
    MNY_REQUIRE(src && tiles && mean3 && std3 && out && ws, "mny_prep_tiles: null pointer");
    MNY_REQUIRE(B >= 1 && max_h >= 1 && max_w >= 1 && out_h >= 1 && out_w >= 1, "mny_prep_tiles: bad sizes B=%d in<=%dx%d out=%dx%d", B, max_h, max_w,
                out_h, out_w);
    MNY_REQUIRE((int64_t)max_h * out_w < ((int64_t)1 << 31) / 3 && B <= 65535, "mny_prep_tiles: window too large / more than 65535 slots");
    MNY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "mny_prep_tiles: std must be non-zero");
    return prep_launch<mny_tile_desc>("mny_prep_tiles", src, tiles, B, max_h, max_w, out_h, out_w, mean3, std3, out, ws, (hipStream_t)stream);
}

extern "C" int mny_det_append_tiles(const float* src_rows, int src_stride, const int32_t* src_counts, const mny_tile_map* maps, int B, float* dst_rows,
                                    int dst_stride, int32_t* counts, int32_t* dropped, int N, void* stream) {
    MNY_REQUIRE(B >= 0 && N >= 0 && src_stride >= 0 && dst_stride >= 0, "det_append_tiles: bad sizes (B %d, N %d, strides %d -> %d)", B, N, src_stride,
                dst_stride);
    if (B == 0 || N == 0) return MNY_OK;
    MNY_REQUIRE(src_counts && maps && counts && dropped, "det_append_tiles: null pointer");
    MNY_REQUIRE((src_rows || src_stride == 0) && (dst_rows || dst_stride == 0), "det_append_tiles: null rows with a non-zero stride");
    MNY_REQUIRE(src_stride <= (1 << 28) / 7 && dst_stride <= (1 << 28) / 7, "det_append_tiles: stride too large");
    hipLaunchKernelGGL(det_append_tiles_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, src_rows, src_stride, src_counts, maps, B, dst_rows,
                       dst_stride, counts, dropped);
    return check_launch("det_append_tiles_kernel");
}
