// Sort of (64-bit key, 32-bit value) pairs on the device, shared by the evaluation stages (evalmap.hip, cocoeval.hip, detreport.hip).
// Everything sits in an unnamed namespace of namespace mny: every translation unit that includes it gets its own copy of the kernels.
#pragma once
#include "common.h"

namespace mny {
namespace {

// ---- sort of (key, value) pairs, ascending in (key, value) ----------------------------------------------------------------
// The values of equal keys are distinct and ascend in stored order (evalmap.hip: stored detection index << 2 | flags; cocoeval.hip: the
// index; detreport.hip: index << 1 | TP), so the pair order is total and equals the stable order by key.  Bitonic network
// over n2 = 2^m >= D padded pairs: every run of steps with partner distance < kSortChunk happens inside LDS (one workgroup per
// 4096-pair chunk), the few steps with a longer distance are one global compare-exchange pass each (6 MB for VOC07-test).
constexpr int kSortChunk = 4096;

__device__ __forceinline__ bool pair_gt(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb) { return ka > kb || (ka == kb && va > vb); }

__global__ void map_sort_pad_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int D, int n2) {
    const int i = D + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n2) { keys[i] = ~0ull; vals[i] = ~0u; }
}

// steps j = j_first, j_first/2, ..., 1 of stage k (or, with k_first > 0, ALL stages k = 2 .. k_first) on one chunk
__global__ __launch_bounds__(1024) void map_sort_local_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int k_first, int k, int j_first) {
    __shared__ uint64_t sk[kSortChunk];
    __shared__ uint32_t sv[kSortChunk];
    const int base = blockIdx.x * kSortChunk;
    for (int i = threadIdx.x; i < kSortChunk; i += blockDim.x) { sk[i] = keys[base + i]; sv[i] = vals[base + i]; }
    __syncthreads();
    auto steps = [&](int kk, int jf) {
        for (int j = jf; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < kSortChunk; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = ((base + i) & kk) == 0;
                    const uint64_t a = sk[i], b = sk[l];
                    const uint32_t x = sv[i], y = sv[l];
                    if (pair_gt(a, x, b, y) == up) { sk[i] = b; sk[l] = a; sv[i] = y; sv[l] = x; }
                }
            }
            __syncthreads();
        }
    };
    if (k_first > 0) { for (int kk = 2; kk <= k_first; kk <<= 1) steps(kk, kk >> 1); }
    else steps(k, j_first);
    for (int i = threadIdx.x; i < kSortChunk; i += blockDim.x) { keys[base + i] = sk[i]; vals[base + i] = sv[i]; }
}

__global__ void map_sort_global_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int n2, int k, int j) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = i ^ j;
    if (i >= n2 || l <= i) return;
    const bool up = (i & k) == 0;
    const uint64_t a = keys[i], b = keys[l];
    const uint32_t x = vals[i], y = vals[l];
    if (pair_gt(a, x, b, y) == up) { keys[i] = b; keys[l] = a; vals[i] = y; vals[l] = x; }
}

inline int sort_size(int64_t D) { int n2 = kSortChunk; while (n2 < D) n2 <<= 1; return n2; }

int sort_pairs(uint64_t* keys, uint32_t* vals, int D, hipStream_t st) {
    const int n2 = sort_size(D);
    if (n2 > D) map_sort_pad_kernel<<<(int)cdiv(n2 - D, 256), 256, 0, st>>>(keys, vals, D, n2);
    const int chunks = n2 / kSortChunk;
    map_sort_local_kernel<<<chunks, 1024, 0, st>>>(keys, vals, kSortChunk, 0, 0);
    for (int k = 2 * kSortChunk; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= kSortChunk; j >>= 1) map_sort_global_kernel<<<(int)cdiv(n2, 256), 256, 0, st>>>(keys, vals, n2, k, j);
        map_sort_local_kernel<<<chunks, 1024, 0, st>>>(keys, vals, 0, k, kSortChunk >> 1);
    }
    return check_launch("mny_map sort");
}

__device__ __forceinline__ int lower_bound_key(const uint64_t* keys, int n, uint64_t k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace
}  // namespace mny
