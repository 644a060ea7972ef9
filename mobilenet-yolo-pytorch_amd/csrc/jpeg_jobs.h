// The job list of the JPEG kernels (csrc/jpeg.hip, csrc/jpegenc.hip): every workgroup rebuilds, in LDS, the exclusive prefix sum
// of the per-image job counts from the item records, as augseq.hip does, and finds the image of a job by bisection.
#pragma once
#include <stdint.h>

namespace mny {
namespace jpeg_jobs {

constexpr int kMaxItems = 4096;

struct job_lds {
    uint32_t pref[kMaxItems + 1];
    uint32_t part[256];
};

// exclusive prefix sum of count(i) over the items into J.pref; -> the total
template <typename F>
__device__ uint32_t build_jobs(job_lds& J, int n, F count) {
    const int tid = threadIdx.x;
    const int per = (n + 255) / 256;
    const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
    uint32_t local = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t c = count(i);
        J.pref[i] = c;
        local += c;
    }
    J.part[tid] = local;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const uint32_t add = tid >= s ? J.part[tid - s] : 0u;
        __syncthreads();
        J.part[tid] += add;
        __syncthreads();
    }
    uint32_t run = J.part[tid] - local;
    for (int i = i0; i < i1; ++i) {
        const uint32_t c = J.pref[i];
        J.pref[i] = run;
        run += c;
    }
    const uint32_t total = J.part[255];
    if (tid == 0) J.pref[n] = total;
    __syncthreads();
    return total;
}

__device__ __forceinline__ int find_item(const job_lds& J, int n, uint32_t job) {   // the last item with pref <= job
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.pref[mid] <= job) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace jpeg_jobs
}  // namespace mny
