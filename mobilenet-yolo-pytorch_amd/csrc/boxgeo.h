// Class test, image lookup and fp64 box geometry of the packed evaluation layout (include/mnyolo.h: mny_coco_eval), shared by
// cocoeval.hip and detreport.hip.  Both are compiled with -ffp-contract=off: areas and IoUs must round like the separate fp64
// operations of the specification.  Unnamed namespace: every translation unit that includes it gets its own copy.
#pragma once
#include "common.h"

namespace mny {
namespace {

__device__ __forceinline__ uint32_t class_of(float label, int n_classes) {
    if (!(label >= 1.f && label <= (float)(n_classes - 1))) return 0;
    const uint32_t c = (uint32_t)label;
    return (float)c == label ? c : 0;
}

__device__ __forceinline__ int image_of(const int32_t* off, int n_images, int d) {   // largest i with off[i] <= d
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= d) lo = mid; else hi = mid;
    }
    return lo;
}

struct geo { double x1, y1, w, h, area; };

__device__ __forceinline__ geo geo_of(const float* boxes, size_t i, double W, double H) {
    const float4 b = ld4(boxes + 4 * i);
    geo g;
    g.x1 = (double)b.x * W; g.y1 = (double)b.y * H;
    g.w = (double)b.z * W - g.x1; g.h = (double)b.w * H - g.y1;
    g.area = g.w * g.h;
    return g;
}

__device__ __forceinline__ double iou_of(const geo& d, const geo& g, bool crowd) {    // maskApi.c bbIou on (x, y, w, h)
    const double iw = fmin(d.x1 + d.w, g.x1 + g.w) - fmax(d.x1, g.x1);
    if (iw <= 0) return 0.0;
    const double ih = fmin(d.y1 + d.h, g.y1 + g.h) - fmax(d.y1, g.y1);
    if (ih <= 0) return 0.0;
    const double inter = iw * ih;
    const double uni = crowd ? d.area : (d.area + g.area) - inter;
    return inter / uni;
}

__device__ __forceinline__ void size_of(const float* image_sizes, int img, double& W, double& H) {
    W = image_sizes ? (double)image_sizes[2 * (size_t)img] : 1.0;
    H = image_sizes ? (double)image_sizes[2 * (size_t)img + 1] : 1.0;
}

}  // namespace
}  // namespace mny
