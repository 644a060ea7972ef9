// The reference's box IoU, one definition for every file that must agree on its bits (detect.hip, anchors.hip).  Files that include
// this are compiled with -ffp-contract=off: every product, sum and quotient below is an fp32 operation of its own.
#pragma once
#include <hip/hip_runtime.h>

namespace mny {

struct Box { float x1, y1, x2, y2; };

__device__ __forceinline__ float iou_ref(const Box& a, const Box& b) {   // utils/iou.py:32-49 (a = set_1)
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.f);
    const float inter = iw * ih;
    const float aa = (a.x2 - a.x1) * (a.y2 - a.y1);
    const float ab = (b.x2 - b.x1) * (b.y2 - b.y1);
    return inter / (aa + ab - inter);
}

// iou_ref on [0,0,w,h] and [0,0,aw,ah] for positive sizes, the two areas (area = w * h, a_area = aw * ah, one fp32 product each) formed
// by the caller: x - 0 and max(x, 0) are the identity there, so the bits are iou_ref's (include/mnyolo.h "Shape IoU")
__device__ __forceinline__ float shape_iou(float w, float h, float area, float aw, float ah, float a_area) {
    const float inter = fminf(w, aw) * fminf(h, ah);
    return inter / ((area + a_area) - inter);
}

}  // namespace mny
