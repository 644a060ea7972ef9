// Sixteen zero bytes in device memory: what an LDS-DMA instruction reads for a chunk past the end of its operand.  Included by exactly the units
// whose kernels use it (pwnt_kernel.h -> pwgemm.hip / pwntred.hip, pwwgrad.hip, pwbnbwd.hip): every unit that sees the definition gets its own copy.
#pragma once
#include "common.h"

namespace mny {

__device__ const float4 mny_zero16 = {0.f, 0.f, 0.f, 0.f};

}  // namespace mny
