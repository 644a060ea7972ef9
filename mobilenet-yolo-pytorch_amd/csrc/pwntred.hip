// The pointwise data-gradient GEMMs with a reduction epilogue: the RED != 0 instantiations of the LDS-DMA ring NT kernel (pwnt_kernel.h) —
// a unit of their own so that they compile beside the forward instantiations of pwgemm.hip, not behind them.
#include "pwnt_kernel.h"

namespace mny {

Nt2Kernel nt2_red_kernel(int TN, int XF, int BF, int RED, int X6, int RB) {
#define MNY_K(T, XF_, BF_, RED_, X6_, RB_) case nt2_key(T, XF_, BF_, RED_, X6_, RB_): return (Nt2Kernel)pw_gemm_nt_dma_kernel<T, XF_, BF_, RED_, X6_, RB_>;
#define MNY_RED(T, RED_) MNY_K(T, 0, 0, RED_, 0, 0) MNY_K(T, 0, 0, RED_, 1, 0) MNY_K(T, 0, 1, RED_, 0, 0)           // fp32 MFMA, six-product, bf16 storage
#define MNY_FIX(T) MNY_K(T, 0, 0, 2, 0, 1) MNY_K(T, 0, 0, 2, 1, 1) MNY_K(T, 1, 0, 2, 0, 1) MNY_K(T, 1, 0, 2, 1, 1)
    switch (nt2_key(TN, XF, BF, RED, X6, RB)) {
        // data gradient + BatchNorm sums (RED = 1; = 2: with an addend — own instantiations: the addend loads cost the TN = 4 variant registers),
        // column tiles of <= 128 (kRedMaxTn); on weight planes the addend form stops at 96
        MNY_RED(1, 1) MNY_RED(2, 1) MNY_RED(3, 1) MNY_RED(4, 1) MNY_RED(1, 2) MNY_RED(2, 2) MNY_RED(3, 2) MNY_RED(4, 2)
        MNY_K(1, 0, 0, 1, 3, 0) MNY_K(2, 0, 0, 1, 3, 0) MNY_K(3, 0, 0, 1, 3, 0) MNY_K(4, 0, 0, 1, 3, 0)
        MNY_K(1, 0, 0, 2, 3, 0) MNY_K(2, 0, 0, 2, 3, 0) MNY_K(3, 0, 0, 2, 3, 0)
        // low-rank fix with a reduction target (RB = 1: the bias row r), column tiles of <= 96
        MNY_FIX(1) MNY_FIX(2) MNY_FIX(3)
    }
#undef MNY_FIX
#undef MNY_RED
#undef MNY_K
    return nullptr;
}

}  // namespace mny
