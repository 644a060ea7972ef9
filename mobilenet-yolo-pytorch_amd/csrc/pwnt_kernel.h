// The LDS-DMA ring NT kernel of the pointwise forward / data-gradient GEMMs, for the two units that instantiate it: pwgemm.hip (RED == 0: forward,
// plain data gradient) and pwntred.hip (RED != 0: data gradient + BatchNorm sums, low-rank fix) — 103 instantiations compile in two halves side by side.
#pragma once
#include <type_traits>

#include "common.h"
#include "dma_zero.h"      // mny_zero16: the DMA source for B chunks past K
#include "x6.h"

namespace mny {

constexpr int BM = 128;

// ------------------------------------------------------------------------------------------------
// NT GEMM v2: LDS-DMA pipeline.
//
// The register-staged kernel (pw_gemm_nt_kernel, pwntv1.hip) exposes HBM/L2 latency: one k-tile of prefetch, two waves per SIMD and
// one M-tile per block leave each wave idle ~60 % of the time.  v2 fixes the structure, CDNA4-style:
//   * global_load_lds_dwordx4 (LDS-DMA) copies tiles HBM -> LDS without touching VGPRs, so a 3-stage ring
//     keeps two k-tiles in flight behind the one being multiplied (counted `s_waitcnt vmcnt(N)` + raw
//     `s_barrier`: the DMA queue is never drained inside the loop);
//   * with no staging registers the kernel fits 3 workgroups per CU (48 KB LDS, <=168 VGPR+AGPR);
//   * each block is persistent over a run of consecutive M-tiles and walks one flat (tile, k-tile) sequence,
//     so the next tile's loads are already in flight during the epilogue stores;
//   * BN-apply + activation of the producer is applied when the A fragment is READ from LDS (3 VALU per
//     element, hidden under 64-cycle MFMAs) because a DMA cannot transform;
//   * the LDS image is lane-linear per DMA instruction (hardware rule), so bank conflicts are removed by
//     XOR-swizzling the 16-B chunk index on the SOURCE address and on the fragment read (chunk ^ (row>>2)&3);
//   * block id -> (m-run, n-tile) puts the n-tiles that share an A panel on the same XCD (bid % 8).
// Requirements: K % 4 == 0 (16-B aligned input rows); other K (the 75-channel heads' data gradient, the 10-channel gate) take
// the register-staged kernel.  A ragged output width (N % 4 != 0) is handled in the TRANSPOSED epilogue: up to four element
// stores off one address per row.  (An earlier scalar tail on the un-transposed accumulators — 16*TN stores with 16*TN
// addresses, fully unrolled — cost ~40 VGPRs and made the TN >= 3 main loops spill to scratch.)
// Out-of-range rows are clamped to a valid row (their outputs are never stored); k-chunks past K re-read the
// row start and are annihilated by zeroed B fragments (and zero scale/shift).
// ------------------------------------------------------------------------------------------------
struct Gemm2Args {   // A / B / addend / C: float* (BF = 0) or bf16_t* (BF = 1)
    const void* A; const float* in_scale; const float* in_shift; int in_act;
    const void* B; const float* bias; const void* addend; void* C; float* stats;
    int64_t M; int K; int N;
    int m_tiles, tiles_per_block, gx, n_tiles;
    // RED = 1 (data-gradient GEMM feeding a BN unit): C is that unit's dL/d(output); its BN-backward sums
    // (sum dz, sum dz*xhat per column, dz = C * act'(r_scale*rY + r_shift)) leave through `stats` instead of the plain column sums
    const void* rY; const float* r_scale; const float* r_shift; const float* r_mean; const float* r_invstd; int r_act;
};

// XF: 0 = A used as is, 1 = scale/shift + min(max(z, slope*z), hi) activation, 2 = scale/shift + hswish
// BF: 0 = fp32 operands, v_mfma_f32_32x32x2_f32;  1 = bf16 operands (A, B, addend, C), v_mfma_f32_32x32x16_bf16.
//     The LDS image is the same in bytes (64-B rows of four 16-B chunks): a chunk is 4 fp32 or 8 bf16 k-values, a stage
//     covers 16 or 32 k, and the lane's 16-B fragment read IS the bf16 MFMA operand (k-block = lane>>5), so the bf16
//     main loop is 2 MFMAs per accumulator per stage instead of 16.
#ifndef MNY_W6_GROUP
#define MNY_W6_GROUP 4            // SWP: column blocks advanced together (an accumulator's next product is this many MFMA issues away)
#endif
#ifndef MNY_W6_SWP
#define MNY_W6_SWP 1              // planes mode without a reduction epilogue: the A fragment of stage t is read, transformed and cut BETWEEN the MFMAs of stage t-1 (0: one stage at a time)
#endif
// RB (RED kernels only): the product carries the per-column constant p.bias INSIDE the sums of the reduction epilogue (mny_pw_lr_fix); a template
// flag, not a run-time test: one more live register in the data-gradient instantiations broke the bf16 TN = 3 addend form (NaN outputs, round 6)
template <int TN, int XF, int BF, int RED = 0, int X6 = 0, int RB = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((X6 == 3 && RED == 0 && MNY_W6_SWP) ? 2 : 3, 8))) void pw_gemm_nt_dma_kernel(Gemm2Args p) {
    using T = typename std::conditional<BF != 0, bf16_t, float>::type;
    constexpr int EPC = BF ? 8 : 4;                                           // elements per 16-B chunk
    constexpr int BKE = 4 * EPC;                                              // k-values per stage
    const T* pA = (const T*)p.A;
    const T* pB = (const T*)p.B;
    const T* pAdd = (const T*)p.addend;
    T* pC = (T*)p.C;
    constexpr int BN = 32 * TN, BKD = 16, S = 3;
    // X6 == 3: B arrives PRE-CUT (mny_cut3_batch): three bf16 planes [N][nk][2][8], the eight k-values of a 16-B chunk in the order a lane
    // of this kernel holds them (k = 4h..4h+3, 8+4h..8+4h+3 for half h); a stage of B is 3 x 32*TN rows x 32 B, one DMA instruction per
    // (plane, 32-row block).  Lane l of that instruction fetches (column l & 31, half l >> 5), so the lane-linear LDS image is
    // [half][column] and lane (column, half) reads back ITS OWN 16 bytes: consecutive lanes, consecutive chunks, no bank conflict.
    // (Round 2 laid the image out [column][half]: the lanes of a half then read every OTHER chunk — SQ_LDS_BANK_CONFLICT was 40 % of
    // the LDS-active cycles of every planes kernel, profiles/r03_pmc_step_lds.txt.)
    constexpr int A_ST = BM * BKD, B_ST = X6 == 3 ? BN * 24 : BN * BKD;                          // floats
    constexpr int NA = BM / 16, NB = X6 == 3 ? 3 * TN : BN / 16, NL = NA + NB;                   // 1-KiB DMA instructions per stage
    constexpr int LPW = (NL + 3) / 4;                                         // per wave (surplus ones duplicate the last)
    // Ring layout: [S slots of A][SB slots of B][scale / shift cache].  Planes mode (round 3): the pre-cut weight planes are L2-resident
    // and need less lead than the activation rows from HBM, so their ring is TWO slots deep (stage t+1 is requested while stage t is
    // multiplied, A stays two stages ahead): 3 x 8 KB + 2 x 3 TN KB is exactly the LDS of the plain mode (3 x (8 + 2 TN) KB), so the planes
    // kernels keep the plain mode's THREE resident workgroups per CU — with a three-slot plane ring (60 KB at TN = 4) they ran two.
    // Software-pipelined form (round 3, SWP): the products of stage t-1 and the cut of stage t share an iteration, so a plane slot is
    // read one iteration after it landed: the plane ring is three slots again (24 + 9 TN KB per workgroup; this form runs two
    // workgroups per CU on registers — 200-250 VGPRs — anyway, 2 x 69 KB fits).
    constexpr bool SWP = X6 == 3 && RED == 0 && MNY_W6_SWP != 0;
    constexpr int SB = X6 == 3 ? (SWP ? 3 : 2) : S;
    constexpr int NA_W = NA / 4;                                              // A instructions per wave: slots [0, NA_W) are A, the rest B
    static_assert(NA % 4 == 0 && NA_W < LPW, "slot split");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const sA = smem;
    float* const sB = smem + S * A_ST;
    float* sScale = sB + SB * B_ST;

    // block -> (m-run x, n-tile y): the n_tiles blocks of one m-run are consecutive within one XCD
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int y = local % p.n_tiles, x = (local / p.n_tiles) * 8 + xcd;
    if (x >= p.gx) return;
    const int n0 = y * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, khalf = lane >> 5;
    const int swz = (lrow >> 2) & 3;
    const int nk = (p.K + BKE - 1) / BKE;
    const int Kpad = nk * BKE;
    float* sShift = sScale + Kpad;
    const float slope = act_slope(p.in_act), hi = act_hi(p.in_act);
    if (XF != 0) {
        const bool has_xf = p.in_scale != nullptr;
        for (int k = tid; k < Kpad; k += 256) {
            sScale[k] = (k < p.K) ? (has_xf ? p.in_scale[k] : 1.f) : 0.f;
            sShift[k] = (k < p.K && has_xf) ? p.in_shift[k] : 0.f;
        }
    }
    const int mt_begin = x * p.tiles_per_block;
    const int mt_end = min(mt_begin + p.tiles_per_block, p.m_tiles);
    const int total = (mt_end - mt_begin) * nk;

    // DMA instruction j (wave-uniform, j = wv + 4i) covers tile rows 16j..16j+15, 4 lanes per row.  Per-lane state is kept
    // to the minimum — the row-in-group, ONE swizzled chunk offset (the swizzle depends on row & 15 only) and the B row
    // pointers; everything else is scalar.  (Per-instruction row/offset arrays pushed the TN >= 3 kernels over the
    // 168-VGPR budget of 3 waves/SIMD and the main loop spilled to scratch.)
    const int drow = lane >> 2;
    const int dk = ((lane & 3) ^ ((drow >> 2) & 3)) * EPC;       // swizzled source chunk, in elements
    int d_lds[LPW], d_row0[LPW];
    bool d_isA[LPW];
    const T* d_bptr[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int j = wv + 4 * i;
        if (j >= NL) j = NL - 1;
        d_isA[i] = j < NA;                                        // (== i < NA_W: NA is a multiple of 4)
        d_row0[i] = (d_isA[i] ? j : j - NA) * 16;                 // scalar
        d_lds[i] = d_isA[i] ? j * 256 : (j - NA) * 256;           // scalar, relative to the slot of its own ring
        if constexpr (X6 == 3) {
            const int jb = d_isA[i] ? 0 : j - NA;                 // (plane, column block) of this instruction
            const int pl = jb / TN, u = jb - pl * TN;
            int n = n0 + u * 32 + (lane & 31);                    // LDS image of a (plane, column block): [k half][32 columns] 16-B chunks, lane-linear
            if (n >= p.N) n = p.N - 1;
            d_lds[i] = d_isA[i] ? j * 256 : jb * 256;
            d_bptr[i] = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p.B) + ((int64_t)pl * p.N + n) * nk * 32 + (lane >> 5) * 16);
        } else {
            int n = n0 + d_row0[i] + drow;
            if (n >= p.N) n = p.N - 1;
            d_bptr[i] = pB + (int64_t)n * p.K + dk;
        }
    }
    const T* zero_src = reinterpret_cast<const T*>(&mny_zero16);
    const bool ragged_k = (p.K % BKE) != 0;

    // Running DMA sources (round 3): one pointer per slot, advanced by one k-stage per issue and re-seated when the flat walk enters a
    // new M tile.  The first cut recomputed every source from (tile, k-tile) per instruction — a 64-bit multiply-add, clamps and a
    // wave-uniform A / B branch per DMA instruction: ~30 vector + ~20 scalar instructions and 4-6 branches per stage in a loop whose
    // waves are latency-bound; now a stage's issue is LPW pointer bumps.
    const T* d_cur[LPW];
    int d_step[LPW];                                              // elements of T per k-stage (wave-uniform)
#pragma unroll
    for (int i = 0; i < LPW; ++i) d_step[i] = d_isA[i] ? BKE : (X6 == 3 ? 32 / (int)sizeof(T) : BKE);
    auto seat = [&](int mt) {                                     // sources of stage (mt, k-tile 0)
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            if (d_isA[i]) {
                int m = mt * BM + d_row0[i] + drow;
                if (m >= (int)p.M) m = (int)p.M - 1;
                d_cur[i] = pA + (int64_t)m * p.K + dk;
            } else {
                d_cur[i] = d_bptr[i];
            }
        }
    };
    auto issue_part = [&](int kt, float* stage, int i0, int i1) {  // slots [i0, i1) of this wave into `stage` (a slot of the A or the B ring)
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            if (i < i0 || i >= i1) continue;
            const T* src = d_cur[i];
            if (ragged_k) {                                       // kernel-uniform; K % 16 != 0 only
                const bool kout = kt == nk - 1 && kt * BKE + dk >= p.K;      // this lane's chunk lies past K
                if (kout) src = d_isA[i] ? d_cur[i] - (kt * BKE + dk) : (X6 == 3 ? src : zero_src);   // A: finite filler (row start), annihilated by zero B / zero scale
            }
            d_cur[i] += d_step[i];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(stage + d_lds[i]), 16, 0, 0);
        }
    };
    auto issue_a = [&](int kt, int slot) { issue_part(kt, sA + slot * A_ST, 0, NA_W); };
    auto issue_b = [&](int kt, int slot) { issue_part(kt, sB + slot * B_ST, NA_W, LPW); };

    f32x16 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float s1[TN], s2[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) { s1[t] = 0.f; s2[t] = 0.f; }

    auto compute = [&](int kt, int slot, int slot_b) {
        const float* stA = sA + slot * A_ST;
        const float* stB = sB + slot_b * B_ST;
        const float* a_row = stA + (wv * 32 + lrow) * BKD;
        if constexpr (BF != 0) {
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                const int chunk = kc * 2 + khalf;
                v4u_t au = lds_read_u4(a_row + ((chunk ^ swz) << 2));
                v4u_t bu[TN];
#pragma unroll
                for (int u = 0; u < TN; ++u) bu[u] = lds_read_u4(stB + (u * 32 + lrow) * BKD + ((chunk ^ swz) << 2));
                v4f_t sc0, sc1, sh0, sh1;
                if (XF != 0) {
                    const int kbase = kt * BKE + chunk * 8;
                    sc0 = lds_read_f4(sScale + kbase); sc1 = lds_read_f4(sScale + kbase + 4);
                    sh0 = lds_read_f4(sShift + kbase); sh1 = lds_read_f4(sShift + kbase + 4);
                }
                MNY_LGKM_WAIT(au);
#pragma unroll
                for (int u = 0; u < TN; ++u) MNY_LGKM_DEP(bu[u]);
                if (XF != 0) {
                    MNY_LGKM_DEP(sc0); MNY_LGKM_DEP(sc1); MNY_LGKM_DEP(sh0); MNY_LGKM_DEP(sh1);
                    float z[8] = {__uint_as_float(au.x << 16), __uint_as_float(au.x & 0xffff0000u), __uint_as_float(au.y << 16),
                                  __uint_as_float(au.y & 0xffff0000u), __uint_as_float(au.z << 16), __uint_as_float(au.z & 0xffff0000u),
                                  __uint_as_float(au.w << 16), __uint_as_float(au.w & 0xffff0000u)};
                    const float scv[8] = {sc0.x, sc0.y, sc0.z, sc0.w, sc1.x, sc1.y, sc1.z, sc1.w};
                    const float shv[8] = {sh0.x, sh0.y, sh0.z, sh0.w, sh1.x, sh1.y, sh1.z, sh1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float zz = fmaf(z[e], scv[e], shv[e]);
                        z[e] = XF == 1 ? __builtin_amdgcn_fmed3f(zz, slope * zz, hi) : zz * __builtin_amdgcn_fmed3f(zz + 3.f, 0.f, 6.f) * (1.f / 6.f);
                    }
                    au = v4u_t{pack_bf16x2(z[0], z[1]), pack_bf16x2(z[2], z[3]), pack_bf16x2(z[4], z[5]), pack_bf16x2(z[6], z[7])};
                }
                const bf16x8_t a8 = __builtin_bit_cast(bf16x8_t, au);
#pragma unroll
                for (int u = 0; u < TN; ++u)
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, __builtin_bit_cast(bf16x8_t, bu[u]), acc[u], 0, 0, 0);
            }
            return;
        }
        if constexpr (X6 != 0) {
            // the lane's eight k-values of this stage: chunks khalf and 2 + khalf (the same two the fp32 path reads one after the other)
            const int c0 = khalf, c1 = 2 + khalf;
            v4f_t a0 = lds_read_f4(a_row + ((c0 ^ swz) << 2)), a1 = lds_read_f4(a_row + ((c1 ^ swz) << 2));
            v4f_t b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;          // (never a copy of a0: its register is still in flight here)
            if constexpr (X6 != 3) { b0 = lds_read_f4(stB + lrow * BKD + ((c0 ^ swz) << 2)); b1 = lds_read_f4(stB + lrow * BKD + ((c1 ^ swz) << 2)); }
            v4f_t sc0, sc1, sh0, sh1;
            if (XF != 0) {
                sc0 = lds_read_f4(sScale + kt * BKD + c0 * 4); sc1 = lds_read_f4(sScale + kt * BKD + c1 * 4);
                sh0 = lds_read_f4(sShift + kt * BKD + c0 * 4); sh1 = lds_read_f4(sShift + kt * BKD + c1 * 4);
            }
            MNY_LGKM_WAIT(a0);
            MNY_LGKM_DEP(a1); MNY_LGKM_DEP(b0); MNY_LGKM_DEP(b1);
            if (XF != 0) {
                MNY_LGKM_DEP(sc0); MNY_LGKM_DEP(sc1); MNY_LGKM_DEP(sh0); MNY_LGKM_DEP(sh1);
                float z[8] = {fmaf(a0.x, sc0.x, sh0.x), fmaf(a0.y, sc0.y, sh0.y), fmaf(a0.z, sc0.z, sh0.z), fmaf(a0.w, sc0.w, sh0.w),
                              fmaf(a1.x, sc1.x, sh1.x), fmaf(a1.y, sc1.y, sh1.y), fmaf(a1.z, sc1.z, sh1.z), fmaf(a1.w, sc1.w, sh1.w)};
#pragma unroll
                for (int e = 0; e < 8; ++e) z[e] = XF == 1 ? __builtin_amdgcn_fmed3f(z[e], slope * z[e], hi) : z[e] * __builtin_amdgcn_fmed3f(z[e] + 3.f, 0.f, 6.f) * (1.f / 6.f);
                a0 = v4f_t{z[0], z[1], z[2], z[3]}; a1 = v4f_t{z[4], z[5], z[6], z[7]};
            }
            bf16x8_t ah, am, al;
            x6_split(a0, a1, ah, am, al);
            if constexpr (X6 == 3) {
                const float* src0 = stB + (khalf * 32 + lrow) * 4;
                v4f_t ph = lds_read_f4(src0), pm = lds_read_f4(src0 + TN * 256), pl = lds_read_f4(src0 + 2 * TN * 256);
                MNY_LGKM_WAIT(ph); MNY_LGKM_DEP(pm); MNY_LGKM_DEP(pl);
#pragma unroll
                for (int u = 0; u < TN; ++u) {
                    v4f_t nh, nm, nl;
                    if (u + 1 < TN) {                             // the next column block's pieces are requested before this one's MFMAs
                        const float* src = stB + ((u + 1) * 64 + khalf * 32 + lrow) * 4;
                        nh = lds_read_f4(src); nm = lds_read_f4(src + TN * 256); nl = lds_read_f4(src + 2 * TN * 256);
                    }
                    const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, ph), bm = __builtin_bit_cast(bf16x8_t, pm), bl = __builtin_bit_cast(bf16x8_t, pl);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[u], 0, 0, 0);
                    if (u + 1 < TN) { MNY_LGKM_WAIT(nh); MNY_LGKM_DEP(nm); MNY_LGKM_DEP(nl); ph = nh; pm = nm; pl = nl; }
                }
                return;
            }
#pragma unroll
            for (int u = 0; u < TN; ++u) {
                v4f_t n0, n1;
                if (u + 1 < TN) {                                 // next column block's fragment is requested before this one's MFMAs
                    n0 = lds_read_f4(stB + ((u + 1) * 32 + lrow) * BKD + ((c0 ^ swz) << 2));
                    n1 = lds_read_f4(stB + ((u + 1) * 32 + lrow) * BKD + ((c1 ^ swz) << 2));
                }
                bf16x8_t bh, bm, bl;
                x6_split(b0, b1, bh, bm, bl);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[u], 0, 0, 0);      // small terms first
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[u], 0, 0, 0);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[u], 0, 0, 0);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[u], 0, 0, 0);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[u], 0, 0, 0);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[u], 0, 0, 0);
                if (u + 1 < TN) { MNY_LGKM_WAIT(n0); MNY_LGKM_DEP(n1); b0 = n0; b1 = n1; }
            }
            return;
        }
#pragma unroll
        for (int kc = 0; kc < BKD / 8; ++kc) {
            const int chunk = kc * 2 + khalf;
            v4f_t af = lds_read_f4(a_row + ((chunk ^ swz) << 2));
            v4f_t bf[TN];
#pragma unroll
            for (int u = 0; u < TN; ++u) bf[u] = lds_read_f4(stB + (u * 32 + lrow) * BKD + ((chunk ^ swz) << 2));
            v4f_t sc, sh;
            if (XF != 0) {
                const int kbase = kt * BKD + chunk * 4;
                sc = lds_read_f4(sScale + kbase);
                sh = lds_read_f4(sShift + kbase);
            }
            MNY_LGKM_WAIT(af);
#pragma unroll
            for (int u = 0; u < TN; ++u) MNY_LGKM_DEP(bf[u]);
            if (XF != 0) {
                MNY_LGKM_DEP(sc);
                MNY_LGKM_DEP(sh);
                float z0 = fmaf(af.x, sc.x, sh.x), z1 = fmaf(af.y, sc.y, sh.y), z2 = fmaf(af.z, sc.z, sh.z), z3 = fmaf(af.w, sc.w, sh.w);
                if (XF == 1) {
                    af.x = fminf(fmaxf(z0, slope * z0), hi); af.y = fminf(fmaxf(z1, slope * z1), hi);
                    af.z = fminf(fmaxf(z2, slope * z2), hi); af.w = fminf(fmaxf(z3, slope * z3), hi);
                } else {
                    af.x = z0 * fminf(fmaxf(z0 + 3.f, 0.f), 6.f) * (1.f / 6.f); af.y = z1 * fminf(fmaxf(z1 + 3.f, 0.f), 6.f) * (1.f / 6.f);
                    af.z = z2 * fminf(fmaxf(z2 + 3.f, 0.f), 6.f) * (1.f / 6.f); af.w = z3 * fminf(fmaxf(z3 + 3.f, 0.f), 6.f) * (1.f / 6.f);
                }
            }
            // accumulators interleaved: consecutive MFMAs never depend on each other
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf[u].x, acc[u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf[u].y, acc[u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf[u].z, acc[u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf[u].w, acc[u], 0, 0, 0);
        }
    };

    // Epilogue.  The MFMA layout gives a lane one COLUMN (16 rows of it); storing that directly is 64 four-byte
    // stores per lane.  Instead each group of 4 accumulator registers (rows b..b+3 of the lane's column) is transposed
    // across the lane's quad with two DPP butterfly stages, after which lane jq of a quad holds row b+jq, columns
    // 4q..4q+3 -> one 16-byte store (4x fewer store instructions, full 128-B row segments per quad-row).
    const int quad = lrow >> 2, jq = lane & 3;
    const bool nvec = (p.N & 3) == 0;
    auto epilogue = [&](int mt) {
        const int64_t m0 = (int64_t)mt * BM;
#pragma unroll
        for (int u = 0; u < TN; ++u) {
            const int colq = n0 + u * 32 + quad * 4;              // first of this lane's 4 output columns
            const bool cok = colq < p.N;                          // N % 4 == 0: all four or none; ragged N: per element below
            float4 bv = f4zero();
            if (p.bias && cok) {
                if (nvec) bv = ld4(p.bias + colq);
                else {
                    bv.x = p.bias[colq];
                    if (colq + 1 < p.N) bv.y = p.bias[colq + 1];
                    if (colq + 2 < p.N) bv.z = p.bias[colq + 2];
                    if (colq + 3 < p.N) bv.w = p.bias[colq + 3];
                }
            }
            if (RED) {                                            // BN-backward sums of the unit this gradient belongs to
                const int col = n0 + u * 32 + lrow;
                const bool ccol = col < p.N;
                const int cc = ccol ? col : 0;
                const float rsc = p.r_scale[cc], rsh = p.r_shift[cc], rmu = p.r_mean[cc], ris = p.r_invstd[cc];
                float rbias = 0.f;                                // (mny_pw_lr_fix: the gradient carries a per-column constant; data gradients have none)
                if constexpr (RB != 0) rbias = p.bias[cc];
                const float rslope = act_slope(p.r_act), rhi = act_hi(p.r_act);
                const int64_t rbase = m0 + wv * 32 + 4 * khalf;
                const int rows_left = (int)max((int64_t)0, min((int64_t)64, p.M - rbase));   // rows rbase + 8*gq + j, 8*gq + j < rows_left, exist
                const T* ybase = (const T*)p.rY + (rows_left > 0 ? rbase : 0) * p.N + cc;
                const T* abase = RED == 2 ? pAdd + (rows_left > 0 ? rbase : 0) * p.N + cc : nullptr;   // RED = 2: earlier contributions to the same gradient
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {                  // four rows at a time: the loads of a group are all that is in flight
                    float yv[4], av[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) yv[j] = ld1(ybase + (ccol && 8 * gq + j < rows_left ? 8 * gq + j : 0) * p.N);
                    if (RED == 2) {                               // the sums are over the COMPLETE gradient = product + addend
#pragma unroll
                        for (int j = 0; j < 4; ++j) av[j] = ld1(abase + (ccol && 8 * gq + j < rows_left ? 8 * gq + j : 0) * p.N);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float z = fmaf(yv[j], rsc, rsh);
                        const float dact = p.r_act >= MNY_ACT_HSWISH ? act_bwd(z, p.r_act) : (z > 0.f ? 1.f : rslope) * (z < rhi ? 1.f : 0.f);
                        const float dz = stored<T>(RB != 0 ? acc[u][gq * 4 + j] + rbias + av[j] : acc[u][gq * 4 + j] + av[j]) * dact;
                        if (ccol && 8 * gq + j < rows_left) { s1[u] += dz; s2[u] = fmaf(dz, (yv[j] - rmu) * ris, s2[u]); }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if (p.stats) {                                 // column sums come from the un-transposed registers
                const bool ccol = n0 + u * 32 + lrow < p.N;
                if (m0 + BM <= p.M) {                             // whole tile inside M (all but the last one): packed pairs, no row tests
                    v2f a1 = v2f{0.f, 0.f}, a2 = v2f{0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const v2f q = v2f{stored<T>(acc[u][r]), stored<T>(acc[u][r + 1])};
                        a1 += q;
                        a2 = __builtin_elementwise_fma(q, q, a2);
                    }
                    if (ccol) { s1[u] += a1.x + a1.y; s2[u] += a2.x + a2.y; }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t row = m0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                        const float q = stored<T>(acc[u][r]);
                        if (ccol && row < p.M) { s1[u] += q; s2[u] = fmaf(q, q, s2[u]); }
                    }
                }
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float r0 = acc[u][gq * 4 + 0], r1 = acc[u][gq * 4 + 1], r2 = acc[u][gq * 4 + 2], r3 = acc[u][gq * 4 + 3];
                {   // stage A: exchange with lane^1 inside the quad
                    const bool odd = lane & 1;
                    const float xa = odd ? r0 : r1, xb = odd ? r2 : r3;
                    const float ya = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xa), 0xB1, 0xF, 0xF, true));
                    const float yb = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xb), 0xB1, 0xF, 0xF, true));
                    if (odd) { r0 = ya; r2 = yb; } else { r1 = ya; r3 = yb; }
                }
                {   // stage B: exchange with lane^2
                    const bool hi2 = lane & 2;
                    const float xa = hi2 ? r0 : r2, xb = hi2 ? r1 : r3;
                    const float ya = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xa), 0x4E, 0xF, 0xF, true));
                    const float yb = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xb), 0x4E, 0xF, 0xF, true));
                    if (hi2) { r0 = ya; r1 = yb; } else { r2 = ya; r3 = yb; }
                }
                const int64_t row = m0 + wv * 32 + 8 * gq + 4 * khalf + jq;
                if (cok && row < p.M) {
                    float4 v = make_float4(r0, r1, r2, r3);
                    if (p.bias) { v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w; }        // wave-uniform: only the two head convs carry a bias
                    if (nvec) {
                        if (pAdd) add4(v, ld4(pAdd + row * p.N + colq));
                        // a row of this 32-column tile is 128 contiguous bytes in fp32 (whole lines: streaming stores) but 64 in bf16 storage: non-temporal
                        // PARTIAL lines cost DRAM efficiency (round 5: MobileNetV3 512x512 bs 64 bf16 14.05 -> 13.91 ms with plain stores, same box)
                        if (sizeof(T) == 2) st4(pC + row * p.N + colq, v); else st4_stream(pC + row * p.N + colq, v);
                    } else {
                        // ragged width (75-channel heads, 10-channel gate): rows are not 16-B aligned -> up to four element stores
                        // off ONE address (the transposed layout keeps this cheap: one row, consecutive columns)
                        T* dst = pC + row * p.N + colq;
                        const T* ad = pAdd ? pAdd + row * p.N + colq : nullptr;
                        st1(dst, v.x + (ad ? ld1(ad) : 0.f));
                        if (colq + 1 < p.N) st1(dst + 1, v.y + (ad ? ld1(ad + 1) : 0.f));
                        if (colq + 2 < p.N) st1(dst + 2, v.z + (ad ? ld1(ad + 2) : 0.f));
                        if (colq + 3 < p.N) st1(dst + 3, v.w + (ad ? ld1(ad + 3) : 0.f));
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[u][gq * 4 + i] = 0.f;
                // keep the 4*TN store groups sequential: letting the scheduler hoist every addend load / transpose ahead of
                // the first store raised the kernel's peak VGPR demand by ~27 and made the TN >= 3 main loops spill
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // flat (tile, k-tile) walk; stage t lives in ring slot t % 3, two stages stay in flight behind the consumer
    int c_mt = mt_begin, c_kt = 0, c_slot = 0, c_slot_b = 0;           // stage being consumed
    auto consume = [&]() {
        compute(c_kt, c_slot, X6 != 3 ? c_slot : c_slot_b);
        if (++c_kt == nk) { epilogue(c_mt); c_kt = 0; ++c_mt; }
        if (++c_slot == S) c_slot = 0;
        c_slot_b ^= 1;
    };
    if constexpr (X6 != 3) {
        int i_mt = mt_begin, i_kt = 0, i_slot = 0;       // next stage to issue
        seat(mt_begin);
        auto issue_next = [&]() {
            issue_a(i_kt, i_slot); issue_b(i_kt, i_slot);
            if (++i_kt == nk) { i_kt = 0; ++i_mt; if (i_mt < mt_end) seat(i_mt); }
            if (++i_slot == S) i_slot = 0;
        };
        const int pre = total < S - 1 ? total : S - 1;
        for (int t = 0; t < pre; ++t) issue_next();
        const int steady = total - pre;                      // steps that still have a stage to issue
        for (int t = 0; t < steady; ++t) {
            wait_vmcnt<LPW*(S - 2)>();                       // my share of the oldest stage has landed
            __builtin_amdgcn_s_barrier();                    // ... for every wave; the slot refilled below is fully consumed
            issue_next();
            consume();
        }
        for (int t = 0; t < pre; ++t) {                      // drain
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            consume();
        }
    } else if constexpr (SWP) {
        // ---- planes mode, software-pipelined -------------------------------------------------------------------------------------
        // Measured on the one-stage-at-a-time form (profiles/r03_pmc_step.txt, ISA): per k-stage a wave issues ~110 vector-ALU
        // instructions (LDS addresses, BN-apply + activation of the A fragment, the three-way cut) BEFORE its 6 TN MFMAs, back to back —
        // ~450 cycles in which it feeds the matrix pipe nothing; SQ_VALU_MFMA_BUSY 40-44 % on the fat shapes.  Here iteration t cuts
        // stage t while the products of stage t-1 issue: the cut is split into 24 pieces of 2-4 instructions and one piece follows each
        // MFMA (an 8-pass MFMA occupies the pipe for 32 cycles, a piece issues in 8-16), LDS reads carry their offsets as immediates.
        // Same products in the same order per accumulator as the one-at-a-time form: bit-identical results.
        // Measured (tools/ab/w6_bench.py, same box): 512x512 at 22x22 0.499 -> 0.464 ms (130 -> 140 TF/s), K960 N160 -12 %, K576 N96 -9 %,
        // K1280 N512 -6 %.  What it did NOT fix: the kernel is not bound by any one thing — timing builds with a part removed give, for
        // 512x512: no plane DMA -18 %, no plane LDS reads -17 %, no A DMA -9 %, no cut -7 %, no barrier / vmcnt wait -5 %, all of them
        // together 0.27 ms (the MFMAs + epilogue alone, 57 % of the bf16 peak / 6).  Issuing the DMA pieces between the MFMAs, requesting
        // the next stage's first planes a stage ahead and the size of the accumulator group (2 / 4) all measured neutral.  The plane
        // traffic (12 KB of DMA per stage per workgroup, 12 KB of LDS reads per stage per WAVE) is the largest single share.  The 64-row
        // wave tile that halves it per FLOP (two row blocks share each plane read and DMA: 256 x 128 workgroup tile, 128 accumulators
        // pinned to accumulation registers, 84 KB of LDS, hence ONE wave per SIMD) was built on this scaffold and measured: 512x512
        // 0.47 -> 0.55 ms, K1280 N512 0.29 -> 0.34 — a lone wave per SIMD exposes every barrier, vmcnt and LDS round trip that the
        // second wave covers here; removed again.
        int a_mt = mt_begin, a_kt = 0, a_slot = 0, a_n = 0;   // next A stage to issue
        int b_mt = mt_begin, b_kt = 0, b_slot = 0, b_n = 0;   // next B stage to issue
        auto seat_part = [&](int mt, bool part_a) {
#pragma unroll
            for (int i = 0; i < LPW; ++i) {
                if ((i < NA_W) != part_a) continue;
                if (part_a) {
                    int m = mt * BM + d_row0[i] + drow;
                    if (m >= (int)p.M) m = (int)p.M - 1;
                    d_cur[i] = pA + (int64_t)m * p.K + dk;
                } else {
                    d_cur[i] = d_bptr[i];
                }
            }
        };
        seat_part(mt_begin, true); seat_part(mt_begin, false);
        auto next_a = [&]() {
            issue_a(a_kt, a_slot); ++a_n;
            if (++a_kt == nk) { a_kt = 0; ++a_mt; if (a_mt < mt_end) seat_part(a_mt, true); }
            if (++a_slot == S) a_slot = 0;
        };
        auto next_b = [&]() {
            issue_b(b_kt, b_slot); ++b_n;
            if (++b_kt == nk) { b_kt = 0; ++b_mt; if (b_mt < mt_end) seat_part(b_mt, false); }
            if (++b_slot == SB) b_slot = 0;
        };
        // loop-invariant LDS byte addresses of the lane
        const unsigned oA0 = lds_off(sA + (wv * 32 + lrow) * BKD + ((khalf ^ swz) << 2));
        const unsigned oA1 = lds_off(sA + (wv * 32 + lrow) * BKD + (((2 + khalf) ^ swz) << 2));
        const unsigned oB = lds_off(sB + lane * 4);
        const unsigned oS = lds_off(sScale + khalf * 4);
        const unsigned shift_off = (unsigned)Kpad * 4u;
        bf16x8_t qh, qm, ql;                                  // the cut A fragment whose products come next
        int p_kt = 0, p_slot = 0;                             // stage being cut
        int m_slot_b = 0;                                     // plane slot of the stage being multiplied (its tile / k-tile: c_mt, c_kt)
        auto step = [&](auto prep_c, auto mma_c) -> bool {
            constexpr bool PREP = decltype(prep_c)::value, MMA = decltype(mma_c)::value;
            constexpr int NPIECE = 24, NISSUE = MMA ? 6 * TN : 1;
            v4f_t a0, a1, sc0, sc1, sh0, sh1;
            float z[8];
            v2f r1[4], r2[4];
            v4u_t nhu, nmu, nlu;
            auto piece = [&](auto pc) {
                constexpr int P = decltype(pc)::value;
                if constexpr (PREP) {
                    if constexpr (P < 8) {                            // element P: BN-apply + activation of the producer
                        const float av = P < 4 ? a0[P & 3] : a1[P & 3];
                        if constexpr (XF != 0) {
                            const float zz = fmaf(av, P < 4 ? sc0[P & 3] : sc1[P & 3], P < 4 ? sh0[P & 3] : sh1[P & 3]);
                            z[P] = XF == 1 ? __builtin_amdgcn_fmed3f(zz, slope * zz, hi) : zz * __builtin_amdgcn_fmed3f(zz + 3.f, 0.f, 6.f) * (1.f / 6.f);
                        } else {
                            z[P] = av;
                        }
                        asm volatile("" : "+v"(z[P]));               // pins the piece HERE (values used only by the next iteration are otherwise sunk below the MFMAs)
                    } else if constexpr (P < 16) {                    // three-way cut of the pair (2i, 2i+1), in two halves (x6_split's arithmetic)
                        constexpr int i = (P - 8) >> 1;
                        if constexpr (((P - 8) & 1) == 0) {
                            const v2f a = v2f{z[2 * i], z[2 * i + 1]};
                            const v2f ah = v2f{__uint_as_float(__float_as_uint(a.x) & 0xffff0000u), __uint_as_float(__float_as_uint(a.y) & 0xffff0000u)};
                            r1[i] = a - ah;
                            asm volatile("" : "+v"(r1[i]));
                        } else {
                            const v2f b = r1[i];
                            const v2f bh = v2f{__uint_as_float(__float_as_uint(b.x) & 0xffff0000u), __uint_as_float(__float_as_uint(b.y) & 0xffff0000u)};
                            r2[i] = b - bh;
                            asm volatile("" : "+v"(r2[i]));
                        }
                    } else if constexpr (P < 22) {                    // pack the high halves: two dwords per piece
                        constexpr int q = P - 16, w = q >> 1, d = (q & 1) * 2;
                        auto pk = [](float lo, float hi_) { return __builtin_amdgcn_perm(__float_as_uint(hi_), __float_as_uint(lo), 0x07060302u); };
                        unsigned t0, t1;
                        if constexpr (w == 0) { t0 = pk(z[2 * d], z[2 * d + 1]); t1 = pk(z[2 * d + 2], z[2 * d + 3]); }
                        if constexpr (w == 1) { t0 = pk(r1[d].x, r1[d].y); t1 = pk(r1[d + 1].x, r1[d + 1].y); }
                        if constexpr (w == 2) { t0 = pk(r2[d].x, r2[d].y); t1 = pk(r2[d + 1].x, r2[d + 1].y); }
                        asm volatile("" : "+v"(t0), "+v"(t1));
                        if constexpr (w == 0) { nhu[d] = t0; nhu[d + 1] = t1; }
                        if constexpr (w == 1) { nmu[d] = t0; nmu[d + 1] = t1; }
                        if constexpr (w == 2) { nlu[d] = t0; nlu[d + 1] = t1; }
                    }
                }
            };
            auto pieces_of = [&](auto ic) {                           // the pieces that follow issue point I
                constexpr int I = decltype(ic)::value;
                static_for<0, NPIECE>([&](auto pc) {
                    constexpr int P = decltype(pc)::value;
                    if constexpr (P * NISSUE / NPIECE == I) piece(pc);
                });
            };
            if constexpr (!MMA) {                                     // first stage of the walk: nothing to multiply yet
                const unsigned bA = (unsigned)p_slot * (A_ST * 4);
                a0 = lds_read_f4_at<0>(oA0 + bA); a1 = lds_read_f4_at<0>(oA1 + bA);
                if constexpr (XF != 0) {
                    const unsigned bS = oS + (unsigned)p_kt * (BKD * 4), bH = bS + shift_off;
                    sc0 = lds_read_f4_at<0>(bS); sc1 = lds_read_f4_at<32>(bS); sh0 = lds_read_f4_at<0>(bH); sh1 = lds_read_f4_at<32>(bH);
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(sc0), "+v"(sc1), "+v"(sh0), "+v"(sh1));
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1));
                }
                pieces_of(std::integral_constant<int, 0>{});
            } else {
                // Column blocks in GROUPS of up to four (MNY_W6_GROUP; TN = 5: 3 + 2): product k is issued for every block of the group before
                // product k+1, so an MFMA's predecessor on the same accumulator is `group size` issues back (the pairs form left 38 % of the
                // wave cycles in issue stalls with the pipe 58 % idle: dependent issues).  A group's planes are requested up front in the
                // order the products need them — high, (the cut's operands), low, mid — and waited for with counted lgkmcnt.
                const unsigned bB = oB + (unsigned)m_slot_b * (B_ST * 4);
                v4f_t PH[TN], PM[TN], PL[TN];
                constexpr int NPREP = PREP ? (XF != 0 ? 6 : 2) : 0;  // LDS reads of the cut
                constexpr int G0 = TN <= MNY_W6_GROUP ? TN : (TN + 1) / 2;     // size of the first group (TN = 5 -> 3 + 2)
                auto rdH = [&](auto uc) { constexpr int u = decltype(uc)::value; PH[u] = lds_read_f4_at<u * 1024>(bB); };
                auto rdM = [&](auto uc) { constexpr int u = decltype(uc)::value; PM[u] = lds_read_f4_at<(TN + u) * 1024>(bB); };
                auto rdL = [&](auto uc) { constexpr int u = decltype(uc)::value; PL[u] = lds_read_f4_at<(2 * TN + u) * 1024>(bB); };
                auto tie = [&](auto uc, v4f_t* P_) { constexpr int u = decltype(uc)::value; asm volatile("" : "+v"(P_[u])); };
                auto group = [&](auto u0c, auto gsc, auto firstc) {
                    constexpr int u0 = decltype(u0c)::value, gs = decltype(gsc)::value;
                    constexpr bool first = decltype(firstc)::value;
                    constexpr bool more = u0 + gs < TN;              // a second group follows (its planes are requested before this group's third product)
                    constexpr int I0 = 6 * u0;
                    if constexpr (first) {
                        static_for<u0, u0 + gs>(rdH);
                        if constexpr (PREP) {
                            const unsigned bA = (unsigned)p_slot * (A_ST * 4);
                            a0 = lds_read_f4_at<0>(oA0 + bA); a1 = lds_read_f4_at<0>(oA1 + bA);
                            if constexpr (XF != 0) {
                                const unsigned bS = oS + (unsigned)p_kt * (BKD * 4), bH = bS + shift_off;
                                sc0 = lds_read_f4_at<0>(bS); sc1 = lds_read_f4_at<32>(bS); sh0 = lds_read_f4_at<0>(bH); sh1 = lds_read_f4_at<32>(bH);
                            }
                        }
                        static_for<u0, u0 + gs>(rdL);
                        static_for<u0, u0 + gs>(rdM);
                        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(NPREP + 2 * gs) : "memory");      // high planes landed
                        static_for<u0, u0 + gs>([&](auto uc) { tie(uc, PH); });
                    } else {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                             // requested during the first group
                        static_for<u0, u0 + gs>([&](auto uc) { tie(uc, PH); tie(uc, PL); tie(uc, PM); });
                    }
                    auto prod = [&](auto kc, const bf16x8_t& A_, v4f_t* P_) {
                        constexpr int k = decltype(kc)::value;
                        static_for<0, gs>([&](auto jc) {
                            constexpr int j = decltype(jc)::value, u = u0 + j, IA = I0 + k * gs + j;
                            acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A_, __builtin_bit_cast(bf16x8_t, P_[u]), acc[u], 0, 0, 0);
                            if constexpr (PREP && first && k == 0 && j == 0) {     // the cut's operands: queued behind the high planes
                                if constexpr (XF != 0) asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a0), "+v"(a1), "+v"(sc0), "+v"(sc1), "+v"(sh0), "+v"(sh1) : "n"(2 * gs));
                                else asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a0), "+v"(a1) : "n"(2 * gs));
                            }
                            pieces_of(std::integral_constant<int, IA>{});
                            __builtin_amdgcn_sched_barrier(0);
                        });
                    };
                    prod(std::integral_constant<int, 0>{}, ql, PH);                // small terms first (the order of the one-at-a-time form)
                    if constexpr (first) {
                        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(gs) : "memory");               // low planes landed
                        static_for<u0, u0 + gs>([&](auto uc) { tie(uc, PL); });
                    }
                    prod(std::integral_constant<int, 1>{}, qh, PL);
                    if constexpr (first) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                          // mid planes landed
                        static_for<u0, u0 + gs>([&](auto uc) { tie(uc, PM); });
                        if constexpr (more) { static_for<u0 + gs, TN>(rdH); static_for<u0 + gs, TN>(rdL); static_for<u0 + gs, TN>(rdM); }
                    }
                    prod(std::integral_constant<int, 2>{}, qm, PM);
                    prod(std::integral_constant<int, 3>{}, qm, PH);
                    prod(std::integral_constant<int, 4>{}, qh, PM);
                    prod(std::integral_constant<int, 5>{}, qh, PH);
                };
                group(std::integral_constant<int, 0>{}, std::integral_constant<int, G0>{}, std::true_type{});
                if constexpr (G0 < TN) group(std::integral_constant<int, G0>{}, std::integral_constant<int, TN - G0>{}, std::false_type{});
            }
            bool fin = false;
            if constexpr (MMA) {
                if (++c_kt == nk) { c_kt = 0; fin = true; }
                if (++m_slot_b == SB) m_slot_b = 0;
            }
            if constexpr (PREP) {
                qh = __builtin_bit_cast(bf16x8_t, nhu); qm = __builtin_bit_cast(bf16x8_t, nmu); ql = __builtin_bit_cast(bf16x8_t, nlu);
                if (++p_kt == nk) p_kt = 0;
                if (++p_slot == S) p_slot = 0;
            }
            return fin;
        };
        if (total > 0) { next_a(); next_b(); }               // A(0), B(0), then A(1): the order the counted wait below assumes
        if (total > 1) next_a();
        if (total > 0) {                                     // (three separate code paths, not one loop with a three-way branch: the accumulators
            wait_vmcnt<NA_W>();                              //  then merge only at the loop header and are not copied per iteration)
            if (total == 1) wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();                    // A(0), B(0) landed
            if (b_n < total) next_b();                       // B(1)
            if (a_n < total) next_a();                       // A(2)
            step(std::true_type{}, std::false_type{});
            for (int t = 1; t < total; ++t) {
                if (t + 1 < total) wait_vmcnt<NA_W>(); else wait_vmcnt<0>();     // A(t), B(t) landed; A(t+1) may still be in flight
                __builtin_amdgcn_s_barrier();                // every wave has cut stage t-1 and multiplied stage t-2: A slot (t+2) % 3, B slot (t+1) % 3 are free
                if (b_n < total) next_b();                   // B(t+1)
                if (a_n < total) next_a();                   // A(t+2)
                if (step(std::true_type{}, std::true_type{})) { epilogue(c_mt); ++c_mt; }
            }
            step(std::false_type{}, std::true_type{});
            epilogue(c_mt);
        }
    } else {
        // planes mode: A two stages ahead (3 slots), B one stage ahead (2 slots).  The A and the B sources walk the same (tile, k-tile)
        // sequence with their own cursors; issue order inside an iteration is B(t+1) THEN A(t+2), so that at the top of iteration t+1 the
        // in-order counter may leave exactly A(t+2)'s NA_W instructions outstanding: everything older — A(t+1), B(t+1) — has landed.
        int a_mt = mt_begin, a_kt = 0, a_slot = 0, a_n = 0;   // next A stage to issue
        int b_mt = mt_begin, b_kt = 0, b_slot = 0, b_n = 0;   // next B stage to issue
        auto seat_part = [&](int mt, bool part_a) {
#pragma unroll
            for (int i = 0; i < LPW; ++i) {
                if ((i < NA_W) != part_a) continue;
                if (part_a) {
                    int m = mt * BM + d_row0[i] + drow;
                    if (m >= (int)p.M) m = (int)p.M - 1;
                    d_cur[i] = pA + (int64_t)m * p.K + dk;
                } else {
                    d_cur[i] = d_bptr[i];
                }
            }
        };
        seat_part(mt_begin, true); seat_part(mt_begin, false);
        auto next_a = [&]() {
            issue_a(a_kt, a_slot); ++a_n;
            if (++a_kt == nk) { a_kt = 0; ++a_mt; if (a_mt < mt_end) seat_part(a_mt, true); }
            if (++a_slot == S) a_slot = 0;
        };
        auto next_b = [&]() {
            issue_b(b_kt, b_slot); ++b_n;
            if (++b_kt == nk) { b_kt = 0; ++b_mt; if (b_mt < mt_end) seat_part(b_mt, false); }
            b_slot ^= 1;
        };
        if (total > 0) { next_a(); next_b(); }               // A(0), B(0), then A(1): the order the counted wait below assumes
        if (total > 1) next_a();
        for (int t = 0; t < total; ++t) {
            if (t + 1 < total) wait_vmcnt<NA_W>(); else wait_vmcnt<0>();     // A(t), B(t) landed; A(t+1) may still be in flight
            __builtin_amdgcn_s_barrier();                    // every wave is past stage t-1: B slot (t+1) % 2 and A slot (t+2) % 3 are free
            if (b_n < total) next_b();                       // B(t+1)
            if (a_n < total) next_a();                       // A(t+2)
            consume();
        }
    }

    if (p.stats) {
        wait_vmcnt<0>();
        __syncthreads();
        float* red = smem;   // [4][BN][2]
#pragma unroll
        for (int u = 0; u < TN; ++u) {
            const float a = s1[u] + __shfl_xor(s1[u], 32);
            const float b = s2[u] + __shfl_xor(s2[u], 32);
            if (khalf == 0) {
                red[(wv * BN + u * 32 + lrow) * 2 + 0] = a;
                red[(wv * BN + u * 32 + lrow) * 2 + 1] = b;
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < p.N) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { a += red[(w * BN + tid) * 2]; b += red[(w * BN + tid) * 2 + 1]; }
            p.stats[(int64_t)x * 2 * p.N + n0 + tid] = a;
            p.stats[(int64_t)x * 2 * p.N + p.N + n0 + tid] = b;
        }
    }
}

typedef void (*Nt2Kernel)(Gemm2Args);
// THE tables of pw_gemm_nt_dma_kernel instantiations (nt2_kernel in pwgemm.hip, nt2_red_kernel in pwntred.hip) are switches over this key: what neither names is not compiled (one more live register broke <3,0,1,2>)
static constexpr int nt2_key(int TN, int XF, int BF, int RED, int X6, int RB) { return ((((TN * 3 + XF) * 2 + BF) * 3 + RED) * 4 + X6) * 2 + RB; }
Nt2Kernel nt2_red_kernel(int TN, int XF, int BF, int RED, int X6, int RB);      // pwntred.hip: the RED != 0 table, nullptr: no such kernel

}  // namespace mny
