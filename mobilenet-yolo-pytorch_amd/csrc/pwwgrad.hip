// Pointwise (1x1) convolution, weight gradient:  dW[N,K] = dY[M,N]^T * act_in(X)[M,K]      ("TN", reduction over M), mny_pw_wgrad / mny_pw_wgrad_bf16.
// The three tile-kernel templates (register-staged, LDS-DMA fp32 / six-product, LDS-DMA bf16 storage: 113 instantiations) with their tables and plan,
// the fixed-order combine of the partial rows (reduce_parts_kernel, also launched for pwbnbwd.hip: reduce_parts_launch of pwgemm.h), the bias
// gradient's column sums, the route (pw_wgrad_route: the stream kernel of pwwgs.hip or a tile kernel) and the entry points.
#include "pwgemm.h"
#include "x6.h"
#include "dma_zero.h"

namespace mny {

// ------------------------------------------------------------------------------------------------
// weight gradient: dW[N][K] = sum_m dY[m][n] * act_in(X)[m][k]      (reduction over M, output tiny)
//
// Both operands are M-major, which is exactly the MFMA operand layout (lane = channel, k = row).
// A block owns a BI x BJ tile of dW for a slice of M; it streams 16/32-row chunks of dY and X through a
// double-buffered LDS stage (coalesced float4 loads along the channel axis, BN-apply + activation applied
// to X on the way in) and feeds v_mfma_f32_32x32x2_f32 from conflict-free ds_read_b32 (lanes = consecutive
// channels).  Two decompositions:
//   MODE 0 (fat dW):  2x2 waves, each TIxTJ tiles of 32x32 -> BI = 64*TI, BJ = 64*TJ, chunk = 16 rows.
//   MODE 1 (thin dW): all 4 waves own the SAME TIxTJ tiles (BI = 32*TI, BJ = 32*TJ = whole dW) and split the
//                     32-row chunk four ways; a fixed-order LDS reduction combines them at the end.
// Partials [split][N][K] are then summed in a fixed order by reduce_parts_kernel (deterministic).
// ------------------------------------------------------------------------------------------------
struct WgradArgs {   // X / dY are T* of the kernel instantiation
    const void* X; const float* in_scale; const float* in_shift; int in_act;
    const void* dY; float* partial;
    int64_t M; int K; int N;
    int64_t rows_per_block;
    int gx, gy, splits;          // XCD-aware launches of the LDS-DMA kernels (1-D grid): output tiles gx x gy, M splits; gx == 0: plain 3-D grid
};

// XCD-aware block order of the LDS-DMA weight-gradient kernels (round 3).  The gx*gy output tiles of one M split read the SAME rows of X
// and dY; launched as a (gx, gy, splits) grid their workgroups have consecutive linear ids and the dispatcher deals those round-robin
// over the 8 XCDs — each with its own L2 — so every tile fetched its operands from HBM again: counter traffic 1.67x the algorithmic bytes
// (profiles/r02_traffic_mny_pw_wgrad.json; K64 N384 = 6 tiles: (384 + 6*64) / (384 + 64) = 1.71).  A 1-D grid of 8*ceil(splits/8)*gx*gy
// blocks, block L -> XCD L & 7, puts all tiles of a split on one XCD, next to each other in its dispatch order.
struct WgBlock { int bx, by, bz; bool live; };
__device__ __forceinline__ WgBlock wg_block(const WgradArgs& p) {
    WgBlock b;
    if (p.gx == 0) { b.bx = blockIdx.x; b.by = blockIdx.y; b.bz = blockIdx.z; b.live = true; return b; }
    const int T = p.gx * p.gy, L = blockIdx.x, idx = L >> 3, grp = idx / T, t = idx - grp * T;
    b.bz = grp * 8 + (L & 7);
    b.bx = t % p.gx; b.by = t / p.gx;
    b.live = b.bz < p.splits;
    return b;
}

template <typename T, int MODE, int TI, int TJ>
__global__ __launch_bounds__(256) void pw_wgrad_kernel(WgradArgs p) {
    constexpr int KC = MODE == 0 ? 16 : 32;
    constexpr int BI = (MODE == 0 ? 64 : 32) * TI;
    constexpr int BJ = (MODE == 0 ? 64 : 32) * TJ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;                      // [2][KC][BI]  dY
    float* sB = smem + 2 * KC * BI;        // [2][KC][BJ]  act(X)
    float* sScale = sB + 2 * KC * BJ;      // [BJ]
    float* sShift = sScale + BJ;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kk = lane >> 5;
    const int co0 = blockIdx.x * BI, ci0 = blockIdx.y * BJ;
    const int64_t m_begin = (int64_t)blockIdx.z * p.rows_per_block;
    const int64_t m_end = min(m_begin + p.rows_per_block, p.M);
    const bool has_xf = p.in_scale != nullptr;
    const bool do_xf = has_xf || p.in_act != MNY_ACT_NONE;
    const bool vecA = (p.N & 3) == 0, vecB = (p.K & 3) == 0;

    for (int j = tid; j < BJ; j += 256) {
        const int ci = ci0 + j;
        sScale[j] = (has_xf && ci < p.K) ? p.in_scale[ci] : 1.f;
        sShift[j] = (has_xf && ci < p.K) ? p.in_shift[ci] : 0.f;
    }
    __syncthreads();

    const int ioff = MODE == 0 ? (wave >> 1) * 32 * TI : 0;
    const int joff = MODE == 0 ? (wave & 1) * 32 * TJ : 0;
    const int krow0 = MODE == 0 ? 0 : wave * (KC / 4);
    constexpr int KROWS = MODE == 0 ? KC : KC / 4;

    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    constexpr int A_F4 = KC * BI / 4, B_F4 = KC * BJ / 4;
    constexpr int A_PER = (A_F4 + 255) / 256, B_PER = (B_F4 + 255) / 256;
    float4 ra[A_PER], rb[B_PER];

    auto gload = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int idx = tid + i * 256;
            float4 v = f4zero();
            if (idx < A_F4) {
                const int row = idx / (BI / 4), c = (idx % (BI / 4)) * 4;
                const int64_t m = m0 + row;
                const int co = co0 + c;
                if (m < m_end && co < p.N) {
                    const T* src = (const T*)p.dY + m * p.N + co;
                    if (vecA) v = ld4(src);
                    else { v.x = ld1(src); if (co + 1 < p.N) v.y = ld1(src + 1); if (co + 2 < p.N) v.z = ld1(src + 2); if (co + 3 < p.N) v.w = ld1(src + 3); }
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int idx = tid + i * 256;
            float4 v = f4zero();
            if (idx < B_F4) {
                const int row = idx / (BJ / 4), c = (idx % (BJ / 4)) * 4;
                const int64_t m = m0 + row;
                const int ci = ci0 + c;
                if (m < m_end && ci < p.K) {
                    const T* src = (const T*)p.X + m * p.K + ci;
                    if (vecB) v = ld4(src);
                    else { v.x = ld1(src); if (ci + 1 < p.K) v.y = ld1(src + 1); if (ci + 2 < p.K) v.z = ld1(src + 2); if (ci + 3 < p.K) v.w = ld1(src + 3); }
                    if (do_xf) {
                        v = xform4(v, ld4(sScale + c), ld4(sShift + c), p.in_act);
                        if (!vecB) { if (ci + 1 >= p.K) v.y = 0.f; if (ci + 2 >= p.K) v.z = 0.f; if (ci + 3 >= p.K) v.w = 0.f; }
                    }
                }
            }
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int idx = tid + i * 256;
            if (idx < A_F4) st4(sA + buf * KC * BI + idx * 4, ra[i]);       // [row][c] is exactly idx*4
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int idx = tid + i * 256;
            if (idx < B_F4) st4(sB + buf * KC * BJ + idx * 4, rb[i]);
        }
    };

    const int64_t nchunks = (m_end - m_begin + KC - 1) / KC;
    if (nchunks > 0) {
        gload(m_begin);
        lstore(0);
    }
    __syncthreads();
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int buf = (int)(ch & 1);
        if (ch + 1 < nchunks) gload(m_begin + (ch + 1) * KC);
        const float* a_base = sA + buf * KC * BI + (krow0 + kk) * BI + ioff + li;
        const float* b_base = sB + buf * KC * BJ + (krow0 + kk) * BJ + joff + li;
#pragma unroll
        for (int kp = 0; kp < KROWS / 2; ++kp) {
            float af[TI], bf[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) af[i] = a_base[kp * 2 * BI + i * 32];
#pragma unroll
            for (int j = 0; j < TJ; ++j) bf[j] = b_base[kp * 2 * BJ + j * 32];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (ch + 1 < nchunks) lstore(buf ^ 1);
        __syncthreads();
    }

    float* dst = p.partial + (int64_t)blockIdx.z * p.N * p.K;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const int ci = ci0 + joff + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + ioff + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                    if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = acc[i][j][r];
                }
            }
    } else {
        float* red = smem;                 // [3][16][64] (12 KB <= staging area)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                __syncthreads();
                if (wave > 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[i][j][r];
                }
                __syncthreads();
                if (wave == 0) {
                    const int ci = ci0 + j * 32 + li;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = ((acc[i][j][r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) + red[(2 * 16 + r) * 64 + lane];
                        const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                        if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = v;
                    }
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// weight gradient v2: the same decomposition fed by LDS-DMA (3-stage ring of 16-row chunks, counted
// vmcnt, raw barriers).  The chunk image [row][channel] is linear, i.e. exactly the lane-linear order a
// DMA instruction writes, and fragments are read along the channel axis (conflict-free ds_read_b32), so no
// swizzle is needed.  Rows past the block's M-slice take dY from a 16-B zero buffer (product = 0 * finite),
// X rows are clamped to a valid row; BN-apply + activation is applied to X when its fragment is read.
// Requires N % 4 == 0 and K % 4 == 0 (16-B aligned rows) and a non-hswish view.
// ------------------------------------------------------------------------------------------------
template <int MODE, int TI, int TJ, int X6 = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TI * TJ >= 8 ? 2 : 1, 8))) void pw_wgrad_dma_kernel(WgradArgs p) {
    constexpr int KC = 16, S = 3;
    constexpr int BI = (MODE == 0 ? 64 : 32) * TI;
    constexpr int BJ = (MODE == 0 ? 64 : 32) * TJ;
    constexpr int A_ST = KC * BI, B_ST = KC * BJ, STAGE = A_ST + B_ST;      // floats
    constexpr int NA = A_ST / 256, NB = B_ST / 256, NL = NA + NB;           // 1-KiB DMA instructions per stage
    constexpr int LPW = (NL + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kk = lane >> 5;
    const WgBlock blk = wg_block(p);
    if (!blk.live) return;
    const int co0 = blk.bx * BI, ci0 = blk.by * BJ;
    const int64_t m_begin = (int64_t)blk.bz * p.rows_per_block;
    const int64_t m_end = min(m_begin + p.rows_per_block, p.M);
    const bool has_xf = p.in_scale != nullptr;
    const float slope = act_slope(p.in_act), hi = act_hi(p.in_act);

    const int ioff = MODE == 0 ? (wave >> 1) * 32 * TI : 0;
    const int joff = MODE == 0 ? (wave & 1) * 32 * TJ : 0;
    const int krow0 = MODE == 0 ? 0 : wave * (KC / 4);
    constexpr int KROWS = MODE == 0 ? KC : KC / 4;

    float sc[TJ], sh[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        const int ci = ci0 + joff + j * 32 + li;
        sc[j] = (has_xf && ci < p.K) ? p.in_scale[ci] : 1.f;
        sh[j] = (has_xf && ci < p.K) ? p.in_shift[ci] : 0.f;
    }

    // per-lane constants of this wave's DMA instructions
    const float* zero_src = reinterpret_cast<const float*>(&mny_zero16);
    // running sources (round 3, as in the NT GEMM): one pointer per slot, bumped by 16 rows per stage; rows past the block's M slice
    // select a fixed filler (dY: zeros, X: the slice's last row) — no per-instruction branch, no 64-bit multiply in the loop
    int d_row[LPW], d_lds[LPW], d_step[LPW];
    const float* d_cur[LPW];
    const float* d_past[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int j = wave + 4 * i;
        if (j >= NL) j = NL - 1;
        const bool isA = j < NA;
        const int q = (isA ? j : j - NA) * 64 + lane;                // float4 index inside the tile
        const int W4 = (isA ? BI : BJ) / 4;
        d_row[i] = q / W4;
        const int c = (q % W4) * 4;
        d_lds[i] = isA ? j * 256 : A_ST + (j - NA) * 256;
        const bool ok = isA ? co0 + c < p.N : ci0 + c < p.K;
        const float* base = isA ? (const float*)p.dY : (const float*)p.X;
        const int stride = isA ? p.N : p.K, off = isA ? co0 + c : ci0 + c;
        d_cur[i] = ok ? base + (m_begin + d_row[i]) * stride + off : zero_src;
        d_past[i] = (ok && !isA) ? base + (m_end - 1) * stride + off : zero_src;
        d_step[i] = ok ? KC * stride : 0;
    }

    auto issue = [&](int64_t m0, int slot) {
        float* stage = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const float* src = (m0 + d_row[i] < m_end) ? d_cur[i] : d_past[i];
            d_cur[i] += d_step[i];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(stage + d_lds[i]), 16, 0, 0);
        }
    };

    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int slot) {
        const float* a_base = smem + slot * STAGE + (krow0 + kk) * BI + ioff + li;
        const float* b_base = smem + slot * STAGE + A_ST + (krow0 + kk) * BJ + joff + li;
        if constexpr (X6 != 0 && MODE == 0) {
            // six-product bf16 form (see x6_split): the lane's eight rows of the chunk are rows 2*kp + kk, the ones the fp32 path
            // feeds one MFMA step at a time; a whole 16-row chunk is one v_mfma_f32_32x32x16_bf16 per partial product
            bf16x8_t ah[TI], am[TI], al[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const v4f_t x0 = {a_base[0 * BI + i * 32], a_base[2 * BI + i * 32], a_base[4 * BI + i * 32], a_base[6 * BI + i * 32]};
                const v4f_t x1 = {a_base[8 * BI + i * 32], a_base[10 * BI + i * 32], a_base[12 * BI + i * 32], a_base[14 * BI + i * 32]};
                x6_split(x0, x1, ah[i], am[i], al[i]);
            }
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                float z[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = fmaf(b_base[2 * e * BJ + j * 32], sc[j], sh[j]);
                    z[e] = fminf(fmaxf(t, slope * t), hi);
                }
                bf16x8_t bh, bm, bl;
                x6_split(v4f_t{z[0], z[1], z[2], z[3]}, v4f_t{z[4], z[5], z[6], z[7]}, bh, bm, bl);
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
                }
            }
            return;
        }
#pragma unroll
        for (int kp = 0; kp < KROWS / 2; ++kp) {
            float af[TI], bf[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) af[i] = a_base[kp * 2 * BI + i * 32];
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const float z = fmaf(b_base[kp * 2 * BJ + j * 32], sc[j], sh[j]);
                bf[j] = fminf(fmaxf(z, slope * z), hi);
            }
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };

    const int total = (int)((m_end - m_begin + KC - 1) / KC);
    int i_t = 0, i_slot = 0, c_slot = 0;
    auto issue_next = [&]() {
        issue(m_begin + (int64_t)i_t * KC, i_slot);
        ++i_t;
        if (++i_slot == S) i_slot = 0;
    };
    const int pre = total < S - 1 ? total : S - 1;
    for (int t = 0; t < pre; ++t) issue_next();
    const int steady = total - pre;
    for (int t = 0; t < steady; ++t) {
        wait_vmcnt<LPW*(S - 2)>();
        __builtin_amdgcn_s_barrier();
        issue_next();
        compute(c_slot);
        if (++c_slot == S) c_slot = 0;
    }
    for (int t = 0; t < pre; ++t) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        compute(c_slot);
        if (++c_slot == S) c_slot = 0;
    }

    float* dst = p.partial + (int64_t)blk.bz * p.N * p.K;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const int ci = ci0 + joff + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + ioff + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                    if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = acc[i][j][r];
                }
            }
    } else {
        float* red = smem;                 // [3][16][64] (12 KB <= ring)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                __syncthreads();
                if (wave > 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[i][j][r];
                }
                __syncthreads();
                if (wave == 0) {
                    const int ci = ci0 + j * 32 + li;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = ((acc[i][j][r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) + red[(2 * 16 + r) * 64 + lane];
                        const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                        if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = v;
                    }
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// weight gradient, bf16 operands (dY, X in bf16): same tile decomposition and LDS-DMA ring, on
// v_mfma_f32_32x32x16_bf16.  The MFMA wants, per lane, 8 consecutive REDUCTION indices (rows m) of one
// channel, but the chunk image is [row][channel] with channels contiguous — exactly the case gfx950's
// transposing LDS read exists for: ds_read_b64_tr_b16 hands lane c of a 16-lane group the 4 rows of column c of a
// [4 rows][16 channels] block (each lane supplies the address of 4 contiguous channels of row i/4), so two such
// reads build one operand with no shuffles.  BN-apply + activation of X runs on the transposed fragment, where
// a lane holds ONE channel (scalar scale/shift per lane).  MODE 0: 16-row chunks, 2x2 waves over the tile;
// MODE 1: 64-row chunks, each wave a 16-row quarter of the whole (thin) dW, combined through LDS at the end.
// Requires N % 8 == 0 and K % 8 == 0 (16-B chunks of 8 bf16); anything else takes the register-staged kernel.
// ------------------------------------------------------------------------------------------------
typedef short v4s_t __attribute__((ext_vector_type(4)));

template <int MODE, int TI, int TJ, int XF>
__global__ __launch_bounds__(256) void pw_wgrad_bf16_kernel(WgradArgs p) {
    constexpr int KC = MODE == 0 ? 16 : 64, S = 3;
    constexpr int BI = (MODE == 0 ? 64 : 32) * TI;
    constexpr int BJ = (MODE == 0 ? 64 : 32) * TJ;
    constexpr int A_ST = KC * BI, B_ST = KC * BJ, STAGE = A_ST + B_ST;      // bf16 elements
    constexpr int NA = A_ST / 512, NB = B_ST / 512, NL = NA + NB;           // 1-KiB DMA instructions per stage
    constexpr int LPW = (NL + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    bf16_t* smem = reinterpret_cast<bf16_t*>(smem_f);
    const bf16_t* pX = (const bf16_t*)p.X;
    const bf16_t* pdY = (const bf16_t*)p.dY;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kk = lane >> 5;
    const WgBlock blk = wg_block(p);
    if (!blk.live) return;
    const int co0 = blk.bx * BI, ci0 = blk.by * BJ;
    const int64_t m_begin = (int64_t)blk.bz * p.rows_per_block;
    const int64_t m_end = min(m_begin + p.rows_per_block, p.M);
    const bool has_xf = p.in_scale != nullptr;
    const float slope = act_slope(p.in_act), hi = act_hi(p.in_act);

    const int ioff = MODE == 0 ? (wave >> 1) * 32 * TI : 0;
    const int joff = MODE == 0 ? (wave & 1) * 32 * TJ : 0;
    const int krow0 = MODE == 0 ? 0 : wave * 16;

    float sc[TJ], sh[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        const int ci = ci0 + joff + j * 32 + li;
        sc[j] = (has_xf && ci < p.K) ? p.in_scale[ci] : 1.f;
        sh[j] = (has_xf && ci < p.K) ? p.in_shift[ci] : 0.f;
    }

    const bf16_t* zero_src = reinterpret_cast<const bf16_t*>(&mny_zero16);
    // running sources (round 3): see pw_wgrad_dma_kernel
    int d_row[LPW], d_lds[LPW], d_step[LPW];
    const bf16_t* d_cur[LPW];
    const bf16_t* d_past[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int j = wave + 4 * i;
        if (j >= NL) j = NL - 1;
        const bool isA = j < NA;
        const int q = (isA ? j : j - NA) * 64 + lane;                // 16-B chunk index inside the tile
        const int W8 = (isA ? BI : BJ) / 8;
        d_row[i] = q / W8;
        const int c = (q % W8) * 8;
        d_lds[i] = isA ? j * 512 : A_ST + (j - NA) * 512;            // bf16 elements
        const bool ok = isA ? co0 + c < p.N : ci0 + c < p.K;
        const bf16_t* base = isA ? pdY : pX;
        const int stride = isA ? p.N : p.K, off = isA ? co0 + c : ci0 + c;
        d_cur[i] = ok ? base + (m_begin + d_row[i]) * stride + off : zero_src;
        d_past[i] = (ok && !isA) ? base + (m_end - 1) * stride + off : zero_src;
        d_step[i] = ok ? KC * stride : 0;
    }

    auto issue = [&](int64_t m0, int slot) {
        bf16_t* stage = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const bf16_t* src = (m0 + d_row[i] < m_end) ? d_cur[i] : d_past[i];
            d_cur[i] += d_step[i];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(stage + d_lds[i]), 16, 0, 0);
        }
    };

    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposing read: 16-lane group g = (lane>>4)&1 covers channels 16g..16g+15 of the lane's 32-channel tile; lane i of
    // the group addresses row i/4, channels 4(i%4)..+3 of the [4][16] block and RECEIVES rows 0..3 of channel i.
    const int tr_row = (lane & 15) >> 2;
    const int tr_col = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
    auto frag = [&](const bf16_t* tile, int pitch, int col0) -> uint4 {
        const bf16_t* base = tile + (krow0 + 8 * kk + tr_row) * pitch + col0 + tr_col;
        const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(base));
        const v4s_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(base + 4 * pitch));
        const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi4);
        return make_uint4(a.x, a.y, b.x, b.y);                    // k = 8*kk + 0..7 of this lane's channel
    };

    auto compute = [&](int slot) {
        const bf16_t* tA = smem + slot * STAGE;
        const bf16_t* tB = tA + A_ST;
        uint4 af[TI], bf[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = frag(tA, BI, ioff + i * 32);
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            uint4 u = frag(tB, BJ, joff + j * 32);
            if (XF != 0) {
                float z[8] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                              __uint_as_float(u.y & 0xffff0000u), __uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u),
                              __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u)};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float zz = fmaf(z[e], sc[j], sh[j]);
                    z[e] = XF == 1 ? __builtin_amdgcn_fmed3f(zz, slope * zz, hi) : zz * __builtin_amdgcn_fmed3f(zz + 3.f, 0.f, 6.f) * (1.f / 6.f);
                }
                u = make_uint4(pack_bf16x2(z[0], z[1]), pack_bf16x2(z[2], z[3]), pack_bf16x2(z[4], z[5]), pack_bf16x2(z[6], z[7]));
            }
            bf[j] = u;
        }
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bf[j]),
                                                                    acc[i][j], 0, 0, 0);
    };

    const int total = (int)((m_end - m_begin + KC - 1) / KC);
    int i_t = 0, i_slot = 0, c_slot = 0;
    auto issue_next = [&]() {
        issue(m_begin + (int64_t)i_t * KC, i_slot);
        ++i_t;
        if (++i_slot == S) i_slot = 0;
    };
    const int pre = total < S - 1 ? total : S - 1;
    for (int t = 0; t < pre; ++t) issue_next();
    const int steady = total - pre;
    for (int t = 0; t < steady; ++t) {
        wait_vmcnt<LPW*(S - 2)>();
        __builtin_amdgcn_s_barrier();
        issue_next();
        compute(c_slot);
        if (++c_slot == S) c_slot = 0;
    }
    for (int t = 0; t < pre; ++t) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        compute(c_slot);
        if (++c_slot == S) c_slot = 0;
    }

    float* dst = p.partial + (int64_t)blk.bz * p.N * p.K;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                const int ci = ci0 + joff + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + ioff + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                    if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = acc[i][j][r];
                }
            }
    } else {
        float* red = smem_f;               // [3][16][64] floats (12 KB <= ring)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                __syncthreads();
                if (wave > 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[i][j][r];
                }
                __syncthreads();
                if (wave == 0) {
                    const int ci = ci0 + j * 32 + li;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = ((acc[i][j][r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) + red[(2 * 16 + r) * 64 + lane];
                        const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                        if (co < p.N && ci < p.K) dst[(int64_t)co * p.K + ci] = v;
                    }
                }
            }
    }
}

typedef void (*WgKernel)(WgradArgs);
static WgKernel wg_bf16_kernel(int mode, int TI, int TJ, int XF) {
    switch (mode * 100 + TI * 10 + TJ) {
#define MNY_W(MD, I, J) case MD * 100 + I * 10 + J: return XF == 0 ? (WgKernel)pw_wgrad_bf16_kernel<MD, I, J, 0> : XF == 1 ? (WgKernel)pw_wgrad_bf16_kernel<MD, I, J, 1> : (WgKernel)pw_wgrad_bf16_kernel<MD, I, J, 2>;
        MNY_W(0, 1, 1) MNY_W(0, 1, 2) MNY_W(0, 2, 1) MNY_W(0, 2, 2)
        MNY_W(1, 1, 1) MNY_W(1, 1, 2) MNY_W(1, 1, 3) MNY_W(1, 1, 4) MNY_W(1, 1, 5) MNY_W(1, 1, 6) MNY_W(1, 2, 1) MNY_W(1, 2, 2) MNY_W(1, 2, 3)
        MNY_W(1, 3, 1) MNY_W(1, 3, 2) MNY_W(1, 4, 1) MNY_W(1, 5, 1) MNY_W(1, 6, 1)
#undef MNY_W
        default: return nullptr;
    }
}

// the tiles the six-product form is compiled for (the cases of wg_dma_kernel below); every other tile of a six-product route runs the fp32 MFMA
static bool wg_has_x6(int mode, int TI, int TJ) {
    const int t = TI * 10 + TJ;
    return mode == 0 && (t == 11 || t == 12 || t == 21 || t == 22 || t == 24);
}

static WgKernel wg_dma_kernel(int mode, int TI, int TJ, int x6 = 0) {
    if (x6 && wg_has_x6(mode, TI, TJ)) switch (TI * 10 + TJ) {
        case 11: return (WgKernel)pw_wgrad_dma_kernel<0, 1, 1, 1>; case 12: return (WgKernel)pw_wgrad_dma_kernel<0, 1, 2, 1>;
        case 21: return (WgKernel)pw_wgrad_dma_kernel<0, 2, 1, 1>; case 22: return (WgKernel)pw_wgrad_dma_kernel<0, 2, 2, 1>;
        case 24: return (WgKernel)pw_wgrad_dma_kernel<0, 2, 4, 1>;
    }
    switch (mode * 100 + TI * 10 + TJ) {
#define MNY_W(MD, I, J) case MD * 100 + I * 10 + J: return (WgKernel)pw_wgrad_dma_kernel<MD, I, J>;
        MNY_W(0, 1, 1) MNY_W(0, 1, 2) MNY_W(0, 2, 1) MNY_W(0, 2, 2)
        MNY_W(1, 1, 1) MNY_W(1, 1, 2) MNY_W(1, 1, 3) MNY_W(1, 1, 4) MNY_W(1, 1, 5) MNY_W(1, 1, 6) MNY_W(1, 2, 1) MNY_W(1, 2, 2) MNY_W(1, 2, 3)
        MNY_W(1, 3, 1) MNY_W(1, 3, 2) MNY_W(1, 4, 1) MNY_W(1, 5, 1) MNY_W(1, 6, 1)
#undef MNY_W
        default: return nullptr;
    }
}

struct WgPlan { int mode, TI, TJ, gx, gy, splits; int64_t rows_per_block; size_t lds, lds_dma; };

static int pick_block(int c) {      // 64 or 128: minimise the padded extent, ties -> 128
    const int p64 = (int)cdiv(c, 64) * 64, p128 = (int)cdiv(c, 128) * 128;
    return p128 <= p64 ? 128 : 64;
}

// wide (round 6): the six-product fp32 form with a 128 x 256 tile per workgroup (a wave = 2 x 4 blocks of 32: three operand cuts per 24 MFMAs instead
// of four — both operands of a weight gradient are activations, cut in the kernel —, and a 512 x 512 problem re-reads dY twice and X four times
// instead of four + four); 254 VGPRs at two waves per SIMD, 72 KB of LDS ring (two workgroups per CU).  The split count is the 128 x 128 plan's
// either way, so the partial-row count does not depend on which of the two a launch takes.  Measured (bracketed steps, same box): 512 x 512 @
// M 123 904 0.423 -> 0.399 ms, 1280 -> 512 @ 30 976 0.262 -> 0.248, the 33 weight gradients of the headline step 4.30 -> 4.20 ms
static bool wg_wide_shape(int64_t M, int K, int N) {
    return nt_x6(M, K, N) && K % 256 == 0 && N % 128 == 0;
}

static WgPlan wg_plan(int64_t M, int K, int N, bool bf16 = false, bool wide_ok = false) {
    WgPlan pl;
    const int nco = (int)cdiv(N, 32), nci = (int)cdiv(K, 32);
    int BI, BJ, KC;
    if (nco * nci <= 6) {
        pl.mode = 1; pl.TI = nco; pl.TJ = nci; BI = 32 * nco; BJ = 32 * nci; KC = bf16 ? 64 : 32;
        pl.gx = pl.gy = 1;
    } else if (!bf16 && ((K == 96 && N >= 192) || (N == 96 && K >= 192))) {
        // a 96-wide side is 1.5 of the 64-wide units of the 2x2-wave tiles (25-33 % of the MFMAs multiply padding): slice the
        // other side instead and give every workgroup exact 96 x 64 tiles in the all-waves-share-the-tile mode
        pl.mode = 1; KC = 32;
        if (K == 96) { pl.TJ = 3; pl.TI = 2; } else { pl.TI = 3; pl.TJ = 2; }
        BI = 32 * pl.TI; BJ = 32 * pl.TJ;
        pl.gx = (int)cdiv(N, BI); pl.gy = (int)cdiv(K, BJ);
    } else {
        pl.mode = 0; BI = pick_block(N); BJ = pick_block(K); KC = 16;
        pl.TI = BI / 64; pl.TJ = BJ / 64;
        pl.gx = (int)cdiv(N, BI); pl.gy = (int)cdiv(K, BJ);
    }
    constexpr int wg_blocks = 1024;     // (round 6, next to the 128 x 256 tile: 1536 -> 1024: weight gradients 4.00 -> 3.99 ms, their combines 0.34 -> 0.31 ms, 0.4 GB fewer partial rows per step; 768: 4.32 ms)
    int64_t splits = wg_blocks / ((int64_t)pl.gx * pl.gy);
    if (splits < 1) splits = 1;
    const int64_t max_splits = cdiv(M, 4 * KC);
    if (splits > max_splits) splits = max_splits;
    if (splits > 768) splits = 768;
    const int64_t rpb = cdiv(cdiv(M, splits), KC) * KC;
    pl.rows_per_block = rpb;
    pl.splits = (int)cdiv(M, rpb);
    if (wide_ok && !bf16 && pl.mode == 0 && BI == 128 && wg_wide_shape(M, K, N)) { BJ = 256; pl.TJ = 4; pl.gy = K / 256; }
    size_t stage = (size_t)2 * (bf16 ? 32 : KC) * (BI + BJ) * sizeof(float);    // register-staged kernel: fp32 image, its own KC
    if (pl.mode == 0) stage = (size_t)2 * 16 * (BI + BJ) * sizeof(float);
    if (stage < 3 * 16 * 64 * sizeof(float)) stage = 3 * 16 * 64 * sizeof(float);
    pl.lds = stage + 2 * BJ * sizeof(float);
    pl.lds_dma = bf16 ? (size_t)3 * KC * (BI + BJ) * 2 : (size_t)3 * 16 * (BI + BJ) * sizeof(float);
    if (pl.lds_dma < 3 * 16 * 64 * sizeof(float)) pl.lds_dma = 3 * 16 * 64 * sizeof(float);
    return pl;
}

// partial rows [parts][n] -> out[n]: 32 outputs x 8 part-slices per block, fp64, fixed order
__global__ __launch_bounds__(256) void reduce_parts_kernel(const float* __restrict__ parts, int nparts, int64_t n, float* __restrict__ out) {
    __shared__ double red[8][32];
    const int ol = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int64_t i = (int64_t)blockIdx.x * 32 + ol;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (i < n) {
        int pidx = slice;                              // four partial rows in flight per thread: the loop is pure load latency otherwise
        for (; pidx + 24 < nparts; pidx += 32) {
            s0 += (double)parts[(int64_t)pidx * n + i];        s1 += (double)parts[(int64_t)(pidx + 8) * n + i];
            s2 += (double)parts[(int64_t)(pidx + 16) * n + i]; s3 += (double)parts[(int64_t)(pidx + 24) * n + i];
        }
        for (; pidx < nparts; pidx += 8) s0 += (double)parts[(int64_t)pidx * n + i];
    }
    red[slice][ol] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (slice == 0 && i < n) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) s += red[k][ol];
        out[i] = (float)s;
    }
}

// column sums of a [M][C] matrix -> partial rows; used for the head convs' bias gradient
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ y, float* __restrict__ parts, int64_t M, int C,
                                                     int64_t rows_per_block) {
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    const int slot = threadIdx.x >> 6;
    __shared__ float red[4][64];
    const int64_t m0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t m1 = min(m0 + rows_per_block, M);
    float s = 0.f;
    if (c < C)
        for (int64_t m = m0 + slot; m < m1; m += 4) s += ld1(y + m * C + c);
    red[slot][threadIdx.x & 63] = s;
    __syncthreads();
    if (slot == 0 && c < C) parts[(int64_t)blockIdx.x * C + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

static int colsum_parts(int64_t M) { int64_t p = cdiv(M, 256); return (int)(p < 512 ? p : 512); }

void reduce_parts_launch(const float* parts, int nparts, int64_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, st, parts, nparts, n, out);
}

}  // namespace mny

using namespace mny;
static thread_local int g_wg_kernel = -1;       // kernel code of this thread's last weight-gradient call (mny_pw_wgrad_last_kernel below)

// ---- which kernel a weight-gradient call takes ---------------------------------------------------------------------------------------------
// The route of this operation, as PwRoute is of the forward / data-gradient ones (pwgemm.hip): the complete description of a call in, the decision
// out.  The launcher acts on it; mny_pw_wgrad_splits*, _ws_floats, _kernel and mny_pw_route(op = 2) ask the same function.  pw_wgs_ok, the
// MNY_WGRAD_V1 switch and the channel-alignment test of the weight gradient appear here only.
struct WgRoute {
    int family = MNY_ROUTE_TILE_V1;     // MNY_ROUTE_*
    const char* why = nullptr;          // NULL: supported; else what keeps the call off this entry point
    int parts = MNY_EINVAL;             // the splits of the partial rows [splits][Nc][K] the call writes
    int x6 = 0;                         // an LDS-DMA route under the six-product rule (nt_x6)
    WgPlan wg{};                        // tile kernels
    int wg_xf = 0;                      //   the XF of the bf16 LDS-DMA kernel: 0 = no view, 1 = linear / clamp view, 2 = h-swish view
    int wg_kernel = MNY_EINVAL;         //   the kernel launched: template * 1000 + MODE * 100 + TI * 10 + TJ (mny_pw_wgrad_kernel)
};

// (mny_pw_wgrad, _bf16)
static WgRoute pw_wgrad_route(int bf, int64_t M, int K, int Nc, int in_act, bool bias_grad, bool view) {      // view: in_scale / in_shift are passed
    WgRoute r;
    if (M <= 0 || K <= 0 || Nc <= 0) { r.why = "empty problem"; return r; }
    if (!bf && pw_wgs_ok(M, K, Nc) && !bias_grad) {        // narrow-sided shape: barrier-free stream kernel (pwwgs.hip)
        r.family = MNY_ROUTE_WGRAD_STREAM;
        r.parts = pw_wgs_splits(M, K, Nc);
        r.wg_kernel = 5000;
        return r;
    }
    // the LDS-DMA kernels read raw 16-B chunks: aligned rows only; the fp32 one has no h-swish view
    const int al = bf ? 7 : 3;
    const bool dma = (Nc & al) == 0 && (K & al) == 0 && !sw(SW_WGRAD_V1) && (bf || in_act != MNY_ACT_HSWISH);
    r.x6 = !bf && dma && nt_x6(M, K, Nc);
    r.family = !dma ? MNY_ROUTE_TILE_V1 : r.x6 ? MNY_ROUTE_DMA_X6 : MNY_ROUTE_DMA_F32;
    r.wg = wg_plan(M, K, Nc, bf, !bf && dma);
    r.parts = r.wg.splits;
    r.wg_xf = (!view && in_act == MNY_ACT_NONE) ? 0 : (in_act == MNY_ACT_HSWISH ? 2 : 1);
    // The kernel template.  The six-product form is compiled for five MODE 0 tiles only: a six-product route whose plan is MODE 1 (K 96, N 576)
    // or another MODE 0 tile (!wg_has_x6) runs the plain fp32-MFMA kernel of that tile: wg_dma_kernel falls through to its second table.  That is kept as it
    // is.  The family stays MNY_ROUTE_DMA_X6 — it names the rule the shape fell under —, the kernel code says template 1: what is launched.
    const int tile = r.wg.mode * 100 + r.wg.TI * 10 + r.wg.TJ;
    const int tmpl = !dma ? 0 : bf ? 3 : (r.x6 && wg_has_x6(r.wg.mode, r.wg.TI, r.wg.TJ)) ? 2 : 1;
    r.wg_kernel = tmpl * 1000 + tile;
    return r;
}

int mny::pw_wgrad_family(int bf, int64_t M, int K, int N) { return pw_wgrad_route(bf, M, K, N, MNY_ACT_NONE, false, false).family; }

// room for whichever kernel the call takes: with a bias gradient the narrow-sided shapes stay off the stream kernel, and the bf16 entry point (which
// has no query of its own) plans a 96-wide side on the 2x2-wave tiles with 16-row chunks: up to twice the splits of the fp32 plan (K 96, N 200).
// An fp32 caller at such a shape pays for the bf16 plan's rows too (memory only).
extern "C" size_t mny_pw_wgrad_ws_floats(int64_t M, int K, int Nc) {
    if (M <= 0 || K <= 0 || Nc <= 0) return 0;
    int parts = pw_wgrad_route(0, M, K, Nc, MNY_ACT_NONE, false, false).parts;
    for (const int p : {pw_wgrad_route(0, M, K, Nc, MNY_ACT_NONE, true, false).parts, pw_wgrad_route(1, M, K, Nc, MNY_ACT_NONE, false, false).parts})
        if (p > parts) parts = p;
    return (size_t)parts * Nc * K + (size_t)colsum_parts(M) * Nc;
}
extern "C" int mny_pw_wgrad_splits(int64_t M, int K, int Nc) { return pw_wgrad_route(0, M, K, Nc, MNY_ACT_NONE, false, false).parts; }
extern "C" int mny_pw_wgrad_splits_bf16(int64_t M, int K, int Nc) { return pw_wgrad_route(1, M, K, Nc, MNY_ACT_NONE, false, false).parts; }
// which kernel a weight-gradient call launches, and which one this thread's last call did launch: both read the route's wg_kernel
extern "C" int mny_pw_wgrad_kernel(int bf16, int64_t M, int K, int Nc, int in_act, int has_view, int bias_grad) {
    return pw_wgrad_route(bf16 ? 1 : 0, M, K, Nc, in_act, bias_grad != 0, has_view != 0).wg_kernel;
}
extern "C" int mny_pw_wgrad_last_kernel(void) { return g_wg_kernel; }

template <typename T>
static int pw_wgrad_impl(const T* x, const float* in_scale, const float* in_shift, int in_act, const T* dy,
                         float* dw, float* dbias, float* ws, int64_t M, int K, int Nc, void* stream) {
    MNY_REQUIRE(x && dy && ws, "pw_wgrad: null pointer");
    MNY_REQUIRE(dw || !dbias, "pw_wgrad: a deferred combine (dw == NULL) cannot carry a bias gradient");
    constexpr bool is_f32 = sizeof(T) == 4;
    const WgRoute r = pw_wgrad_route(!is_f32, M, K, Nc, in_act, dbias != nullptr, in_scale != nullptr);
    MNY_REQUIRE(!r.why, "pw_wgrad: %s", r.why);
    pw_set_last_route(r.family);
    g_wg_kernel = r.wg_kernel;
    hipStream_t st = (hipStream_t)stream;
    if (r.family == MNY_ROUTE_WGRAD_STREAM) {              // partial rows [r.parts][Nc][K]
        int rc = pw_wgs_launch((const float*)x, in_scale, in_shift, in_act, (const float*)dy, ws, M, K, Nc, st);
        if (rc || !dw) return rc;
        const int64_t n = (int64_t)Nc * K;
        hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, st, ws, r.parts, n, dw);
        return check_launch("reduce_parts_kernel");
    }
    const WgPlan& pl = r.wg;
    WgradArgs a{x, in_scale, in_shift, in_act, dy, ws, M, K, Nc, pl.rows_per_block, 0, pl.gy, pl.splits};
    dim3 grid(pl.gx, pl.gy, pl.splits), block(256);
    if (r.family != MNY_ROUTE_TILE_V1) {                   // LDS-DMA kernels
        const int tmpl = r.wg_kernel / 1000;                // 1: fp32 MFMA, 2: six-product form, 3: bf16 storage
        const WgKernel dk = tmpl == 3 ? wg_bf16_kernel(pl.mode, pl.TI, pl.TJ, r.wg_xf) : wg_dma_kernel(pl.mode, pl.TI, pl.TJ, tmpl == 2);
        if (!dk) {
            set_error("pw_wgrad: no kernel for mode %d tile %dx%d", pl.mode, pl.TI, pl.TJ); return MNY_EUNSUPPORTED;
        }
        if (pl.lds_dma > 64 * 1024 && !allow_lds((const void*)dk, 160 * 1024)) {      // > 64 KB of dynamic LDS needs a per-kernel opt-in (once)
            set_error("pw_wgrad: hipFuncSetAttribute failed"); return MNY_EHIP;
        }
        // workgroups grouped per XCD (MNY_WGRAD_NO_XCD: same-box A/B switch) — only with >= 64 splits, i.e. >= 8 per XCD: K1280 N512 — 40 tiles,
        // 38 splits — lost 11 % to XCD imbalance
        const bool use_xcd = !sw(SW_WGRAD_NO_XCD) && pl.gx * pl.gy > 1 && pl.splits >= 64;
        if (use_xcd) a.gx = pl.gx;
        hipLaunchKernelGGL(dk, use_xcd ? dim3((unsigned)(cdiv(pl.splits, 8) * 8 * pl.gx * pl.gy)) : grid, block, pl.lds_dma, st, a);
    } else {
#define MNY_WG(MD, I, J) case MD * 100 + I * 10 + J: hipLaunchKernelGGL((pw_wgrad_kernel<T, MD, I, J>), grid, block, pl.lds, st, a); break;
        switch (pl.mode * 100 + pl.TI * 10 + pl.TJ) {
            MNY_WG(0, 1, 1) MNY_WG(0, 1, 2) MNY_WG(0, 2, 1) MNY_WG(0, 2, 2)
            MNY_WG(1, 1, 1) MNY_WG(1, 1, 2) MNY_WG(1, 1, 3) MNY_WG(1, 1, 4) MNY_WG(1, 1, 5) MNY_WG(1, 1, 6) MNY_WG(1, 2, 1) MNY_WG(1, 2, 2) MNY_WG(1, 2, 3)
            MNY_WG(1, 3, 1) MNY_WG(1, 3, 2) MNY_WG(1, 4, 1) MNY_WG(1, 5, 1) MNY_WG(1, 6, 1)
            default: set_error("pw_wgrad: no kernel for mode %d tile %dx%d", pl.mode, pl.TI, pl.TJ); return MNY_EUNSUPPORTED;
        }
#undef MNY_WG
    }
    int rc = check_launch("pw_wgrad_kernel");
    if (rc) return rc;
    if (!dw) return MNY_OK;                         // partials only: the caller combines them (mny_reduce_batch)
    const int64_t n = (int64_t)Nc * K;
    hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, st, ws, pl.splits, n, dw);
    rc = check_launch("reduce_parts_kernel");
    if (rc) return rc;
    if (dbias) {
        const int parts = colsum_parts(M);
        float* cs = ws + (size_t)pl.splits * Nc * K;
        const int64_t rpb = cdiv(M, parts);
        hipLaunchKernelGGL((colsum_kernel<T>), dim3(parts, (unsigned)cdiv(Nc, 64)), dim3(256), 0, st, dy, cs, M, Nc, rpb);
        hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)cdiv(Nc, 32)), dim3(256), 0, st, cs, parts, (int64_t)Nc, dbias);
        rc = check_launch("colsum");
    }
    return rc;
}
extern "C" int mny_pw_wgrad(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* dy,
                            float* dw, float* dbias, float* ws, int64_t M, int K, int Nc, void* stream) {
    return pw_wgrad_impl<float>(x, in_scale, in_shift, in_act, dy, dw, dbias, ws, M, K, Nc, stream);
}
extern "C" int mny_pw_wgrad_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* dy,
                                 float* dw, float* dbias, float* ws, int64_t M, int K, int Nc, void* stream) {
    return pw_wgrad_impl<bf16_t>((const bf16_t*)x, in_scale, in_shift, in_act, (const bf16_t*)dy, dw, dbias, ws, M, K, Nc, stream);
}
