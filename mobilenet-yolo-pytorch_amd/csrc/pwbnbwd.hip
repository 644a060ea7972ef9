// Pointwise (1x1) convolution: the fused BatchNorm-backward + weight gradient + data gradient of the thin "expand" units (Cin <= 32), mny_pw_bnbwd*.
// Kernels (stage 1, fp64 finalize, the two data-gradient generations), plan, workspace layout and entry points; the algebra is under the banner
// below.  pw_bnbwd_finalize_launch (pwgemm.h) serves the producers of the same partial rows in exdw.hip, gate.hip and stemdw.hip; the combine
// in front of it is reduce_parts_kernel of pwwgrad.hip.  Both streaming stages are LDS-DMA pipelines like the weight-gradient kernels of pwwgrad.hip.
#include "pwgemm.h"
#include "x6.h"
#include "dma_zero.h"

namespace mny {

// ================================================================================================
// Fused BatchNorm-backward for HBM-bound "expand" pointwise units (Cin <= 32, one 32-wide tile).
//
// Unit: Y = X W^T, A = act(sc*Y + sh) with batch statistics; G = dL/dA.  With dz = G*act'(sc*Y+sh) and the
// per-channel BN-backward coefficients (ca, cb, cc):  dY = ca*dz + cb*Y + cc.  Hence
//     dW = ca o (dz^T X) + cb o (W X^T X) + cc (x) colsum(X)          (Y^T X = W X^T X)
//     dX = dz (ca o W) + Y (cb o W) + (cc . W)
// so dY is never materialised and the unit's big output tensor is read 4 times instead of 7:
//   stage 1 (one pass over G, Y, X): sum dz, sum dz*yhat, P1 = dz^T X, Gram = X^T X, colsum(X)
//   finalize (tiny, fp64)          : dgamma, dbeta, ca/cb/cc, dW, B1 = ca o W^T, B2 = cb o W^T, bias = cc . W
//   stage 2 (one pass over G, Y)   : dX = dz B1^T + Y B2^T + bias (+ addend)
// Both streaming stages are LDS-DMA pipelines like the kernels above.
// ================================================================================================
struct BnwArgs {
    const float* G; const float* Y; const float* sc; const float* sh; int act; const float* mean; const float* invstd;
    const float* X; const float* xsc; const float* xsh; int xact;
    float* partial; unsigned long long* mask;   // mask[i*npairs + m/2]: bit (m&1)*32 + c%32 = [act'(z) is the "on" value]
    int64_t npairs; int64_t M; int K; int N; int64_t rows_per_block;
    int tiles_total;    // ceil(N/32); blockIdx.y selects a slice of TI column tiles (wide units run as two slices: occupancy)
};

// partial layout per split: P1[N*K] | Gram[K*K] | s1[N] | s2[N] | s3[K]   (bnw_stride: pwgemm.h — exdw.hip writes the same rows)

// Stage 1, second generation (round 3).  Same tiling, LDS-DMA ring, lane mapping, partial-row layout and arithmetic (order
// included: bit-identical results) as the first-generation stage 1 it replaced; what changed is the instruction stream.  The counters of the first
// generation (profiles/r03_pmc_pw_bnbwd.txt, 16 -> 96 @ 176x176) showed 15 scalar and 20 vector instructions per MFMA, 44 % of the
// wave cycles stalled at issue and the matrix pipe 30 % busy at 4.45 TB/s: every LDS read sat in its own basic block behind a
// `lane == 0` mask store (s_cbranch_execz + lgkmcnt(0) per read), the DMA issue went through per-instruction kind / range branches.
// Here the row loop body is ONE basic block: all 2 + 4 TI fragment reads of a stage are issued together, the ballots of a stage are
// kept in scalar registers and leave through one exec-masked group of 16-byte stores, the DMA sources are running pointers
// (select, not branch, for the rows past the slice), the Gram MFMA is unconditional (its column-slice twin is simply not stored).
// T: storage type of G, Y, X (float, or bf16_t for bf16-storage plans: the LDS image holds bf16, a 16-byte DMA chunk is 8 elements, the
// arithmetic is the same fp32; K % 8 == 0 and N % 8 == 0 there)
// S: ring depth.  A stage is 16 rows whatever the storage type, i.e. HALF the bytes with bf16 storage (2 x 5 KB per workgroup in flight at
// three stages; the bf16 instantiation runs 2.9 TB/s where the fp32 one runs 4.3-5.2).  Six stages were measured in round 5, same box: 15.24 / 15.24
// vs 15.20 / 15.25 ms — no gain, 3 stays: bytes in flight are not what holds this kernel back.
template <int TI, typename T = float, int S = 3>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void pw_bnbwd_stage1b_kernel(BnwArgs p) {
    constexpr int KC = 16, BI = 32 * TI, BJ = 32;
    constexpr int EPC = 16 / (int)sizeof(T), EPI = 64 * EPC;                  // elements per 16-byte chunk / per 1-KiB DMA instruction
    constexpr int G_ST = KC * BI, X_ST = KC * BJ, STAGE = 2 * G_ST + X_ST;   // elements of T: G | Y | X
    constexpr int NG = (G_ST + EPI - 1) / EPI, NX = (X_ST + EPI - 1) / EPI, NL = 2 * NG + NX;
    static_assert(G_ST % EPI == 0 && X_ST % EPI == 0, "whole DMA instructions per tile");
    constexpr int LPW = (NL + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    T* const smem = reinterpret_cast<T*>(smem_f);
    const T* const pG = reinterpret_cast<const T*>(p.G);
    const T* const pY = reinterpret_cast<const T*>(p.Y);
    const T* const pX = reinterpret_cast<const T*>(p.X);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, kk = lane >> 5;
    const int64_t m_begin = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t m_end = min(m_begin + p.rows_per_block, p.M);
    const bool has_xf = p.xsc != nullptr;
    const float xslope = act_slope(p.xact), xhi = act_hi(p.xact);
    const float aslope = act_slope(p.act), ahi = act_hi(p.act);
    const int krow0 = wave * (KC / 4);
    const int tile_off = blockIdx.y * TI, n_off = tile_off * 32;
    const bool slice0 = blockIdx.y == 0;

    float sc[TI], sh[TI], mu[TI], is[TI], s1[TI], s2[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int co = n_off + i * 32 + li;
        const bool ok = co < p.N;
        sc[i] = ok ? p.sc[co] : 0.f; sh[i] = ok ? p.sh[co] : 0.f; mu[i] = ok ? p.mean[co] : 0.f; is[i] = ok ? p.invstd[co] : 0.f;
        s1[i] = 0.f; s2[i] = 0.f;
    }
    const float xs = (has_xf && li < p.K) ? p.xsc[li] : 1.f, xh = (has_xf && li < p.K) ? p.xsh[li] : 0.f;
    float s3 = 0.f;

    // DMA instruction slots of this wave: a running source pointer per slot (row m_begin + d_row of its tensor), the clamp target
    // for rows past the slice (Y, X: the slice's last row — finite filler, its products are annihilated by dz = 0 / b = 0; G: zeros)
    const T* zero_src = reinterpret_cast<const T*>(&mny_zero16);
    const T* d_cur[LPW];
    const T* d_past[LPW];
    int d_row[LPW], d_lds[LPW], d_step[LPW];
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int j = wave + 4 * i;
        if (j >= NL) j = NL - 1;
        const int kind = j < NG ? 0 : (j < 2 * NG ? 1 : 2);              // 0: G, 1: Y, 2: X
        const int jj = kind == 0 ? j : (kind == 1 ? j - NG : j - 2 * NG);
        const int q = jj * 64 + lane;                                     // 16-byte chunk index inside the tile
        const int W4 = (kind == 2 ? BJ : BI) / EPC;
        d_row[i] = q / W4;
        const int c = (q % W4) * EPC;
        d_lds[i] = (kind == 0 ? 0 : (kind == 1 ? G_ST : 2 * G_ST)) + jj * EPI;
        const bool ok = kind == 2 ? c < p.K : n_off + c < p.N;
        const T* base = kind == 0 ? pG : (kind == 1 ? pY : pX);
        const int stride = kind == 2 ? p.K : p.N;
        const int off = kind == 2 ? c : n_off + c;
        d_cur[i] = ok ? base + (m_begin + d_row[i]) * stride + off : zero_src;
        d_past[i] = (ok && kind != 0) ? base + (m_end - 1) * stride + off : zero_src;
        d_step[i] = ok ? KC * stride : 0;
    }
    auto issue = [&](int64_t m0, int slot) {
        T* stage = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const T* src = (m0 + d_row[i] < m_end) ? d_cur[i] : d_past[i];
            d_cur[i] += d_step[i];
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(stage + d_lds[i]), 16, 0, 0);
        }
    };

    f32x16 acc[TI], gram;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) gram[r] = 0.f;

    auto compute = [&](int64_t m0, int slot) {
        const T* gb = smem + slot * STAGE + (krow0 + kk) * BI + li;
        const T* yb = gb + G_ST;
        const T* xb = smem + slot * STAGE + 2 * G_ST + (krow0 + kk) * BJ + li;
        float xr[KC / 8], gr[KC / 8][TI], yr[KC / 8][TI];
#pragma unroll
        for (int kp = 0; kp < KC / 8; ++kp) {                             // every fragment read of the stage, one wait
            xr[kp] = ld1(xb + kp * 2 * BJ);
#pragma unroll
            for (int i = 0; i < TI; ++i) { gr[kp][i] = ld1(gb + kp * 2 * BI + i * 32); yr[kp][i] = ld1(yb + kp * 2 * BI + i * 32); }
        }
        unsigned long long bal[KC / 8][TI];
#pragma unroll
        for (int kp = 0; kp < KC / 8; ++kp) {
            const bool rok = m0 + krow0 + kp * 2 + kk < m_end;
            const float xz = fmaf(xr[kp], xs, xh);
            const float b = rok ? fminf(fmaxf(xz, xslope * xz), xhi) : 0.f;     // rows past the slice contribute nothing
            s3 += b;
            float af[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const float g = gr[kp][i], y = yr[kp][i];
                const float z = fmaf(y, sc[i], sh[i]);
                const bool on = z > 0.f && z < ahi;                                // act' = on ? 1 : slope
                bal[kp][i] = __ballot(on);
                const float dz = on ? g : g * aslope;
                s1[i] += dz;
                s2[i] = fmaf(dz, (y - mu[i]) * is[i], s2[i]);
                af[i] = dz;
            }
#pragma unroll
            for (int i = 0; i < TI; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], b, acc[i], 0, 0, 0);
            gram = __builtin_amdgcn_mfma_f32_32x32x2f32(b, b, gram, 0, 0, 0);
        }
        // the stage's mask words (rows 2 pair, 2 pair + 1 <-> the two lane halves; kp = 0, 1 are consecutive pairs, pair0 is even):
        // one 16-byte store per column tile from lane 0
        if (lane == 0) {
            const int64_t pair0 = (m0 + krow0) >> 1;
            const bool full = m0 + krow0 + 2 < m_end;                              // both pairs of this wave start inside the slice
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                if (tile_off + i < p.tiles_total) {
                    unsigned long long* dstw = p.mask + (int64_t)(tile_off + i) * p.npairs + pair0;
                    if (full) *reinterpret_cast<ulonglong2*>(dstw) = make_ulonglong2(bal[0][i], bal[1][i]);
                    else if (m0 + krow0 < m_end) dstw[0] = bal[0][i];
                }
            }
        }
    };

    const int total = (int)((m_end - m_begin + KC - 1) / KC);
    int i_t = 0, i_slot = 0, c_slot = 0, c_t = 0;
    auto issue_next = [&]() { issue(m_begin + (int64_t)i_t * KC, i_slot); ++i_t; if (++i_slot == S) i_slot = 0; };
    auto consume = [&]() { compute(m_begin + (int64_t)c_t * KC, c_slot); ++c_t; if (++c_slot == S) c_slot = 0; };
    const int pre = total < S - 1 ? total : S - 1;
    for (int t = 0; t < pre; ++t) issue_next();
    for (int t = 0; t < total - pre; ++t) {
        wait_vmcnt<LPW*(S - 2)>();
        __builtin_amdgcn_s_barrier();
        issue_next();
        consume();
    }
    for (int t = 0; t < pre; ++t) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        consume();
    }

    // ---- block reduction over the 4 waves (fixed order) and the two k-halves, then one partial row (as the first generation)
    float* dst = p.partial + (int64_t)blockIdx.x * bnw_stride(p.N, p.K);
    float* red = smem_f;                       // [3][16][64]
    auto reduce_tile = [&](f32x16& t, float* out, int rows, int cols, int ld, int row0) {
        __syncthreads();
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = t[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = ((t[r] + red[(0 * 16 + r) * 64 + lane]) + red[(1 * 16 + r) * 64 + lane]) + red[(2 * 16 + r) * 64 + lane];
                const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                if (row < rows && li < cols) out[(int64_t)row * ld + li] = v;
            }
        }
    };
#pragma unroll
    for (int i = 0; i < TI; ++i) reduce_tile(acc[i], dst, p.N, p.K, p.K, n_off + i * 32);
    if (slice0) reduce_tile(gram, dst + (int64_t)p.N * p.K, p.K, p.K, p.K, 0);
    __syncthreads();
    float* vred = smem_f;                      // [4][2*TI+1][32]
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const float a = s1[i] + __shfl_xor(s1[i], 32), b2 = s2[i] + __shfl_xor(s2[i], 32);
        if (kk == 0) { vred[(wave * (2 * TI + 1) + i) * 32 + li] = a; vred[(wave * (2 * TI + 1) + TI + i) * 32 + li] = b2; }
    }
    {
        const float c3 = s3 + __shfl_xor(s3, 32);
        if (kk == 0) vred[(wave * (2 * TI + 1) + 2 * TI) * 32 + li] = c3;
    }
    __syncthreads();
    float* vdst = dst + (int64_t)p.N * p.K + (int64_t)p.K * p.K;
    for (int e = tid; e < (2 * TI + 1) * 32; e += 256) {
        const int v = e / 32, l = e % 32;
        float a = 0.f;
        for (int w = 0; w < 4; ++w) a += vred[(w * (2 * TI + 1) + v) * 32 + l];
        if (v < TI) { const int co = n_off + v * 32 + l; if (co < p.N) vdst[co] = a; }
        else if (v < 2 * TI) { const int co = n_off + (v - TI) * 32 + l; if (co < p.N) vdst[p.N + co] = a; }
        else if (l < p.K && slice0) vdst[2 * p.N + l] = a;
    }
}

static inline size_t bnw_finalize_lds(int N, int K) { return (size_t)3 * N * sizeof(double) + ((size_t)N * K + (size_t)K * K) * sizeof(float); }   // <= 33 KB (N <= 192, K <= 32)

// finalize.  red = [P1 | Gram | s1 | s2 | s3] summed over splits.  Every block recomputes the N coefficient triples (cheap) and
// takes a grid-stride share of the fp64 element loops (one block took 80 us per unit).
__global__ __launch_bounds__(256) void pw_bnbwd_finalize_kernel(const float* __restrict__ red, const float* __restrict__ W,
                                                                const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, double count, int N, int K,
                                                                float* __restrict__ dW, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ B1, float* __restrict__ Q, float* __restrict__ bias) {
    extern __shared__ double sd[];             // ca[N] cb[N] cc[N] | W[N][K] | Gram[K][K] (floats): the element loops below are serial
    double* ca = sd; double* cb = sd + N; double* cc = sd + 2 * N;          // fp64 chains over W and the Gram matrix; out of L2 they took 25 us per launch
    float* sW = reinterpret_cast<float*>(sd + 3 * N); float* sG = sW + N * K;
    for (int e = threadIdx.x; e < N * K; e += blockDim.x) sW[e] = W[e];
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) sG[e] = red[(int64_t)N * K + e];
    const float* P1 = red; const float* Gm = red + (int64_t)N * K; const float* s1 = Gm + (int64_t)K * K;
    const float* s2 = s1 + N; const float* s3 = s2 + N;
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const double a = (double)gamma[n] * (double)invstd[n];
        const double b = -a * (double)invstd[n] * (double)s2[n] / count;
        ca[n] = a; cb[n] = b; cc[n] = -a * (double)s1[n] / count - b * (double)mean[n];
        if (blockIdx.x == 0) { dbeta[n] = s1[n]; dgamma[n] = s2[n]; }
    }
    __syncthreads();
    for (int e = gtid; e < N * K; e += gsz) {
        const int n = e / K, k = e % K;
        double wg = 0.0;
        for (int j = 0; j < K; ++j) wg += (double)sW[n * K + j] * (double)sG[j * K + k];
        dW[e] = (float)(ca[n] * (double)P1[e] + cb[n] * wg + cc[n] * (double)s3[k]);
        B1[(int64_t)k * N + n] = (float)(ca[n] * (double)sW[e]);     // [K][N]: rows = dX columns, contraction over n
    }
    for (int e = gtid; e < K * K; e += gsz) {                         // Y (cb o W) = X (W^T diag(cb) W): Q[kc][k], symmetric
        const int kc = e / K, k = e % K;
        double a = 0.0;
        for (int n = 0; n < N; ++n) a += cb[n] * (double)sW[n * K + kc] * (double)sW[n * K + k];
        Q[e] = (float)a;
    }
    for (int k = gtid; k < K; k += gsz) {
        double a = 0.0;
        for (int n = 0; n < N; ++n) a += cc[n] * (double)sW[n * K + k];
        bias[k] = (float)a;
    }
}

// stage 2: dX[M,Kc] = dz[M,N] B1[Kc,N]^T + act(X)[M,Kc] Q[Kc,Kc]^T + bias (+addend), dz = G * (mask ? 1 : slope).
// Streams ONLY G (plus the 1-bit mask and the thin X).  Tile: 64 rows x 32-wide k-steps (full 128-B lines); waves
// 2 (row halves) x 2 (k-chunk parity), summed once per tile; the last k-step of every tile is the (X, Q) product.
struct BndArgs {
    const float* G; const unsigned long long* mask; int act;
    const float* X; const float* xsc; const float* xsh; int xact;
    const float* B1; const float* Q; const float* bias; const float* addend; float* C;
    int64_t npairs; int64_t M; int N; int Kc; int TI; int m_tiles, tiles_per_block;
    // RED (pw_bnbwd_dgrad2_kernel<.., true>, round 6): C is the complete output gradient of the conv+BN+act unit whose raw output is rY: its
    // BN-backward sums leave as one partial row per workgroup, red[gridDim.x][2][Kc]
    const float* rY; const float* r_scale; const float* r_shift; const float* r_mean; const float* r_invstd; int r_act; float* red;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void pw_bnbwd_dgrad_kernel(BndArgs p) {
    constexpr int BMS = 64, BKD = 32, S = 3;
    constexpr int A_ST = BMS * BKD, B_ST = 32 * BKD, STAGE = A_ST + B_ST;            // G(or X) | B1(or Q)   (12 KB)
    constexpr int NA = A_ST / 256, NB = B_ST / 256, NL = NA + NB;                    // 8 + 4
    constexpr int LPW = NL / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int nkg = (p.N + BKD - 1) / BKD, nk = nkg + 1;                             // + the (X, Q) step
    float* sXs = smem + S * STAGE;                                                   // [32] input-view scale / shift
    float* sXh = sXs + 32;
    float* xred = sXh + 32;                                                          // [2][16][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wk = wv & 1;
    const int lrow = lane & 31, khalf = lane >> 5;
    if (tid < 32) {
        sXs[tid] = (p.xsc && tid < p.Kc) ? p.xsc[tid] : (tid < p.Kc ? 1.f : 0.f);
        sXh[tid] = (p.xsc && tid < p.Kc) ? p.xsh[tid] : 0.f;
    }
    const int mt_begin = blockIdx.x * p.tiles_per_block;
    const int mt_end = min(mt_begin + p.tiles_per_block, p.m_tiles);
    const int total = (mt_end - mt_begin) * nk;

    const float* zero_src = reinterpret_cast<const float*>(&mny_zero16);
    const int drow = lane >> 3, dpos = lane & 7;
    int d_row[LPW], d_k[LPW], d_lds[LPW], d_kind[LPW];           // kind 0: streamed operand, 1: weights, 2: mask words
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        int j = wv + 4 * i;
        if (j >= NL) j = NL - 1;
        d_kind[i] = j < NA ? 0 : (j < NA + NB ? 1 : 2);
        const int jj = d_kind[i] == 0 ? j : j - NA;
        const int row = jj * 8 + drow;
        d_row[i] = row;
        d_k[i] = (dpos ^ (row & 7)) * 4;
        d_lds[i] = d_kind[i] == 2 ? A_ST + B_ST : (d_kind[i] == 0 ? 0 : A_ST) + jj * 256;
    }
    auto issue = [&](int mt, int kt, int slot) {
        float* stage = smem + slot * STAGE;
        const bool xstep = kt == nkg;
        const int width = xstep ? p.Kc : p.N;                 // row length of the streamed operand / contraction length
        const int k0 = xstep ? 0 : kt * BKD;
#pragma unroll
        for (int i = 0; i < LPW; ++i) {
            const int k = k0 + d_k[i];
            const bool kok = k < width;
            const float* src;
            if (d_kind[i] == 0) {
                int m = mt * BMS + d_row[i];
                if (m >= (int)p.M) m = (int)p.M - 1;
                src = (xstep ? p.X : p.G) + (int64_t)m * width + (kok ? k : 0);
            } else if (d_kind[i] == 1) {
                const int n = d_row[i];
                src = (n < p.Kc && kok) ? (xstep ? p.Q : p.B1) + (int64_t)n * width + k : zero_src;
            } else {
                src = zero_src;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(stage + d_lds[i]), 16, 0, 0);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int swz = lrow & 7;
    const float aslope = act_slope(p.act);
    const float xslope = act_slope(p.xact), xhi = act_hi(p.xact);
    // The act' mask word of a step is an ordinary global load.  Loaded where it is used, the compiler has to drain the whole
    // VM queue (vmcnt(0)) in front of it — including the DMA stages just issued — so every step exposed a full memory latency
    // (2.5 TB/s).  It is therefore fetched ONE STEP AHEAD, before that step's DMA batch is issued: by the time it is consumed
    // the counted wait at the top of the next iteration has already covered it and the ring stays two stages deep.
    // (Staging the words through the DMA ring instead was measured slower: 2.13 vs 1.74 ms on the 16->96 unit.)
    auto compute = [&](int mt, int kt, int slot, unsigned long long mw) {
        const float* st = smem + slot * STAGE;
        const float* a_row = st + (wm * 32 + lrow) * BKD;
        const float* b_row = st + A_ST + lrow * BKD;
        const bool xstep = kt == nkg;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const int chunk = (kc * 2 + wk) * 2 + khalf;
            const int o = (chunk ^ swz) << 2;
            v4f_t a = lds_read_f4(a_row + o);                      // raw LDS reads: see "LDS reads the compiler cannot see"
            v4f_t b = lds_read_f4(b_row + o);
            v4f_t xs = lds_read_f4(sXs + chunk * 4), xh = lds_read_f4(sXh + chunk * 4);
            MNY_LGKM_WAIT(a);
            MNY_LGKM_DEP(b); MNY_LGKM_DEP(xs); MNY_LGKM_DEP(xh);
            if (xstep) {
                float z;
                z = fmaf(a.x, xs.x, xh.x); a.x = fminf(fmaxf(z, xslope * z), xhi);
                z = fmaf(a.y, xs.y, xh.y); a.y = fminf(fmaxf(z, xslope * z), xhi);
                z = fmaf(a.z, xs.z, xh.z); a.z = fminf(fmaxf(z, xslope * z), xhi);
                z = fmaf(a.w, xs.w, xh.w); a.w = fminf(fmaxf(z, xslope * z), xhi);
            } else {
                const unsigned bits = (unsigned)(mw >> (chunk * 4)) & 15u;
                a.x = (bits & 1u) ? a.x : a.x * aslope; a.y = (bits & 2u) ? a.y : a.y * aslope;
                a.z = (bits & 4u) ? a.z : a.z * aslope; a.w = (bits & 8u) ? a.w : a.w * aslope;
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    };
    // Epilogue: the two k-parity waves of a row half are summed through LDS; the owner then transposes each group of 4
    // accumulator registers across its lane quad (DPP butterfly, as in the NT kernel) so a lane holds 4 consecutive output
    // columns of one row: 4 float4 addend loads + 4 float4 stores per tile instead of 16 dependent scalar load -> wait ->
    // store chains.  Nothing here may make hipcc drain the VM queue (the next tiles' DMA stages are already in flight):
    //   * the LDS exchange uses raw ds_write_b128 / ds_read_b128 + explicit lgkmcnt + raw s_barrier (a compiler-visible LDS
    //     access, or __syncthreads, waits vmcnt(0));
    //   * the tile's addend rows are fetched by raw global_load_dwordx4 when the tile's FIRST k-step is consumed, i.e. before
    //     the following stages' DMA batches — VM loads retire in order, so the counted waits of the next steps cover them;
    //   * the bias vector is loaded once, before the pipeline starts.
    const int quad = lrow >> 2, jq = lane & 3;
    const int colq = quad * 4;
    const bool cok = colq < p.Kc;                                  // Kc % 4 == 0: all four columns or none
    const int colc = cok ? colq : 0;
    const float4 bv = ld4(p.bias + colc);
    float* xr_w = xred + ((wm * 4) * 64 + lane) * 4;               // [wm][q][lane][4]: lane-contiguous 16-B slots
    v4f_t ad0, ad1, ad2, ad3;
    auto addend_fetch = [&](int mt) {                              // raw loads: see above
        const int64_t m0 = (int64_t)mt * BMS + wm * 32 + 4 * khalf + jq;
        const float* a0 = p.addend + min(m0, p.M - 1) * p.Kc + colc;
        const float* a1 = p.addend + min(m0 + 8, p.M - 1) * p.Kc + colc;
        const float* a2 = p.addend + min(m0 + 16, p.M - 1) * p.Kc + colc;
        const float* a3 = p.addend + min(m0 + 24, p.M - 1) * p.Kc + colc;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(ad0) : "v"(a0) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(ad1) : "v"(a1) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(ad2) : "v"(a2) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(ad3) : "v"(a3) : "memory");
    };
    auto epilogue = [&](int mt) {
        if (wk == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v4f_t v = {acc[q * 4 + 0], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]};
                asm volatile("ds_write_b128 %0, %1" : : "v"(lds_off(xr_w + q * 256)), "v"(v) : "memory");
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wk == 0) {
            v4f_t xq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) xq[q] = lds_read_f4(xr_w + q * 256);
            MNY_LGKM_WAIT(xq[0]);
            MNY_LGKM_DEP(xq[1]); MNY_LGKM_DEP(xq[2]); MNY_LGKM_DEP(xq[3]);
            if (p.addend) { MNY_LGKM_DEP(ad0); MNY_LGKM_DEP(ad1); MNY_LGKM_DEP(ad2); MNY_LGKM_DEP(ad3); }
            const int64_t m0 = (int64_t)mt * BMS;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float r0 = acc[gq * 4 + 0] + xq[gq].x, r1 = acc[gq * 4 + 1] + xq[gq].y;
                float r2 = acc[gq * 4 + 2] + xq[gq].z, r3 = acc[gq * 4 + 3] + xq[gq].w;
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
                const v4f_t ad = gq == 0 ? ad0 : (gq == 1 ? ad1 : (gq == 2 ? ad2 : ad3));
                float4 o = make_float4(r0 + bv.x, r1 + bv.y, r2 + bv.z, r3 + bv.w);
                if (p.addend) { o.x += ad.x; o.y += ad.y; o.z += ad.z; o.w += ad.w; }
                const int64_t row = m0 + wm * 32 + 8 * gq + 4 * khalf + jq;
                if (cok && row < p.M) st4_stream(p.C + row * p.Kc + colq, o);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                              // the exchange buffer may be rewritten by the next tile
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    };
    __syncthreads();
    int i_mt = mt_begin, i_kt = 0, i_slot = 0, c_mt = mt_begin, c_kt = 0, c_slot = 0;
    auto issue_next = [&]() { issue(i_mt, i_kt, i_slot); if (++i_kt == nk) { i_kt = 0; ++i_mt; } if (++i_slot == S) i_slot = 0; };
    // Software pipeline.  The mask word of the NEXT step is fetched with a raw `global_load_dwordx2` (inline asm) placed before
    // that step's DMA batch; the counted wait at the END of the iteration (all but the newest LPW VM operations retired — VM
    // loads retire in issue order) covers it, and only then is it moved into the register the next iteration consumes.  Load,
    // wait and move are volatile asm statements, so their order is fixed and the compiler — which would otherwise put a
    // vmcnt(0) in front of any use of an ordinary load's result and drain the DMA ring every step — never sees a pending load.
    unsigned long long m_next = 0ull, m_cur = 0ull;
    auto mask_fetch = [&](int mt, int kt) {
        const int64_t row = min((int64_t)mt * BMS + wm * 32 + lrow, p.M - 1);
        const int kc = min(kt, nkg - 1);
        const unsigned long long* ptr = p.mask + (int64_t)kc * p.npairs + (row >> 1);
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(m_next) : "v"(ptr) : "memory");
    };
    auto mask_commit = [&]() { asm volatile("v_mov_b64 %0, %1" : "=v"(m_cur) : "v"(m_next)); };
    auto mask_word = [&](int mt) -> unsigned long long {                    // the row's 32 bits of the committed pair word
        const int64_t row = min((int64_t)mt * BMS + wm * 32 + lrow, p.M - 1);
        return m_cur >> ((row & 1) * 32);
    };
    auto consume = [&]() {
        compute(c_mt, c_kt, c_slot, mask_word(c_mt));
        if (++c_kt == nk) { epilogue(c_mt); c_kt = 0; ++c_mt; }
        if (++c_slot == S) c_slot = 0;
    };
    // addend rows of tile `mt` are requested when the loop is about to consume the tile's first step (before that
    // iteration's DMA batch): nk >= 2 steps and their counted waits lie between the request and the epilogue
    auto maybe_fetch_addend = [&]() { if (p.addend && c_kt == 0 && wk == 0) addend_fetch(c_mt); };
    auto fetch_next = [&](bool more) {                                        // mask of the step AFTER the one about to be consumed
        int n_kt = c_kt + 1, n_mt = c_mt;
        if (n_kt == nk) { n_kt = 0; ++n_mt; }
        if (!more) { n_mt = c_mt; n_kt = c_kt; }                              // past the end: re-read a valid word (unused)
        mask_fetch(n_mt, n_kt);
    };
    if (total <= 0) return;
    mask_fetch(c_mt, c_kt);                                                   // oldest entry of the VM queue
    const int pre = total < S - 1 ? total : S - 1;
    for (int t = 0; t < pre; ++t) issue_next();
    const int steady = total - pre;
    if (steady > 0) wait_vmcnt<LPW*(S - 2)>(); else wait_vmcnt<0>();
    mask_commit();
    for (int t = 0; t < steady; ++t) {
        __builtin_amdgcn_s_barrier();                    // every wave's share of the stage to consume has landed
        fetch_next(t + 1 < total);
        maybe_fetch_addend();
        issue_next();
        consume();
        if (t + 1 < steady) wait_vmcnt<LPW*(S - 2)>(); else wait_vmcnt<0>();
        mask_commit();
    }
    for (int t = 0; t < pre; ++t) {
        __builtin_amdgcn_s_barrier();
        fetch_next(steady + t + 1 < total);
        maybe_fetch_addend();
        wait_vmcnt<0>();                                 // drain phase: nothing newer is worth keeping in flight
        consume();
        mask_commit();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// stage 2, second generation: no LDS ring, no barrier in the loop.
// The DMA-ring kernel above streams G at 3.9 TB/s: a 64-row step is 12 KB per workgroup behind a barrier, two of them in flight,
// and the matrix pipe idles on memory latency (replacing its MFMAs by the six-product bf16 form changed nothing).  A wave can
// instead load the A operand of v_mfma_f32_32x32x16_bf16 STRAIGHT from the row-major tensor — lane (row i, half h) owns, per
// 16-column stage, the two 16-B chunks 16s + 4h.. and 16s + 8 + 4h.. of row i — and that access pattern streams at the copy rate
// (tools/probe/rowfrag_probe.hip: 5.3-5.5 TB/s for N = 96 / 144 / 192, as fast as a row-linear float4 stream).  So: one wave =
// one 32-row tile at a time, all of its G fragments (2 * N/16 float4 per lane) in registers, each pair re-requested for the wave's
// NEXT tile the moment it has been cut (rolling prefetch: a full tile of loads always in flight, one buffer); the small operands
// (B1 = ca o W^T [Kc][N], Q [Kc][Kc]) are cut into bf16 planes ONCE per workgroup into LDS in MFMA-operand order; products in the
// six-product form (x6_split), two accumulators (even / odd stages); epilogue = the DPP quad transpose of the first generation.
// N % 16 == 0, N <= 192, Kc <= 32.
// ---------------------------------------------------------------------------------------------------------------------
// T: storage type of G, X, the addend and dX (bf16_t for bf16-storage plans: 8-byte loads widened to fp32, the same cuts and products —
// the bf16-exact G has empty mid / lo pieces, which costs matrix-pipe cycles this HBM-bound kernel has to spare — one RNE on store).
// HALF: N = 16 NS - 8 (the last stage's upper eight columns do not exist: N = 72 of MobileNetV3).
template <int NS, typename T = float, bool HALF = false, bool RED = false>
__global__ __launch_bounds__(256) void pw_bnbwd_dgrad2_kernel(BndArgs p) {
    constexpr int N = NS * 16 - (HALF ? 8 : 0), NW = (N + 31) / 32;               // mask words (32 columns each) per row
    const T* const pG = reinterpret_cast<const T*>(p.G);
    const T* const pX = reinterpret_cast<const T*>(p.X);
    const T* const pAd = reinterpret_cast<const T*>(p.addend);
    T* const pC = reinterpret_cast<T*>(p.C);
    __shared__ __attribute__((aligned(16))) float sB[(NS + 2) * 3 * 256];     // [stage][piece][lane] 16-B slots; stages NS, NS+1 = Q
    __shared__ __attribute__((aligned(16))) float sXs[32];
    __shared__ __attribute__((aligned(16))) float sXh[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, khalf = lane >> 5;
    const int Kc = p.Kc;
    const int XS = (Kc + 15) / 16;                               // stages of the (X, Q) product
    // ---- cut the small operands once per workgroup ----
    for (int c = tid; c < (NS + 2) * 64; c += 256) {
        const int sidx = c >> 6, l = c & 63, j = l & 31, h = l >> 5;
        const bool isq = sidx >= NS;
        const int st = isq ? sidx - NS : sidx;
        const int width = isq ? Kc : N;
        const float* src = (isq ? p.Q : p.B1) + (int64_t)j * width;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = st * 16 + (e < 4 ? 4 * h + e : 8 + 4 * h + (e - 4));
            v[e] = (j < Kc && k < width) ? src[k] : 0.f;
        }
        bf16x8_t hh, mm, ll;
        x6_split(v4f_t{v[0], v[1], v[2], v[3]}, v4f_t{v[4], v[5], v[6], v[7]}, hh, mm, ll);
        float* dst = sB + (sidx * 3) * 256 + l * 4;
        *reinterpret_cast<v4f_t*>(dst) = __builtin_bit_cast(v4f_t, hh);
        *reinterpret_cast<v4f_t*>(dst + 256) = __builtin_bit_cast(v4f_t, mm);
        *reinterpret_cast<v4f_t*>(dst + 512) = __builtin_bit_cast(v4f_t, ll);
    }
    if (tid < 32) {
        sXs[tid] = (p.xsc && tid < Kc) ? p.xsc[tid] : (tid < Kc ? 1.f : 0.f);
        sXh[tid] = (p.xsc && tid < Kc) ? p.xsh[tid] : 0.f;
    }
    __syncthreads();
    const float aslope = act_slope(p.act), xslope = act_slope(p.xact), xhi = act_hi(p.xact);
    const int quad = lrow >> 2, jq = lane & 3;
    const int colq = quad * 4;
    const bool cok = colq < Kc;
    const int colc = cok ? colq : 0;
    const float4 bv = ld4(p.bias + colc);
    float4 rsc = f4one(), rsh = f4zero(), rmu = f4zero(), ris = f4zero(), rs1 = f4zero(), rs2 = f4zero();
    if constexpr (RED) { rsc = ld4(p.r_scale + colc); rsh = ld4(p.r_shift + colc); rmu = ld4(p.r_mean + colc); ris = ld4(p.r_invstd + colc); }
    const float rslope = act_slope(p.r_act), rhi = act_hi(p.r_act);
    const unsigned* mask32 = reinterpret_cast<const unsigned*>(p.mask);
    const int64_t mstride = 2 * p.npairs;                        // 32-bit mask words per 32-column tile

    const int64_t ntiles = (p.M + 31) / 32;
    const int64_t stride = (int64_t)gridDim.x * 4;
    float4 g[2 * NS], xr[4], ad[4];
    unsigned mk[NW];
    auto row_of = [&](int64_t tile) { const int64_t r = tile * 32 + lrow; return r < p.M ? r : p.M - 1; };
    auto load_g = [&](int64_t tile, int s) {
        const T* row = pG + row_of(tile) * N + 16 * s + 4 * khalf;
        g[2 * s] = ld4(row);
        if (HALF && s == NS - 1) g[2 * s + 1] = f4zero(); else g[2 * s + 1] = ld4(row + 8);
    };
    auto load_mx = [&](int64_t tile) {                           // mask words and the thin X row of the lane
        const int64_t r = row_of(tile);
#pragma unroll
        for (int w = 0; w < NW; ++w) mk[w] = mask32[(int64_t)w * mstride + r];
        const T* xrow = pX + r * Kc + 4 * khalf;
        xr[0] = ld4(xrow); xr[1] = (8 + 4 * khalf < Kc) ? ld4(xrow + 8) : f4zero();
        xr[2] = (16 + 4 * khalf < Kc) ? ld4(xrow + 16) : f4zero(); xr[3] = (24 + 4 * khalf < Kc) ? ld4(xrow + 24) : f4zero();
    };
    auto load_ad = [&](int64_t tile) {
        if (p.addend) {
            const int64_t m0 = tile * 32 + 4 * khalf + jq;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) { const int64_t r2 = m0 + 8 * gq; ad[gq] = ld4(pAd + (r2 < p.M ? r2 : p.M - 1) * Kc + colc); }
        }
    };
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) {
#pragma unroll
        for (int s = 0; s < NS; ++s) load_g(tile, s);
        load_mx(tile);
        load_ad(tile);
    }
    for (; tile < ntiles; tile += stride) {
        const int64_t next = tile + stride < ntiles ? tile + stride : tile;      // past the end: harmless re-reads
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 a0 = g[2 * s], a1 = g[2 * s + 1];
            const unsigned word = mk[s >> 1] >> (16 * (s & 1) + 4 * khalf);
            float z[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                z[e] = ((word >> e) & 1u) ? z[e] : z[e] * aslope;
                z[4 + e] = ((word >> (8 + e)) & 1u) ? z[4 + e] : z[4 + e] * aslope;
            }
            bf16x8_t ah, am, al;
            x6_split(v4f_t{z[0], z[1], z[2], z[3]}, v4f_t{z[4], z[5], z[6], z[7]}, ah, am, al);
            // this stage's registers are free: request them for the next tile — HERE, not earlier: without the fence the compiler hoists every
            // load of the next tile to the top of the loop (SSA renames the registers) and the kernel needs two tiles of them (435 VGPRs)
            asm volatile("" : "+v"(ah), "+v"(am), "+v"(al) :: "memory");
            load_g(next, s);
            const float* bsrc = sB + (s * 3) * 256 + lane * 4;
            const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc));
            const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc + 256));
            const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc + 512));
            f32x16& acc = (s & 1) ? acc1 : acc0;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                   // stages in order: the cuts of later stages would otherwise all be formed first
        }
        // the (act(X), Q) product
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            if (st < XS) {
                const float4 a0 = xr[2 * st], a1 = xr[2 * st + 1];
                float z[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float4 s0 = *reinterpret_cast<const float4*>(sXs + st * 16 + 4 * khalf), s1 = *reinterpret_cast<const float4*>(sXs + st * 16 + 8 + 4 * khalf);
                const float4 h0 = *reinterpret_cast<const float4*>(sXh + st * 16 + 4 * khalf), h1 = *reinterpret_cast<const float4*>(sXh + st * 16 + 8 + 4 * khalf);
                const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float t = fmaf(z[e], sv[e], hv[e]); z[e] = fminf(fmaxf(t, xslope * t), xhi); }
                bf16x8_t ah, am, al;
                x6_split(v4f_t{z[0], z[1], z[2], z[3]}, v4f_t{z[4], z[5], z[6], z[7]}, ah, am, al);
                const float* bsrc = sB + ((NS + st) * 3) * 256 + lane * 4;
                const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc));
                const bf16x8_t bm = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc + 256));
                const bf16x8_t bl = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const v4f_t*>(bsrc + 512));
                f32x16& acc = st ? acc1 : acc0;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            }
        }
        asm volatile("" : "+v"(acc0), "+v"(acc1) :: "memory");     // (the next tile's small loads stay behind the last use of this tile's)
        load_mx(next);
        // epilogue: lane = output column lrow, registers = rows; DPP quad transpose -> lane jq of a quad holds row 8 gq + 4 khalf + jq, 4 columns
        const int64_t m0 = tile * 32;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            float r0 = acc0[gq * 4 + 0] + acc1[gq * 4 + 0], r1 = acc0[gq * 4 + 1] + acc1[gq * 4 + 1];
            float r2 = acc0[gq * 4 + 2] + acc1[gq * 4 + 2], r3 = acc0[gq * 4 + 3] + acc1[gq * 4 + 3];
            {
                const bool odd = lane & 1;
                const float xa = odd ? r0 : r1, xb = odd ? r2 : r3;
                const float ya = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xa), 0xB1, 0xF, 0xF, true));
                const float yb = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xb), 0xB1, 0xF, 0xF, true));
                if (odd) { r0 = ya; r2 = yb; } else { r1 = ya; r3 = yb; }
            }
            {
                const bool hi2 = lane & 2;
                const float xa = hi2 ? r0 : r2, xb = hi2 ? r1 : r3;
                const float ya = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xa), 0x4E, 0xF, 0xF, true));
                const float yb = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, xb), 0x4E, 0xF, 0xF, true));
                if (hi2) { r0 = ya; r1 = yb; } else { r2 = ya; r3 = yb; }
            }
            float4 o = make_float4(r0 + bv.x, r1 + bv.y, r2 + bv.z, r3 + bv.w);
            if (p.addend) {
                // scalar adds, spelled out: left to the compiler the bf16 instantiations get v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0]
                // (the addend's widened halves sit swapped in their register pair) for row groups 2 and 3, and on MI355X exactly those
                // sums came out WITHOUT the addend in lanes 48-63 of a few waves per launch, differently from launch to launch
                // (tools/ab/stress_bnbwd_bf16.py; the registers themselves were intact — DESIGN.md, round 3)
                asm("v_add_f32 %0, %0, %1" : "+v"(o.x) : "v"(ad[gq].x)); asm("v_add_f32 %0, %0, %1" : "+v"(o.y) : "v"(ad[gq].y));
                asm("v_add_f32 %0, %0, %1" : "+v"(o.z) : "v"(ad[gq].z)); asm("v_add_f32 %0, %0, %1" : "+v"(o.w) : "v"(ad[gq].w));
            }
            const int64_t row = m0 + 8 * gq + 4 * khalf + jq;
            if (cok && row < p.M) st4_stream(pC + row * Kc + colq, o);
            if constexpr (RED) {                                     // sums over the STORED gradient of the unit in front (its raw output row: a thin 16-B load)
                if (cok && row < p.M) {
                    const float4 yv = ld4(reinterpret_cast<const float*>(p.rY) + row * Kc + colq);
                    const float ov[4] = {o.x, o.y, o.z, o.w}, yy[4] = {yv.x, yv.y, yv.z, yv.w};
                    const float sc4[4] = {rsc.x, rsc.y, rsc.z, rsc.w}, sh4[4] = {rsh.x, rsh.y, rsh.z, rsh.w};
                    const float mu4[4] = {rmu.x, rmu.y, rmu.z, rmu.w}, is4[4] = {ris.x, ris.y, ris.z, ris.w};
                    float a1[4] = {rs1.x, rs1.y, rs1.z, rs1.w}, a2[4] = {rs2.x, rs2.y, rs2.z, rs2.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float z = fmaf(yy[e], sc4[e], sh4[e]);
                        const float dz = ov[e] * ((z > 0.f ? 1.f : rslope) * (z < rhi ? 1.f : 0.f));
                        a1[e] += dz;
                        a2[e] = fmaf(dz, (yy[e] - mu4[e]) * is4[e], a2[e]);
                    }
                    rs1 = make_float4(a1[0], a1[1], a1[2], a1[3]); rs2 = make_float4(a2[0], a2[1], a2[2], a2[3]);
                }
            }
        }
        asm volatile("" ::: "memory");
        load_ad(next);
    }
    if constexpr (RED) {                                             // one partial row per workgroup: the eight lanes of a column quad, then the four waves, fixed order
        __syncthreads();
        float4* sr = reinterpret_cast<float4*>(sB);                  // [2][256]
        sr[tid] = rs1; sr[256 + tid] = rs2;
        __syncthreads();
        if (tid < 16 && tid * 4 < Kc) {                              // thread = column quad
            float4 a = f4zero(), b = f4zero();
            for (int w = 0; w < 4; ++w)
                for (int h = 0; h < 2; ++h)
                    for (int j = 0; j < 4; ++j) {
                        const int l = w * 64 + h * 32 + tid * 4 + j;
                        add4(a, sr[l]); add4(b, sr[256 + l]);
                    }
            float* dst = p.red + (int64_t)blockIdx.x * 2 * Kc;
            st4(dst + tid * 4, a);
            st4(dst + Kc + tid * 4, b);
        }
    }
}

struct BnwPlan { int TI, splits; int64_t rows_per_block; size_t lds1, lds2; int gx2, tiles_per_block, m_tiles; int TIs, nsl; };

static bool bnw_supported(int64_t M, int K, int N) {
    return M >= 4096 && K <= 32 && K % 4 == 0 && N % 4 == 0 && N <= 192 && N > K;
}

static BnwPlan bnw_plan(int64_t M, int K, int N) {
    BnwPlan pl;
    pl.TI = (int)cdiv(N, 32);
    // whole waves of resident workgroups: TI <= 3 -> 168 VGPRs, 3 per CU (768); TI 4,5 -> 2 per CU (512); TI 6 -> 1 per CU
    // stage 1 of a wide unit (5 or 6 column tiles: 225+ VGPRs, 1-2 workgroups per CU) runs as two column slices of <= 3 tiles
    // (168 VGPRs, 3 per CU): each slice streams its half of G and Y and all of the thin X
    pl.nsl = pl.TI >= 5 ? 2 : 1;
    pl.TIs = (int)cdiv(pl.TI, pl.nsl);
    int64_t splits = (pl.TIs <= 3 ? 768 : 1024) / pl.nsl;
    const int64_t max_splits = cdiv(M, 64);
    if (splits > max_splits) splits = max_splits;
    pl.rows_per_block = cdiv(cdiv(M, splits), 16) * 16;
    pl.splits = (int)cdiv(M, pl.rows_per_block);
    pl.lds1 = (size_t)3 * 16 * (2 * 32 * pl.TIs + 32) * sizeof(float);
    const size_t need = (size_t)4 * (2 * pl.TIs + 1) * 32 * sizeof(float);
    if (pl.lds1 < need) pl.lds1 = need;
    if (pl.lds1 < 3 * 16 * 64 * sizeof(float)) pl.lds1 = 3 * 16 * 64 * sizeof(float);
    pl.lds2 = (size_t)3 * (64 * 32 + 32 * 32) * sizeof(float) + 64 * sizeof(float) + 2 * 16 * 64 * sizeof(float);
    pl.m_tiles = (int)cdiv(M, 64);
    int gx = pl.m_tiles < 768 ? pl.m_tiles : 768;
    pl.tiles_per_block = (int)cdiv(pl.m_tiles, gx);
    pl.gx2 = (int)cdiv(pl.m_tiles, pl.tiles_per_block);
    return pl;
}

// combine + finalize of the fused expand-unit backward, also for the producers outside this file (exdw.hip, gate.hip, stemdw.hip): partial rows in the layout above
int pw_bnbwd_finalize_launch(const float* partials, int nparts, float* red, const float* w, const float* gamma, const float* mean,
                             const float* invstd, int64_t M, int Nc, int K, float* dw, float* dgamma, float* dbeta, float* B1, float* Q,
                             float* bias, hipStream_t st) {
    const int64_t stride = bnw_stride(Nc, K);
    reduce_parts_launch(partials, nparts, stride, red, st);
    hipLaunchKernelGGL(pw_bnbwd_finalize_kernel, dim3((unsigned)cdiv((int64_t)Nc * K, 256)), dim3(256), bnw_finalize_lds(Nc, K), st, red, w, gamma,
                       mean, invstd, (double)M, Nc, K, dw, dgamma, dbeta, B1, Q, bias);
    return check_launch("pw_bnbwd_finalize_kernel");
}

}  // namespace mny

using namespace mny;

// ---- fused BN-backward + wgrad + dgrad for thin "expand" units ------------------------------------------------
extern "C" int mny_pw_bnbwd_supported(int64_t M, int K, int Nc) { return bnw_supported(M, K, Nc) ? 1 : 0; }

// the workspace of mny_pw_bnbwd[_bf16]: partials [splits] | reduced row | B1 | Q | bias | 1-bit activation mask (npairs * TI 64-bit words)
struct BnwWs { size_t red, B1, Q, bias, mask; int64_t npairs; size_t floats; };      // offsets and the total, in floats
static BnwWs bnw_ws(const BnwPlan& pl, int64_t M, int K, int Nc) {
    const size_t stride = (size_t)bnw_stride(Nc, K);
    const size_t red = (size_t)pl.splits * stride, B1 = red + stride, Q = B1 + (size_t)Nc * K, bias = Q + (size_t)K * K;
    const size_t mask = (bias + 64 + 15) / 16 * 16;                    // 64-byte aligned mask words
    const int64_t npairs = (M / 2 + 66) / 2 * 2;                       // even (16-B aligned rows of words) + a tile of slack
    return {red, B1, Q, bias, mask, npairs, bias + 64 + 64 + (size_t)npairs * pl.TI * 2};
}
extern "C" size_t mny_pw_bnbwd_ws_floats(int64_t M, int K, int Nc) {
    if (!bnw_supported(M, K, Nc)) return 0;
    // the wave form of bf16 storage (gate.hip) lays its own buffers out in the same workspace: the larger of the two
    const size_t base = bnw_ws(bnw_plan(M, K, Nc), M, K, Nc).floats;
    const size_t wave = pwe_ok(M, K, Nc) ? pwe_ws_floats(M, K, Nc) : 0;
    return base > wave ? base : wave;
}

static bool bnw_red_ok(int64_t M, int K, int Nc) {      // the data-gradient stage that can carry the sums of the unit in front: the barrier-free second generation
    return bnw_supported(M, K, Nc) && (Nc == 96 || Nc == 144 || Nc == 192);
}
constexpr int kBndGrid = 512;      // workgroups of the barrier-free data-gradient stage: two per CU
static int bnw_red_grid(int64_t M) {
    const int64_t tiles = cdiv(M, 32);
    return (int)(cdiv(tiles, 4) < kBndGrid ? cdiv(tiles, 4) : kBndGrid);
}
static int pw_bnbwd_impl(const float* g, const float* y, const float* scale, const float* shift, int act,
                         const float* mean, const float* invstd, const float* gamma,
                         const float* x, const float* in_scale, const float* in_shift, int in_act,
                         const float* w, const float* addend, float* dx /* may be NULL: no data gradient */,
                         float* dw, float* dgamma, float* dbeta, float* ws, int64_t M, int K, int Nc, void* stream,
                         const float* ry = nullptr, const float* r_scale = nullptr, const float* r_shift = nullptr, int r_act = 0,
                         const float* r_mean = nullptr, const float* r_invstd = nullptr, float* red_out = nullptr) {
    MNY_REQUIRE(g && y && scale && shift && mean && invstd && gamma && x && w && dw && dgamma && dbeta && ws, "pw_bnbwd: null pointer");
    MNY_REQUIRE(!red_out || (dx && ry && r_scale && r_shift && r_mean && r_invstd && r_act >= MNY_ACT_NONE && r_act < MNY_ACT_HSWISH && bnw_red_ok(M, K, Nc)),
                "pw_bnbwd_red: incomplete reduction target or unsupported shape (mny_pw_bnbwd_red_supported)");
    MNY_REQUIRE(bnw_supported(M, K, Nc), "pw_bnbwd: shape M=%lld K=%d N=%d not supported (need K<=32, N<=192, N>K)", (long long)M, K, Nc);
    MNY_REQUIRE(in_act != MNY_ACT_HSWISH && in_act != MNY_ACT_HSIGMOID && act != MNY_ACT_HSWISH && act != MNY_ACT_HSIGMOID,
                "pw_bnbwd: h-swish / h-sigmoid activations are not supported");
    BnwPlan pl = bnw_plan(M, K, Nc);
    hipStream_t st = (hipStream_t)stream;
    const BnwWs l = bnw_ws(pl, M, K, Nc);
    float *red = ws + l.red, *B1 = ws + l.B1, *Q = ws + l.Q, *bias = ws + l.bias;
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(ws + l.mask);
    BnwArgs a{g, y, scale, shift, act, mean, invstd, x, in_scale, in_shift, in_act, ws, mask, l.npairs, M, K, Nc, pl.rows_per_block, pl.TI};
    dim3 grid(pl.splits, pl.nsl), block(256);
    switch (pl.TIs) {                       // <= 4 column tiles per slice (bnw_plan): <= 54 KB of dynamic LDS
        case 1: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<1>), grid, block, pl.lds1, st, a); break;
        case 2: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<2>), grid, block, pl.lds1, st, a); break;
        case 3: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<3>), grid, block, pl.lds1, st, a); break;
        default: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<4>), grid, block, pl.lds1, st, a); break;
    }
    int rc = check_launch("pw_bnbwd_stage1b_kernel");
    if (rc) return rc;
    rc = pw_bnbwd_finalize_launch(ws, pl.splits, red, w, gamma, mean, invstd, M, Nc, K, dw, dgamma, dbeta, B1, Q, bias, st);
    if (rc || !dx) return rc;
    if (!allow_lds((const void*)pw_bnbwd_dgrad_kernel, 96 * 1024)) {
        set_error("pw_bnbwd: hipFuncSetAttribute failed"); return MNY_EHIP;
    }
    BndArgs d{g, mask, act, x, in_scale, in_shift, in_act, B1, Q, bias, addend, dx, l.npairs, M, Nc, K, pl.TI, pl.m_tiles, pl.tiles_per_block,
              ry, r_scale, r_shift, r_mean, r_invstd, r_act, red_out};
    if (bnw_red_ok(M, K, Nc)) {                                    // second generation: barrier-free direct fragment loads (N % 16 == 0 instantiations)
        const int grid = bnw_red_grid(M);
        if (red_out) {
            if (Nc == 96) hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<6, float, false, true>), dim3(grid), dim3(256), 0, st, d);
            else if (Nc == 144) hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<9, float, false, true>), dim3(grid), dim3(256), 0, st, d);
            else hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<12, float, false, true>), dim3(grid), dim3(256), 0, st, d);
            return check_launch("pw_bnbwd_dgrad2_kernel<red>");
        }
        if (Nc == 96) hipLaunchKernelGGL(pw_bnbwd_dgrad2_kernel<6>, dim3(grid), dim3(256), 0, st, d);
        else if (Nc == 144) hipLaunchKernelGGL(pw_bnbwd_dgrad2_kernel<9>, dim3(grid), dim3(256), 0, st, d);
        else hipLaunchKernelGGL(pw_bnbwd_dgrad2_kernel<12>, dim3(grid), dim3(256), 0, st, d);
        return check_launch("pw_bnbwd_dgrad2_kernel");
    }
    hipLaunchKernelGGL(pw_bnbwd_dgrad_kernel, dim3(pl.gx2), dim3(256), pl.lds2, st, d);
    return check_launch("pw_bnbwd_dgrad_kernel");
}
extern "C" int mny_pw_bnbwd(const float* g, const float* y, const float* scale, const float* shift, int act,
                            const float* mean, const float* invstd, const float* gamma,
                            const float* x, const float* in_scale, const float* in_shift, int in_act,
                            const float* w, const float* addend, float* dx /* may be NULL: no data gradient */,
                            float* dw, float* dgamma, float* dbeta, float* ws, int64_t M, int K, int Nc, void* stream) {
    return pw_bnbwd_impl(g, y, scale, shift, act, mean, invstd, gamma, x, in_scale, in_shift, in_act, w, addend, dx, dw, dgamma, dbeta, ws, M, K, Nc, stream);
}
// ... whose data gradient completes the output gradient of the conv+BN+act unit in front (raw output ry [M][K], view r_scale / r_shift / r_act of the clamp
// family, statistics r_mean / r_invstd): that unit's BN-backward sums leave with it, red[mny_pw_bnbwd_red_parts(M, K, Nc)][2][K] (fp32 storage, N in {96, 144, 192})
extern "C" int mny_pw_bnbwd_red_supported(int64_t M, int K, int Nc) { return bnw_red_ok(M, K, Nc) ? 1 : 0; }
extern "C" int mny_pw_bnbwd_red_parts(int64_t M, int K, int Nc) { return bnw_red_ok(M, K, Nc) ? bnw_red_grid(M) : MNY_EINVAL; }
extern "C" int mny_pw_bnbwd_red(const float* g, const float* y, const float* scale, const float* shift, int act,
                                const float* mean, const float* invstd, const float* gamma,
                                const float* x, const float* in_scale, const float* in_shift, int in_act,
                                const float* w, const float* addend, float* dx, float* dw, float* dgamma, float* dbeta, float* ws,
                                const float* ry, const float* r_scale, const float* r_shift, int r_act, const float* r_mean, const float* r_invstd, float* red,
                                int64_t M, int K, int Nc, void* stream) {
    MNY_REQUIRE(red && dx, "pw_bnbwd_red: null pointer");
    return pw_bnbwd_impl(g, y, scale, shift, act, mean, invstd, gamma, x, in_scale, in_shift, in_act, w, addend, dx, dw, dgamma, dbeta, ws, M, K, Nc, stream,
                         ry, r_scale, r_shift, r_act, r_mean, r_invstd, red);
}

// ---- bf16-storage twin (round 3): G, Y, X, addend, dX are bf16; W, statistics, dW / dgamma / dbeta, the workspace stay fp32 --------------
// Shapes: K in {8, 16, 24, 32}, N in {64, 72, 96, 144, 192} (the expand units of MobileNetV3 / MobileNetV2), M >= 4096.  Same three steps:
// second-generation stage 1 on a bf16 LDS image, the fp32 finalize, the barrier-free data-gradient stage with widened 8-byte loads.
static bool bnw_supported_bf16(int64_t M, int K, int N) {
    // (stage 1 is instantiated for two and three column tiles per slice: 144 / 192 columns run as two slices of three)
    return bnw_supported(M, K, N) && (K & 7) == 0 && (N == 64 || N == 72 || N == 96 || N == 144 || N == 192);
}
extern "C" int mny_pw_bnbwd_supported_bf16(int64_t M, int K, int Nc) { return bnw_supported_bf16(M, K, Nc) ? 1 : 0; }
extern "C" int mny_pw_bnbwd_bf16(const void* g, const void* y, const float* scale, const float* shift, int act,
                                 const float* mean, const float* invstd, const float* gamma,
                                 const void* x, const float* in_scale, const float* in_shift, int in_act,
                                 const float* w, const void* addend, void* dx /* may be NULL: no data gradient */,
                                 float* dw, float* dgamma, float* dbeta, float* ws, int64_t M, int K, int Nc, void* stream) {
    MNY_REQUIRE(g && y && scale && shift && mean && invstd && gamma && x && w && dw && dgamma && dbeta && ws, "pw_bnbwd_bf16: null pointer");
    MNY_REQUIRE(bnw_supported_bf16(M, K, Nc), "pw_bnbwd_bf16: shape M=%lld K=%d N=%d not supported (mny_pw_bnbwd_supported_bf16)", (long long)M, K, Nc);
    MNY_REQUIRE(in_act != MNY_ACT_HSWISH && in_act != MNY_ACT_HSIGMOID && act != MNY_ACT_HSWISH && act != MNY_ACT_HSIGMOID,
                "pw_bnbwd_bf16: h-swish / h-sigmoid activations are not supported");
    hipStream_t st = (hipStream_t)stream;
    if (pwe_ok(M, K, Nc))                                    // wave form on the bf16 matrix cores (gate.hip)
        return pwe_launch(g, y, scale, shift, act, mean, invstd, gamma, x, in_scale, in_shift, in_act, w, addend, dx, dw, dgamma, dbeta, ws, M, K, Nc, st);
    BnwPlan pl = bnw_plan(M, K, Nc);
    const BnwWs l = bnw_ws(pl, M, K, Nc);
    float *red = ws + l.red, *B1 = ws + l.B1, *Q = ws + l.Q, *bias = ws + l.bias;
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(ws + l.mask);
    BnwArgs a{(const float*)g, (const float*)y, scale, shift, act, mean, invstd, (const float*)x, in_scale, in_shift, in_act, ws, mask, l.npairs, M, K, Nc,
              pl.rows_per_block, pl.TI};
    dim3 grid(pl.splits, pl.nsl), block(256);
    // LDS: the bf16 ring is half the fp32 one, but the block reductions at the end use [3][16][64] + vector scratch in fp32
    constexpr int S1 = 3;       // stages of the bf16 ring
    size_t lds1 = (size_t)S1 * 16 * (2 * 32 * pl.TIs + 32) * sizeof(bf16_t);
    const size_t need = (size_t)4 * (2 * pl.TIs + 1) * 32 * sizeof(float);
    if (lds1 < need) lds1 = need;
    if (lds1 < 3 * 16 * 64 * sizeof(float)) lds1 = 3 * 16 * 64 * sizeof(float);
    switch (pl.TIs) {
        case 2: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<2, bf16_t, S1>), grid, block, lds1, st, a); break;
        case 3: hipLaunchKernelGGL((pw_bnbwd_stage1b_kernel<3, bf16_t, S1>), grid, block, lds1, st, a); break;
        default: set_error("pw_bnbwd_bf16: no stage-1 kernel for %d column tiles", pl.TIs); return MNY_EUNSUPPORTED;
    }
    int rc = check_launch("pw_bnbwd_stage1b_kernel<bf16>");
    if (rc) return rc;
    rc = pw_bnbwd_finalize_launch(ws, pl.splits, red, w, gamma, mean, invstd, M, Nc, K, dw, dgamma, dbeta, B1, Q, bias, st);
    if (rc || !dx) return rc;
    BndArgs d{(const float*)g, mask, act, (const float*)x, in_scale, in_shift, in_act, B1, Q, bias, (const float*)addend, (float*)dx, l.npairs, M, Nc, K, pl.TI,
              pl.m_tiles, pl.tiles_per_block};
    const int grid2 = bnw_red_grid(M);
    switch (Nc) {
        case 64: hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<4, bf16_t, false>), dim3(grid2), dim3(256), 0, st, d); break;
        case 72: hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<5, bf16_t, true>), dim3(grid2), dim3(256), 0, st, d); break;
        case 96: hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<6, bf16_t, false>), dim3(grid2), dim3(256), 0, st, d); break;
        case 144: hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<9, bf16_t, false>), dim3(grid2), dim3(256), 0, st, d); break;
        default: hipLaunchKernelGGL((pw_bnbwd_dgrad2_kernel<12, bf16_t, false>), dim3(grid2), dim3(256), 0, st, d); break;
    }
    return check_launch("pw_bnbwd_dgrad2_kernel<bf16>");
}
