// Pointwise (1x1) convolution, forward / data-gradient side:  C[M,N] = act_in(A)[M,K] * B[N,K]^T (+bias)(+addend)      ("NT")
//
// This unit holds the ROUTES of the forward, data-gradient (+ BatchNorm sums), low-rank-fix and pre-cut-planes entry points — which kernel family
// a call takes (PwRoute below) —, their launchers and queries, the RED == 0 half of the LDS-DMA ring NT kernel's table, the plane cut of the
// six-product form and the weight transposes.  The kernels themselves live elsewhere:
//   pwnt_kernel.h  the LDS-DMA ring NT kernel ("NT GEMM v2"), a header: its RED == 0 instantiations are compiled in this unit, the RED != 0 ones
//                  in pwntred.hip, so that the two halves of the table build side by side
//   pwntv1.hip     the register-staged NT kernel of the MNY_ROUTE_TILE_V1 family (any K, any storage type)
//   pwwgrad.hip    the weight gradient: tile kernels, plan, route and entry points (mny_pw_wgrad*)
//   pwbnbwd.hip    the fused BatchNorm-backward of the thin expand units (mny_pw_bnbwd*)
//   gate.hip, pwthin.hip, pwwide.hip, pwwgs.hip   the other families of pwgemm.h
//
// replaces nn.Conv2d(Cin,Cout,1) at models/mobilenetv2.py:48,69,75,83 and models/mbv2_yolo.py:20,82
// and their autograd backward (convolution_backward = 57.5 % of the reference's CPU step).
#include <map>
#include <mutex>

#include "pwgemm.h"
#include "x6.h"
#include "pwnt_kernel.h"

namespace mny {

// the pw_gemm_nt_dma_kernel (pwnt_kernel.h) of a call: the RED == 0 instantiations are compiled here, the RED != 0 ones in pwntred.hip
static Nt2Kernel nt2_kernel(int TN, int XF, int BF = 0, int RED = 0, int X6 = 0, int RB = 0) {      // nullptr: no such kernel
    if (RED) return nt2_red_kernel(TN, XF, BF, RED, X6, RB);
#define MNY_K(T, XF_, BF_, RED_, X6_, RB_) case nt2_key(T, XF_, BF_, RED_, X6_, RB_): return (Nt2Kernel)pw_gemm_nt_dma_kernel<T, XF_, BF_, RED_, X6_, RB_>;
#define MNY_FWD(T, BF_, X6_) MNY_K(T, 0, BF_, 0, X6_, 0) MNY_K(T, 1, BF_, 0, X6_, 0) MNY_K(T, 2, BF_, 0, X6_, 0)      // no view, linear / clamp view, h-swish view
#define MNY_TN5(M_, ...) M_(1, __VA_ARGS__) M_(2, __VA_ARGS__) M_(3, __VA_ARGS__) M_(4, __VA_ARGS__) M_(5, __VA_ARGS__)
    switch (nt2_key(TN, XF, BF, RED, X6, RB)) {
        // forward / plain data gradient, column tiles of 32 .. 160: fp32 MFMA, six-product (X6 = 1), pre-cut weight planes (X6 = 3), bf16 storage
        MNY_TN5(MNY_FWD, 0, 0) MNY_TN5(MNY_FWD, 0, 1) MNY_TN5(MNY_FWD, 0, 3) MNY_TN5(MNY_FWD, 1, 0)
    }
#undef MNY_TN5
#undef MNY_FWD
#undef MNY_K
    return nullptr;
}

struct Nt2Plan { int TN, n_tiles, m_tiles, gx, tiles_per_block, grid; size_t lds; };

static size_t nt2_lds(int TN, int K, bool xf, int BF = 0) {
    const int Kpad = (int)cdiv(K, BF ? 32 : 16) * (BF ? 32 : 16);
    size_t ring = (size_t)3 * (BM * 16 + 32 * TN * 16) * sizeof(float);
    size_t red = (size_t)4 * 32 * TN * 2 * sizeof(float);
    return (ring > red ? ring : red) + (xf ? 2 * Kpad * sizeof(float) : 0);
}

// kernels whose dynamic LDS exceeds the 64 KB default need the opt-in once (the pre-cut planes mode at TN >= 4 with a deep scale cache)
static void nt2_allow_lds(Nt2Kernel k, size_t lds) {
    if (lds <= 64 * 1024) return;
    (void)allow_lds((const void*)k, lds);
}

// ---- pre-cut weight planes for the six-product form --------------------------------------------------------------------------
// src [R][C] fp32 (a conv weight [Cout][Cin] or its transpose) -> dst: three bf16 planes [R][nk][2][8], nk = ceil(C / 16); chunk
// (row, kt, h) holds k = 16 kt + {4h, 4h+1, 4h+2, 4h+3, 8+4h, ..., 8+4h+3} — the eight values lane-half h of the NT kernel multiplies
// in stage kt — cut by truncation exactly like x6_split (hi + mid + lo == the fp32 value), zeros past C.  One thread per chunk.
struct Cut3Job { const float* src; void* dst; int32_t R, C, block0, pad; };
__global__ __launch_bounds__(256) void cut3_batch_kernel(const Cut3Job* __restrict__ jobs, const int32_t* __restrict__ block_job) {
    const Cut3Job jb = jobs[block_job[blockIdx.x]];
    const int nk = (jb.C + 15) / 16;
    const int64_t idx = (int64_t)(blockIdx.x - jb.block0) * 256 + threadIdx.x;       // chunk index: (row * nk + kt) * 2 + h
    if (idx >= (int64_t)jb.R * nk * 2) return;
    const int h = (int)(idx & 1);
    const int64_t rk = idx >> 1;
    const int kt = (int)(rk % nk);
    const int64_t row = rk / nk;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = kt * 16 + (e < 4 ? 4 * h + e : 8 + 4 * h + (e - 4));
        x[e] = k < jb.C ? jb.src[row * jb.C + k] : 0.f;
    }
    bf16x8_t hh, mm, ll;
    x6_split(v4f_t{x[0], x[1], x[2], x[3]}, v4f_t{x[4], x[5], x[6], x[7]}, hh, mm, ll);
    const int64_t plane = (int64_t)jb.R * nk * 32;                                     // bytes
    char* d = reinterpret_cast<char*>(jb.dst) + idx * 16;
    *reinterpret_cast<v4f_t*>(d) = __builtin_bit_cast(v4f_t, hh);
    *reinterpret_cast<v4f_t*>(d + plane) = __builtin_bit_cast(v4f_t, mm);
    *reinterpret_cast<v4f_t*>(d + 2 * plane) = __builtin_bit_cast(v4f_t, ll);
}

// resident workgroups per CU for (TN, XF) at a given dynamic-LDS size (queried once per distinct size)
static int nt2_blocks_per_cu(int TN, int XF, size_t lds, int BF = 0) {
    static std::map<uint64_t, int> cache;
    static std::mutex mu;
    const uint64_t key = ((uint64_t)BF << 48) | ((uint64_t)TN << 40) | ((uint64_t)XF << 32) | (uint64_t)lds;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)nt2_kernel(TN, XF, BF), 256, lds) != hipSuccess || nb < 1) nb = 1;
    if (nb > 8) nb = 8;
    cache[key] = nb;
    return nb;
}

static Nt2Plan nt2_plan(int64_t M, int K, int N, bool xf, int BF = 0, int tn_cap = 5) {
    Nt2Plan pl;
    int best = 1, best_pad = 1 << 30;
    for (int tn = tn_cap; tn >= 1; --tn) {           // minimise the padded width; ties -> the wider tile (A read fewer times,
        int pad = (int)cdiv(N, 32 * tn) * 32 * tn;   // longer contiguous output rows)
        if (pad < best_pad) { best_pad = pad; best = tn; }
    }
    // grid depends only on (M,K,N): occupancy is taken for the transform variant so stat_parts() and fwd agree
    const int blocks_per_cu = nt2_blocks_per_cu(best, 1, nt2_lds(best, K, true, BF), BF);
    pl.TN = best;
    pl.n_tiles = (int)cdiv(N, 32 * best);
    pl.m_tiles = (int)cdiv(M, BM);
    int want = 256 * blocks_per_cu / pl.n_tiles;      // one full wave of resident workgroups
    if (want < 8) want = 8;
    if (want > kMaxParts) want = kMaxParts;
    int gx = pl.m_tiles < want ? pl.m_tiles : want;
    pl.tiles_per_block = (int)cdiv(pl.m_tiles, gx);
    // Balance the CUs, not the slots: all blocks are resident at once and share their CU's matrix pipes, so a launch takes
    // (blocks on the busiest CU) x (tiles per block).  Filling every slot (3/CU) with 5.04 tiles' worth of work each means 6
    // rounds on CUs holding 3 blocks = 18 tile-times, where 2 blocks/CU x 8 tiles = 16.  Search tiles-per-block upwards from
    // the one-wave minimum; ties -> more blocks (more waves to hide latency).
    constexpr double min_ai = 100.0;
    // ... for the matrix-pipe-bound shapes only (FLOP per byte of A + C rows): an HBM-bound layer wants every slot filled
    // (memory-level parallelism), measured 5 % slower with fewer, longer blocks
    const double ai = 2.0 * K * N / ((BF ? 2.0 : 4.0) * (K + N));
    if (ai >= min_ai) {
        const int t_min = pl.tiles_per_block;
        long best_cost = -1;
        int best_t = t_min, best_b = 0;
        for (int t = t_min; t <= 4 * t_min + 4 && t <= pl.m_tiles; ++t) {
            const int g = (int)cdiv(pl.m_tiles, t);
            const int nb = g * pl.n_tiles;                                     // real blocks (the grid's padding blocks exit at once)
            if (nb < 256) break;                                               // never leave CUs without a block
            const long cost = (long)cdiv(nb, 256) * t;
            if (best_cost < 0 || cost < best_cost || (cost == best_cost && nb > best_b)) { best_cost = cost; best_t = t; best_b = nb; }
        }
        pl.tiles_per_block = best_t;
    }
    pl.gx = (int)cdiv(pl.m_tiles, pl.tiles_per_block);
    pl.grid = (int)cdiv(pl.gx, 8) * 8 * pl.n_tiles;
    pl.lds = nt2_lds(best, K, xf, BF);
    return pl;
}

// dst[c][r] = src[r][c], destination row pitch Rp >= R, pad columns zeroed
template <typename T>
__global__ void transpose_kernel(const float* __restrict__ src, T* __restrict__ dst, int R, int Cc, int Rp) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = by + j, c = bx + threadIdx.x;
        tile[j][threadIdx.x] = (r < R && c < Cc) ? src[(int64_t)r * Cc + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int c = bx + j, r = by + threadIdx.x;
        if (r < Rp && c < Cc) st1(dst + (int64_t)c * Rp + r, r < R ? tile[threadIdx.x][j] : 0.f);
    }
}

}  // namespace mny

using namespace mny;
static thread_local int g_pw_route = -1;        // kernel family of this thread's last pointwise-conv call (mny_pw_last_route below)
void mny::pw_set_last_route(int family) { g_pw_route = family; }      // for the weight-gradient launcher (pwwgrad.hip)

// ---- which kernel a pointwise-conv call takes ------------------------------------------------------------------------------------------
// One route function per operation: the complete description of a call in, the decision out.  The launchers act on it, and every *_parts /
// *_splits / *_supported / *_ws_floats query, mny_pw_w6_supported and mny_pw_route ask the same function about the PLAIN call (no view, no
// bias, no addend) — so a query cannot count other rows than the launcher's kernel writes.  The kernel families' own predicates (pw_thin_ok,
// pw_wide_ok, pwt_ok, pw_wide_fix_ok), the MNY_GEMM_V1 switch and the channel-alignment tests appear in the route functions only: the three
// below and, for the weight gradient (pw_wgs_ok, MNY_WGRAD_V1), pw_wgrad_route of pwwgrad.hip with a route struct of its own.
struct PwRoute {
    int family = MNY_ROUTE_TILE_V1;     // MNY_ROUTE_*
    const char* why = nullptr;          // NULL: supported; else what keeps the call off this entry point
    int parts = MNY_EINVAL;             // partial rows the call writes
    bool as_counted = true;             // the plain call takes the same family — and rows are a function of family and shape: what the query counted holds
    int64_t Mf = 0;                     // wide family: the rows on whole 32-row tiles, wide_parts partial rows; the last M - Mf rows (one more partial
    int wide_parts = 0;                 //   row) follow on the LDS-DMA kernel by `p2`
    int x6 = 0;                         // LDS-DMA families, the X6 of the kernel: 0 = fp32 / bf16 MFMA, 1 = six-product form, 3 = on pre-cut weight planes
    Nt2Plan p2{};                       // LDS-DMA families (and the wide family's last rows)
    size_t lds = 0;                     //   their dynamic LDS
};

// Pre-cut weight planes pay where the matrix pipe is the bound.  Round 2: a stage of B grew from 64 to 96 bytes per row, which cost the mid-size
// shapes their third resident workgroup (7-18 % faster from ~60 FLOP per byte up, 10-30 % slower below ~40).  Round 3: the plane ring is two
// slots deep (the A ring stays at three), the LDS footprint equals the plain mode's and the threshold moved down to 30 FLOP per byte
// (same-box A/B per shape: K576 N96 -11 %, K384 N96 -10 %, the 75-channel heads -9..-11 %, K384 N64 (27 FLOP per byte) +0..+7 % -> 30, was 50)
static bool w6_pays(int K, int Nc) {
    constexpr double min_ai = 30.0;
    return !sw(SW_NO_W6) && 2.0 * K * Nc / (4.0 * (K + Nc)) >= min_ai;
}

// forward / plain data gradient (mny_pw_fwd, _bf16, _w6).  view: the input is read through in_scale / in_shift; planes: the weight is pre-cut (fp32)
static PwRoute pw_fwd_route(int bf, int64_t M, int K, int Nc, int in_act, bool view, bool bias, bool addend, bool planes) {
    PwRoute r;
    if (M <= 0 || K <= 0 || Nc <= 0) { r.why = "empty problem"; return r; }
    const bool v1 = sw(SW_GEMM_V1);   // A/B switch for profiling
    const bool thin = pw_thin_ok(bf, 0, M, K, Nc);                    // short reduction: vector-ALU stream kernel (pwthin.hip)
    const bool wide = !bf && !thin && pw_wide_ok(M, K, Nc, false);    // short reduction, wide output: barrier-free matrix-core kernel (pwwide.hip)
    auto family = [&](int act, bool has_bias, bool has_addend) {
        if (bf && pwt_ok(M, K, Nc, act, has_bias)) return MNY_ROUTE_WAVE16;      // K <= 48 at a large pixel count: a wave per 16 pixels on the bf16 matrix cores (gate.hip)
        if (thin) return MNY_ROUTE_THIN;
        if (wide && !has_bias && !has_addend && act != MNY_ACT_HSIGMOID) return MNY_ROUTE_WIDE;      // (that kernel knows no bias, addend or h-sigmoid view)
        if ((K & (bf ? 7 : 3)) || v1) return MNY_ROUTE_TILE_V1;                  // the LDS-DMA pipeline reads 16-B aligned input rows
        return !bf && nt_x6(M, K, Nc) ? MNY_ROUTE_DMA_X6 : MNY_ROUTE_DMA_F32;
    };
    r.family = family(in_act, bias, addend);
    const int plain = in_act == MNY_ACT_NONE && !bias && !addend ? r.family : family(MNY_ACT_NONE, false, false);
    r.as_counted = r.family == plain;
    // pre-cut planes: one set serves a weight's forward and (transposed) its data gradient with sums — one rule for both
    if (planes && (bf || plain != MNY_ROUTE_DMA_X6 || pw_wide_ok(M, K, Nc, true) || !w6_pays(K, Nc))) r.why = "no pre-cut weight planes for this problem (mny_pw_w6_supported)";
    const bool xf = view || in_act != MNY_ACT_NONE;
    switch (r.family) {
        case MNY_ROUTE_WAVE16: r.parts = pwt_parts(M); return r;
        case MNY_ROUTE_THIN: r.parts = pw_thin_parts(M, K, Nc, 0); return r;
        case MNY_ROUTE_TILE_V1: r.parts = pw_v1_parts(M, K, Nc); return r;
        case MNY_ROUTE_WIDE:
            r.Mf = M & ~(int64_t)31;
            r.parts = r.wide_parts = pw_wide_parts(M, K, Nc, false);
            if (r.Mf == M) return r;
            r.p2 = nt2_plan(M - r.Mf, K, Nc, xf);
            r.x6 = nt_x6(M, K, Nc);
            r.parts += r.p2.gx;
            break;
        default:
            r.p2 = nt2_plan(M, K, Nc, xf, bf);
            r.x6 = r.family == MNY_ROUTE_DMA_X6;
            r.parts = r.p2.gx;
    }
    r.lds = r.p2.lds;
    size_t lds_max = 64 * 1024;
    if (planes) {
        r.x6 = 3;
#if MNY_W6_SWP
        // software-pipelined form: three-slot A ring + THREE-slot plane ring (24 + 9 TN KB) + the scale / shift cache; else three-slot A ring +
        // two-slot plane ring = the plain mode's three-slot (A + fp32 B) ring, to the byte
        r.lds = (size_t)(3 * BM * 16 + 3 * 32 * r.p2.TN * 24) * sizeof(float) + (xf ? 2 * cdiv(K, 16) * 16 * sizeof(float) : 0);
#endif
        lds_max = 96 * 1024;
    }
    if (!r.why && r.lds > lds_max) r.why = "K too large for the LDS scale cache";
    return r;
}

// data gradient + the BatchNorm-backward sums of the unit it feeds (mny_pw_dgrad_bnred, _add, _bf16, _w6).  The reduction epilogue holds four more
// per-column constants and a group of loads: the 160-column tile (TN = 5) spills with it
constexpr int kRedMaxTn = 4;
static PwRoute pw_dgrad_bnred_route(int bf, int64_t M, int K, int Nc, int act, bool addend, bool planes) {
    PwRoute r;
    if (M <= 0 || K <= 0 || Nc <= 0 || (K & (bf ? 7 : 3))) { r.why = "empty problem, or dy rows that are not 16-byte aligned"; return r; }
    const bool v1 = sw(SW_GEMM_V1), thin32 = pw_thin_ok(0, 1, M, K, Nc), wide = pw_wide_ok(M, K, Nc, true);
    r.x6 = !bf && nt_x6(M, K, Nc);                            // (the six-product bf16 form exists for fp32 operands only)
    bool tile = false;
    if (bf && pwt_ok(M, K, Nc, MNY_ACT_NONE, false)) {        // K <= 48 at a large pixel count: a wave per 16 pixels (gate.hip)
        r.family = MNY_ROUTE_WAVE16;
        r.parts = pwt_parts(M);
    } else if (bf ? pw_thin_ok(1, 1, M, K, Nc) : thin32) {
        r.family = MNY_ROUTE_THIN;
        r.parts = pw_thin_parts(M, K, Nc, 1);
    } else if (!bf && wide) {       // whole 32-row tiles on the barrier-free kernel, the last M % 32 rows on the LDS-DMA kernel (one more partial row)
        r.family = MNY_ROUTE_WIDE;
        r.Mf = M & ~(int64_t)31;
        r.parts = r.wide_parts = pw_wide_parts(M, K, Nc, true);
        if (r.Mf != M) {
            r.p2 = nt2_plan(M - r.Mf, K, Nc, false, 0, kRedMaxTn);
            r.parts += r.p2.gx;
        }
    } else {
        // (MNY_GEMM_V1: the first generation takes no sums — unsupported below; the plain data gradient that runs instead takes those kernels)
        r.family = v1 ? MNY_ROUTE_TILE_V1 : r.x6 ? MNY_ROUTE_DMA_X6 : MNY_ROUTE_DMA_F32;
        r.p2 = nt2_plan(M, K, Nc, false, bf, kRedMaxTn);
        r.parts = r.p2.gx;
        tile = true;
    }
    r.lds = r.p2.lds;
    if (act < MNY_ACT_NONE || act > MNY_ACT_HSIGMOID) r.why = "unknown activation";
    else if (v1) r.why = "MNY_GEMM_V1 is set";
    else if (K >= 512 && Nc >= 512) r.why = "matrix-pipe-bound: the reduce pass it would save is cheaper than the longer epilogue";
    // (the next two are the fp32 kernels' limits, answered for either storage type: bf16 plans keep the separate reduce pass on the same units)
    else if (thin32 && act == MNY_ACT_HSIGMOID) r.why = "the short-reduction kernel knows the clamp family and h-swish (what units use)";
    else if (wide && act >= MNY_ACT_HSWISH) r.why = "the wide-output kernel's reduction form knows the clamp family (its h-swish builds spill)";
    // the addend variant exists for column tiles of <= 96 (TN <= 3: the 128-column tile has no registers left for the addend loads)
    else if (addend && tile && r.p2.TN > 3) r.why = "the addend form needs a column tile of <= 96 (mny_pw_dgrad_bnred_add_supported)";
    else if (planes && (bf || r.family != MNY_ROUTE_DMA_X6 || pw_wide_ok(M, K, Nc, false) || !w6_pays(K, Nc))) r.why = "no pre-cut weight planes for this problem (mny_pw_w6_supported)";
    else if (r.lds > (size_t)(planes ? 96 : 64) * 1024) r.why = "K too large";
    if (planes) r.x6 = 3;
    return r;
}

// low-rank fix (mny_pw_lr_fix): red = a call WITH a reduction target, the only one that writes partial rows
static PwRoute pw_lr_fix_route(int64_t M, int K, int r_act, bool red, bool view) {
    PwRoute r;
    if (M <= 0 || K <= 0 || (K & 3)) { r.why = "empty problem, or rows that are not 16-byte aligned"; return r; }
    if (red && pw_wide_fix_ok(M, K) && r_act < MNY_ACT_HSWISH) {            // K = 64 / 96 at whole 32-row tiles: the barrier-free kernel of pwwide.hip
        r.family = MNY_ROUTE_WIDE;
        r.parts = pw_wide_fix_parts(M, K);
        return r;
    }
    r.p2 = nt2_plan(M, K, K, view, 0, 3);                                   // always column tiles of <= 96 (the addend form's limit)
    r.lds = r.p2.lds;
    r.x6 = nt_x6(M, K, K);
    r.family = r.x6 ? MNY_ROUTE_DMA_X6 : MNY_ROUTE_DMA_F32;
    r.parts = r.p2.gx;
    if (r.lds > 64 * 1024) r.why = "K too large";
    return r;
}

extern "C" int mny_pw_stat_parts(int64_t M, int K, int Nc) { return pw_fwd_route(0, M, K, Nc, MNY_ACT_NONE, false, false, false, false).parts; }
extern "C" int mny_pw_stat_parts_bf16(int64_t M, int K, int Nc) { return pw_fwd_route(1, M, K, Nc, MNY_ACT_NONE, false, false, false, false).parts; }

// an LDS-DMA launch as its route planned it
static int nt2_launch(const PwRoute& r, int XF, int BF, int RED, int RB, const Gemm2Args& g, hipStream_t st, const char* what) {
    const Nt2Kernel k = nt2_kernel(r.p2.TN, XF, BF, RED, r.x6, RB);
    if (!k) {
        set_error("%s: no kernel for a %d-column tile", what, 32 * r.p2.TN); return MNY_EUNSUPPORTED;
    }
    nt2_allow_lds(k, r.lds);
    hipLaunchKernelGGL(k, dim3(r.p2.grid), dim3(256), r.lds, st, g);
    return check_launch(what);
}

template <int BF>
static int pw_fwd_impl(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* w, const float* bias, const void* addend,
                       void* y, float* stats, int64_t M, int K, int Nc, void* stream, bool planes = false) {
    MNY_REQUIRE(x && w && y, "pw_fwd: null pointer");
    MNY_REQUIRE(!(stats && bias), "pw_fwd: stats and bias are mutually exclusive");
    const PwRoute r = pw_fwd_route(BF, M, K, Nc, in_act, in_scale != nullptr, bias != nullptr, addend != nullptr, planes);
    MNY_REQUIRE(!r.why, "pw_fwd: M=%lld K=%d N=%d: %s", (long long)M, K, Nc, r.why);
    // mny_pw_stat_parts[_bf16] sizes the caller's partial rows from (M, K, Nc) alone: a view / bias / addend that moves the call to another kernel
    // family than the query assumed would write a different number of rows than mny_bn_finalize sums — refuse it instead
    MNY_REQUIRE(!stats || r.as_counted, "pw_fwd: statistics with in_act=%d%s%s at M=%lld K=%d N=%d take another kernel family than mny_pw_stat_parts%s counted rows for",
                in_act, bias ? ", a bias" : "", addend ? ", an addend" : "", (long long)M, K, Nc, BF ? "_bf16" : "");
    g_pw_route = r.family;
    hipStream_t st = (hipStream_t)stream;
    switch (r.family) {
        case MNY_ROUTE_WAVE16: return pwt_launch(x, in_scale, in_shift, in_act, w, addend, y, stats, M, K, Nc, st);
        case MNY_ROUTE_THIN:
            return pw_thin_launch(BF, x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, st);
        case MNY_ROUTE_TILE_V1: return pw_v1_launch(BF, x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, st);
        case MNY_ROUTE_WIDE: {      // fp32: whole 32-row tiles; the last M % 32 rows follow below
            const int rc = pw_wide_launch((const float*)x, in_scale, in_shift, in_act, (const float*)w, (float*)y, stats, r.Mf, K, Nc, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, 0, nullptr, st);
            if (rc != 0 || r.Mf == M) return rc;
            if (stats) stats += (int64_t)r.wide_parts * 2 * Nc;
            x = (const float*)x + r.Mf * K; y = (float*)y + r.Mf * Nc; M -= r.Mf;
        }
    }
    Gemm2Args g{x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, r.p2.m_tiles, r.p2.tiles_per_block, r.p2.gx, r.p2.n_tiles,
                nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const int XF = !in_scale && in_act == MNY_ACT_NONE ? 0 : (in_act == MNY_ACT_HSWISH ? 2 : 1);
    return nt2_launch(r, XF, BF, 0, 0, g, st, "pw_gemm_nt_dma_kernel");
}
extern "C" int mny_pw_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w,
                          const float* bias, const float* addend, float* y, float* stats, int64_t M, int K, int Nc,
                          void* stream) {
    return pw_fwd_impl<0>(x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, stream);
}
extern "C" int mny_pw_fwd_bf16(const void* x, const float* in_scale, const float* in_shift, int in_act, const void* w,
                               const float* bias, const void* addend, void* y, float* stats, int64_t M, int K, int Nc,
                               void* stream) {
    return pw_fwd_impl<1>(x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, stream);
}

// data-gradient GEMM of a pointwise conv whose INPUT is the output of a conv+BN+act unit: dx = dy * W (W^T given, [K][Nc] rows = [Nc][K]
// transposed -> NT), and in the same epilogue that unit's BN-backward reduction over (dx, its raw output y): the separate
// mny_bn_bwd_reduce pass (one more read of dx and of y) disappears — only y is read, by the tile that just produced dx.
template <int BF>
static int pw_dgrad_bnred_impl(const void* dy, const void* wT, void* dx, const void* y, const float* scale, const float* shift, int act,
                               const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream, const void* addend = nullptr,
                               bool planes = false) {
    MNY_REQUIRE(dy && wT && dx && y && scale && shift && mean && invstd && red, "pw_dgrad_bnred: null pointer");
    const PwRoute r = pw_dgrad_bnred_route(BF, M, K, Nc, act, addend != nullptr, planes);
    MNY_REQUIRE(!r.why, "pw_dgrad_bnred: unsupported problem M=%lld K=%d N=%d act=%d: %s (see mny_pw_dgrad_bnred_supported)", (long long)M, K, Nc, act, r.why);
    g_pw_route = r.family;
    hipStream_t st = (hipStream_t)stream;
    switch (r.family) {
        case MNY_ROUTE_WAVE16: return pwt_launch(dy, nullptr, nullptr, MNY_ACT_NONE, wT, addend, dx, red, M, K, Nc, st, y, scale, shift, mean, invstd, act);
        case MNY_ROUTE_THIN:
            return pw_thin_launch(BF, dy, nullptr, nullptr, MNY_ACT_NONE, wT, nullptr, addend, dx, red, M, K, Nc, addend ? 2 : 1, y, scale, shift, mean, invstd, act, st);
        case MNY_ROUTE_WIDE: {      // fp32: whole 32-row tiles; the last M % 32 rows follow below
            const int rc = pw_wide_launch((const float*)dy, nullptr, nullptr, MNY_ACT_NONE, (const float*)wT, (float*)dx, red, r.Mf, K, Nc, (const float*)y, scale, shift,
                                          mean, invstd, act, (const float*)addend, st);
            if (rc != 0 || r.Mf == M) return rc;
            red += (int64_t)r.wide_parts * 2 * Nc;
            dy = (const float*)dy + r.Mf * K; dx = (float*)dx + r.Mf * Nc; y = (const float*)y + r.Mf * Nc;
            if (addend) addend = (const float*)addend + r.Mf * Nc;
            M -= r.Mf;
        }
    }
    Gemm2Args g{dy, nullptr, nullptr, MNY_ACT_NONE, wT, nullptr, addend, dx, red, M, K, Nc, r.p2.m_tiles, r.p2.tiles_per_block, r.p2.gx, r.p2.n_tiles,
                y, scale, shift, mean, invstd, act};
    return nt2_launch(r, 0, BF, addend ? 2 : 1, 0, g, st, "pw_gemm_nt_dma_kernel<RED>");
}
extern "C" int mny_pw_dgrad_bnred_supported(int64_t M, int K, int Nc, int act) { return !pw_dgrad_bnred_route(0, M, K, Nc, act, false, false).why; }
extern "C" int mny_pw_dgrad_bnred_parts(int64_t M, int K, int Nc) { return pw_dgrad_bnred_route(0, M, K, Nc, MNY_ACT_NONE, false, false).parts; }
extern "C" int mny_pw_dgrad_bnred(const float* dy, const float* wT, float* dx, const float* y, const float* scale, const float* shift, int act,
                                  const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream) {
    return pw_dgrad_bnred_impl<0>(dy, wT, dx, y, scale, shift, act, mean, invstd, red, M, K, Nc, stream);
}
extern "C" int mny_pw_dgrad_bnred_add_supported(int64_t M, int K, int Nc, int act) { return !pw_dgrad_bnred_route(0, M, K, Nc, act, true, false).why; }
extern "C" int mny_pw_dgrad_bnred_add_supported_bf16(int64_t M, int K, int Nc, int act) { return !pw_dgrad_bnred_route(1, M, K, Nc, act, true, false).why; }
extern "C" int mny_pw_dgrad_bnred_add(const float* dy, const float* wT, const float* addend, float* dx, const float* y, const float* scale, const float* shift,
                                      int act, const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream) {
    MNY_REQUIRE(addend, "pw_dgrad_bnred_add: null addend");
    return pw_dgrad_bnred_impl<0>(dy, wT, dx, y, scale, shift, act, mean, invstd, red, M, K, Nc, stream, addend);
}
extern "C" int mny_pw_dgrad_bnred_add_bf16(const void* dy, const void* wT, const void* addend, void* dx, const void* y, const float* scale, const float* shift,
                                           int act, const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream) {
    MNY_REQUIRE(addend, "pw_dgrad_bnred_add: null addend");
    return pw_dgrad_bnred_impl<1>(dy, wT, dx, y, scale, shift, act, mean, invstd, red, M, K, Nc, stream, addend);
}
// bf16 storage: dy, wT, dx, y are bf16; the sums are taken over the ROUNDED dx (what a separate reduce pass would read back)
extern "C" int mny_pw_dgrad_bnred_supported_bf16(int64_t M, int K, int Nc, int act) { return !pw_dgrad_bnred_route(1, M, K, Nc, act, false, false).why; }
extern "C" int mny_pw_dgrad_bnred_parts_bf16(int64_t M, int K, int Nc) { return pw_dgrad_bnred_route(1, M, K, Nc, MNY_ACT_NONE, false, false).parts; }
extern "C" int mny_pw_dgrad_bnred_bf16(const void* dy, const void* wT, void* dx, const void* y, const float* scale, const float* shift, int act,
                                       const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc, void* stream) {
    return pw_dgrad_bnred_impl<1>(dy, wT, dx, y, scale, shift, act, mean, invstd, red, M, K, Nc, stream);
}

// ---- low-rank BatchNorm-backward correction of a wide expand unit's data gradient (csrc/lrbwd.hip) ----------------------------------
// dx = view(x) Q + r + addend  (x the K-wide input of the unit behind its LINEAR view in_scale / in_shift — applied where the A fragment is read,
// as in every forward GEMM —, Q [K][K] symmetric and r [K] from mny_lr_prep, addend = the main term dzc W, usually dx itself); with `red` the
// BN-backward sums of the unit whose complete output gradient dx now is (its raw output ry, as mny_pw_dgrad_bnred_add).
extern "C" int mny_pw_lr_fix_parts(int64_t M, int K, int r_act) { return pw_lr_fix_route(M, K, r_act, true, false).parts; }
extern "C" int mny_pw_lr_fix(const float* x, const float* in_scale, const float* in_shift, const float* q, const float* r, const float* addend, float* dx,
                             const float* ry, const float* r_scale, const float* r_shift, int r_act, const float* r_mean, const float* r_invstd, float* red,
                             int64_t M, int K, void* stream) {
    MNY_REQUIRE(x && q && r && addend && dx && (!in_scale) == (!in_shift), "pw_lr_fix: bad arguments (K=%d)", K);
    MNY_REQUIRE(!red || (ry && r_scale && r_shift && r_mean && r_invstd && r_act >= MNY_ACT_NONE && r_act <= MNY_ACT_HSIGMOID), "pw_lr_fix: incomplete reduction target");
    const bool xf = in_scale != nullptr;
    const PwRoute rt = pw_lr_fix_route(M, K, r_act, red != nullptr, xf);
    MNY_REQUIRE(!rt.why, "pw_lr_fix: bad arguments (M=%lld K=%d): %s", (long long)M, K, rt.why);
    g_pw_route = rt.family;
    if (rt.family == MNY_ROUTE_WIDE)
        return pw_wide_fix_launch(x, in_scale, in_shift, q, r, addend, dx, red, M, K, ry, r_scale, r_shift, r_mean, r_invstd, r_act, (hipStream_t)stream);
    Gemm2Args g{x, in_scale, in_shift, MNY_ACT_NONE, q, r, addend, dx, red, M, K, K, rt.p2.m_tiles, rt.p2.tiles_per_block, rt.p2.gx, rt.p2.n_tiles,
                ry, r_scale, r_shift, r_mean, r_invstd, r_act};
    return nt2_launch(rt, xf ? 1 : 0, 0, red ? 2 : 0, red ? 1 : 0, g, (hipStream_t)stream, "pw_gemm_nt_dma_kernel<lr_fix>");
}

// ---- forward / data-gradient GEMMs on pre-cut weight planes (fp32 plans, six-product form; w6_pays above) -------------------------------
extern "C" int mny_pw_w6_supported(int64_t M, int K, int Nc) { return !pw_fwd_route(0, M, K, Nc, MNY_ACT_NONE, false, false, false, true).why; }
extern "C" size_t mny_pw_w6_bytes(int K, int Nc) { return (K <= 0 || Nc <= 0) ? 0 : (size_t)3 * Nc * ((K + 15) / 16) * 32; }
extern "C" int mny_cut3_batch(const mny_cut3_job* jobs, const int32_t* block_job, int nblocks, void* stream) {
    MNY_REQUIRE(jobs && block_job && nblocks > 0, "cut3_batch: bad arguments");
    static_assert(sizeof(mny_cut3_job) == sizeof(Cut3Job), "job layout");
    hipLaunchKernelGGL(cut3_batch_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const Cut3Job*>(jobs), block_job);
    return check_launch("cut3_batch_kernel");
}
extern "C" int mny_pw_fwd_w6(const float* x, const float* in_scale, const float* in_shift, int in_act, const void* w6, const float* bias,
                             const float* addend, float* y, float* stats, int64_t M, int K, int Nc, void* stream) {      // same tiling and partial rows as mny_pw_fwd
    return pw_fwd_impl<0>(x, in_scale, in_shift, in_act, w6, bias, addend, y, stats, M, K, Nc, stream, true);
}
// data gradient + BN-backward sums of the fed unit (mny_pw_dgrad_bnred / _add semantics; addend may be NULL) on pre-cut W^T planes
extern "C" int mny_pw_dgrad_bnred_w6(const float* dy, const void* wT6, const float* addend, float* dx, const float* y, const float* scale,
                                     const float* shift, int act, const float* mean, const float* invstd, float* red, int64_t M, int K, int Nc,
                                     void* stream) {
    return pw_dgrad_bnred_impl<0>(dy, wT6, dx, y, scale, shift, act, mean, invstd, red, M, K, Nc, stream, addend, true);
}

// which kernel family the LAST pointwise-conv call of this thread took — every launcher assigns it once, from its route.  engine.py records it
// for every call of a plan's first replay; NetPlan.kernel_routes() reports those.
extern "C" int mny_pw_last_route(void) { return g_pw_route; }

// The kernel family of a call with a plain view (no input view, bias, addend or bias gradient): the launchers' own route functions evaluated for
// that call, so for a plain call it is what mny_pw_last_route reports afterwards.  A call behind an h-swish view or with a bias (gradient) can
// take another family.  For shapes no plan at hand launches (tests ask it about the bs-256 shapes while running a bs-64 plan).
extern "C" int mny_pw_route(int op, int bf16, int64_t M, int K, int Nc) {
    if (M <= 0 || K <= 0 || Nc <= 0 || op < 0 || op > 2) return MNY_EINVAL;
    const int bf = bf16 ? 1 : 0;
    if (op == 0) return pw_fwd_route(bf, M, K, Nc, MNY_ACT_NONE, false, false, false, false).family;
    if (op == 1) return pw_dgrad_bnred_route(bf, M, K, Nc, MNY_ACT_NONE, false, false).family;
    return pw_wgrad_family(bf, M, K, Nc);
}

// every W^T of a backward pass in ONE launch: block b serves 32x32 tile (b - job.block0) of job block_job[b]
template <typename T>
__global__ void transpose_batch_kernel(const mny_transpose_job* __restrict__ jobs, const int32_t* __restrict__ block_job) {
    __shared__ float tile[32][33];
    const mny_transpose_job jb = jobs[block_job[blockIdx.x]];
    const int local = (int)blockIdx.x - jb.block0, tx = (jb.Cc + 31) / 32;
    const int bx = (local % tx) * 32, by = (local / tx) * 32;
    const float* src = jb.src;
    T* dst = (T*)jb.dst;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = by + j, c = bx + threadIdx.x;
        tile[j][threadIdx.x] = (r < jb.R && c < jb.Cc) ? src[(int64_t)r * jb.Cc + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int c = bx + j, r = by + threadIdx.x;
        if (r < jb.Rp && c < jb.Cc) st1(dst + (int64_t)c * jb.Rp + r, r < jb.R ? tile[threadIdx.x][j] : 0.f);
    }
}
extern "C" int mny_transpose_batch(const mny_transpose_job* jobs, const int32_t* block_job, int nblocks, void* stream) {
    MNY_REQUIRE(jobs && block_job && nblocks > 0, "transpose_batch: bad arguments");
    hipLaunchKernelGGL((transpose_batch_kernel<float>), dim3((unsigned)nblocks), dim3(32, 8), 0, (hipStream_t)stream, jobs, block_job);
    return check_launch("transpose_batch_kernel");
}
extern "C" int mny_transpose_batch_bf16(const mny_transpose_job* jobs, const int32_t* block_job, int nblocks, void* stream) {
    MNY_REQUIRE(jobs && block_job && nblocks > 0, "transpose_batch: bad arguments");
    hipLaunchKernelGGL((transpose_batch_kernel<bf16_t>), dim3((unsigned)nblocks), dim3(32, 8), 0, (hipStream_t)stream, jobs, block_job);
    return check_launch("transpose_batch_kernel<bf16>");
}

extern "C" int mny_transpose(const float* src, float* dst, int R, int Cc, void* stream) {
    MNY_REQUIRE(src && dst && R > 0 && Cc > 0, "transpose: bad arguments");
    hipLaunchKernelGGL((transpose_kernel<float>), dim3((unsigned)cdiv(Cc, 32), (unsigned)cdiv(R, 32)), dim3(32, 8), 0, (hipStream_t)stream, src, dst, R, Cc, R);
    return check_launch("transpose_kernel");
}
extern "C" int mny_transpose_pad(const float* src, float* dst, int R, int Cc, int Rp, void* stream) {
    MNY_REQUIRE(src && dst && R > 0 && Cc > 0 && Rp >= R, "transpose_pad: bad arguments");
    hipLaunchKernelGGL((transpose_kernel<float>), dim3((unsigned)cdiv(Cc, 32), (unsigned)cdiv(Rp, 32)), dim3(32, 8), 0, (hipStream_t)stream, src, dst, R, Cc, Rp);
    return check_launch("transpose_kernel<pad>");
}
extern "C" int mny_transpose_pad_bf16(const float* src, void* dst, int R, int Cc, int Rp, void* stream) {
    MNY_REQUIRE(src && dst && R > 0 && Cc > 0 && Rp >= R, "transpose_pad: bad arguments");
    hipLaunchKernelGGL((transpose_kernel<bf16_t>), dim3((unsigned)cdiv(Cc, 32), (unsigned)cdiv(Rp, 32)), dim3(32, 8), 0, (hipStream_t)stream, src,
                       (bf16_t*)dst, R, Cc, Rp);
    return check_launch("transpose_kernel<pad,bf16>");
}
extern "C" int mny_transpose_bf16(const float* src, void* dst, int R, int Cc, void* stream) {
    MNY_REQUIRE(src && dst && R > 0 && Cc > 0, "transpose: bad arguments");
    hipLaunchKernelGGL((transpose_kernel<bf16_t>), dim3((unsigned)cdiv(Cc, 32), (unsigned)cdiv(R, 32)), dim3(32, 8), 0, (hipStream_t)stream, src,
                       (bf16_t*)dst, R, Cc, R);
    return check_launch("transpose_kernel<bf16>");
}
