// Pointwise (1x1) convolution, forward / data gradient, first generation: the register-staged NT kernel behind the MNY_ROUTE_TILE_V1 family
// (any K, fp32 or bf16 storage: the 75-channel heads' data gradient, the 10-channel gate, MNY_GEMM_V1 runs).  The second generation — the
// LDS-DMA ring kernel that takes every 16-byte-aligned K — is pwnt_kernel.h.
//
//   C[M,N] = act_in(A)[M,K] * B[N,K]^T (+bias)(+addend)      ("NT")
//
// v_mfma_f32_32x32x2_f32 (exact fp32, 157 TFLOP/s peak = 64 cyc per instruction per SIMD).
// One MFMA consumes a single A and B dword per lane, so LDS/L1 bandwidth is never the limiter in fp32:
// the kernel is kept simple (one barrier per K tile) and spends its effort on (i) fusing the
// producer's BatchNorm-apply + activation into the A load, (ii) fusing the BatchNorm statistics of
// the output into the epilogue, and (iii) exposing enough independent workgroups (>> 256 CUs).
//
// NT kernel: 256 threads = 4 waves stacked along M (32 rows each, BM = 128), every wave spans the
// whole BN = 32*TN tile (TN = 1..4 accumulators of 32x32).  A and B tiles are staged
// global -> registers (float4, transform applied) -> LDS with a row pitch of BK+4 floats, which makes
// the ds_read_b128 fragment reads bank-conflict free (pitch 20 -> 16 distinct 4-bank slots per lane group).
// Fragment trick: lanes with k-half h read the float4 at k = 8*kc + 4*h; MFMA j of the chunk then
// contracts k in {8kc+j, 8kc+4+j} — any consistent permutation of K is a valid contraction order.
#include "pwgemm.h"
#include "x6.h"

namespace mny {

constexpr int BM = 128;      // rows of a workgroup's tile (pwnt_kernel.h, which this unit does not include, has a BM of its own with the same value)

struct GemmArgs {   // A / addend / C are T* (float or bf16_t) of the kernel instantiation, B is T* as well
    const void* A; const float* in_scale; const float* in_shift; int in_act;
    const void* B; const float* bias; const void* addend; void* C; float* stats;
    int64_t M; int K; int N;
    int m_tiles; int tiles_per_block;
};

template <typename T, int TN, int BK>
__global__ __launch_bounds__(256) void pw_gemm_nt_kernel(GemmArgs p) {
    constexpr int BN = 32 * TN;
    const T* pA = (const T*)p.A;
    const T* pAdd = (const T*)p.addend;
    T* pC = (T*)p.C;
    constexpr int LDP = BK + 4;   // LDS row pitch (floats): 20 / 36 -> conflict-free ds_read_b128 fragments
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                           // [2][BM][LDP]
    float* Bs = smem + 2 * BM * LDP;            // [2][BN][LDP]
    float* sScale = Bs + 2 * BN * LDP;          // [Kpad]
    const int Kpad = (p.K + BK - 1) / BK * BK;
    float* sShift = sScale + Kpad;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lrow = lane & 31;
    const int khalf = lane >> 5;
    const int n0 = blockIdx.y * BN;
    const bool has_xf = p.in_scale != nullptr;
    const bool do_xf = has_xf || p.in_act != MNY_ACT_NONE;
    const bool kvec = (p.K & 3) == 0;   // rows 16-B aligned -> float4 loads; else scalar tail-safe loads

    if (do_xf) {                                  // (the host sizes the LDS without this area when !do_xf)
        for (int k = tid; k < Kpad; k += 256) {
            sScale[k] = (has_xf && k < p.K) ? p.in_scale[k] : 1.f;
            sShift[k] = (has_xf && k < p.K) ? p.in_shift[k] : 0.f;
        }
        __syncthreads();
    }

    // staging assignment: A tile = BM*BK/4 = 512 float4 -> 2 per thread; B tile = BN*BK/4 -> TN/2 per thread
    constexpr int A_PER = BM * BK / 4 / 256;
    constexpr int B_F4 = BN * BK / 4;
    constexpr int B_PER = (B_F4 + 255) / 256;
    const int nk = Kpad / BK;

    float s1[TN], s2[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) { s1[t] = 0.f; s2[t] = 0.f; }

    const int mt_begin = blockIdx.x * p.tiles_per_block;
    const int mt_end = min(mt_begin + p.tiles_per_block, p.m_tiles);

    for (int mt = mt_begin; mt < mt_end; ++mt) {
        const int64_t m0 = (int64_t)mt * BM;
        f32x16 acc[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

        float4 ra[A_PER], rb[B_PER];
        auto gload = [&](int kt) {
            const int k0 = kt * BK;
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const int idx = tid + i * 256;
                const int row = idx / (BK / 4), kq = idx % (BK / 4);
                const int64_t m = m0 + row;
                const int k = k0 + kq * 4;
                float4 v = f4zero();
                if (m < p.M && k < p.K) {
                    const T* src = pA + m * p.K + k;
                    if (kvec) v = ld4(src);
                    else { v.x = ld1(src); if (k + 1 < p.K) v.y = ld1(src + 1); if (k + 2 < p.K) v.z = ld1(src + 2); if (k + 3 < p.K) v.w = ld1(src + 3); }
                    if (do_xf) {
                        v = xform4(v, ld4(sScale + k), ld4(sShift + k), p.in_act);
                        if (!kvec) { if (k + 1 >= p.K) v.y = 0.f; if (k + 2 >= p.K) v.z = 0.f; if (k + 3 >= p.K) v.w = 0.f; }
                    }
                }
                ra[i] = v;
            }
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                const int idx = tid + i * 256;
                float4 v = f4zero();
                if (idx < B_F4) {
                    const int row = idx / (BK / 4), kq = idx % (BK / 4);
                    const int n = n0 + row;
                    const int k = k0 + kq * 4;
                    if (n < p.N && k < p.K) {
                        const T* src = (const T*)p.B + (int64_t)n * p.K + k;
                        if (kvec) v = ld4(src);
                        else { v.x = ld1(src); if (k + 1 < p.K) v.y = ld1(src + 1); if (k + 2 < p.K) v.z = ld1(src + 2); if (k + 3 < p.K) v.w = ld1(src + 3); }
                    }
                }
                rb[i] = v;
            }
        };
        auto lstore = [&](int buf) {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const int idx = tid + i * 256;
                const int row = idx / (BK / 4), kq = idx % (BK / 4);
                st4(As + (buf * BM + row) * LDP + kq * 4, ra[i]);
            }
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                const int idx = tid + i * 256;
                if (idx < B_F4) {
                    const int row = idx / (BK / 4), kq = idx % (BK / 4);
                    st4(Bs + (buf * BN + row) * LDP + kq * 4, rb[i]);
                }
            }
        };

        gload(0);
        lstore(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) gload(kt + 1);
            const float* a_base = As + (buf * BM + wave * 32 + lrow) * LDP + khalf * 4;
            const float* b_base = Bs + (buf * BN + lrow) * LDP + khalf * 4;
#pragma unroll
            for (int kc = 0; kc < BK / 8; ++kc) {
                const float4 af = ld4(a_base + kc * 8);
                float4 bf[TN];
#pragma unroll
                for (int t = 0; t < TN; ++t) bf[t] = ld4(b_base + t * 32 * LDP + kc * 8);
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf[t].x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf[t].y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf[t].z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf[t].w, acc[t], 0, 0, 0);
                }
            }
            if (kt + 1 < nk) lstore(buf ^ 1);
            __syncthreads();
        }

        // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const int col = n0 + t * 32 + lrow;
            const bool cok = col < p.N;
            const float bv = (p.bias && cok) ? p.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                float v = acc[t][r] + bv;
                if (cok && row < p.M) {
                    if (pAdd) v += ld1(pAdd + row * p.N + col);
                    st1(pC + row * p.N + col, v);
                    v = stored<T>(v);
                    s1[t] += v;
                    s2[t] = fmaf(v, v, s2[t]);
                }
            }
        }
    }

    if (p.stats) {
        // lanes l and l^32 hold the same column; then the 4 waves are summed in a fixed order via LDS
        __syncthreads();
        float* red = smem;   // [4][BN][2]
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const float a = s1[t] + __shfl_xor(s1[t], 32);
            const float b = s2[t] + __shfl_xor(s2[t], 32);
            if (khalf == 0) {
                red[(wave * BN + t * 32 + lrow) * 2 + 0] = a;
                red[(wave * BN + t * 32 + lrow) * 2 + 1] = b;
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < p.N) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { a += red[(w * BN + tid) * 2]; b += red[(w * BN + tid) * 2 + 1]; }
            p.stats[(int64_t)blockIdx.x * 2 * p.N + n0 + tid] = a;
            p.stats[(int64_t)blockIdx.x * 2 * p.N + p.N + n0 + tid] = b;
        }
    }
}

struct NtPlan { int TN; int BK; int n_tiles; int m_tiles; int gx; int tiles_per_block; size_t lds; };

static NtPlan nt_plan(int64_t M, int K, int N, bool xf = true) {
    NtPlan pl;
    int best = 1; int best_pad = 1 << 30;
    for (int tn = 4; tn >= 1; --tn) {   // minimise padded N; ties -> wider tile (fewer re-reads of A)
        int pad = (int)cdiv(N, 32 * tn) * 32 * tn;
        if (pad < best_pad) { best_pad = pad; best = tn; }
    }
    pl.TN = best;
    pl.n_tiles = (int)cdiv(N, 32 * best);
    pl.m_tiles = (int)cdiv(M, BM);
    int max_gx = kMaxParts;
    int gx = pl.m_tiles < max_gx ? pl.m_tiles : max_gx;
    pl.tiles_per_block = (int)cdiv(pl.m_tiles, gx);
    pl.gx = (int)cdiv(pl.m_tiles, pl.tiles_per_block);
    // deep K: BK = 32 halves the barriers per FLOP — as long as two blocks still fit the CU's 160 KB of LDS
    auto lds_for = [&](int bk) {
        const int Kpad = (int)cdiv(K, bk) * bk;
        return (size_t)(2 * BM * (bk + 4) + 2 * 32 * best * (bk + 4) + (xf ? 2 * Kpad : 0)) * sizeof(float);
    };
    pl.BK = (K >= 64 && K % 32 == 0 && lds_for(32) <= 80 * 1024) ? 32 : 16;
    pl.lds = lds_for(pl.BK);
    return pl;
}

// register-staged NT kernel (any K, any storage type)
template <typename T>
static int pw_fwd_v1(const T* x, const float* in_scale, const float* in_shift, int in_act, const T* w, const float* bias,
                     const T* addend, T* y, float* stats, int64_t M, int K, int Nc, hipStream_t st) {
    const bool xf = in_scale != nullptr || in_act != MNY_ACT_NONE;
    NtPlan pl = nt_plan(M, K, Nc, xf);
    MNY_REQUIRE(pl.lds <= 160 * 1024, "pw_fwd: K=%d too large for the LDS scale cache", K);
    GemmArgs a{x, in_scale, in_shift, in_act, w, bias, addend, y, stats, M, K, Nc, pl.m_tiles, pl.tiles_per_block};
    dim3 grid(pl.gx, pl.n_tiles), block(256);
    {                             // > 64 KB of dynamic LDS needs an explicit opt-in per kernel
        const void* ks[] = {(const void*)pw_gemm_nt_kernel<T, 1, 16>, (const void*)pw_gemm_nt_kernel<T, 2, 16>, (const void*)pw_gemm_nt_kernel<T, 3, 16>,
                            (const void*)pw_gemm_nt_kernel<T, 4, 16>, (const void*)pw_gemm_nt_kernel<T, 1, 32>, (const void*)pw_gemm_nt_kernel<T, 2, 32>,
                            (const void*)pw_gemm_nt_kernel<T, 3, 32>, (const void*)pw_gemm_nt_kernel<T, 4, 32>};
        for (const void* k : ks)
            if (!allow_lds(k, 160 * 1024)) {
                set_error("pw_fwd: hipFuncSetAttribute failed"); return MNY_EHIP;
            }
    }
#define MNY_NT(TN_, B) hipLaunchKernelGGL((pw_gemm_nt_kernel<T, TN_, B>), grid, block, pl.lds, st, a)
    switch (pl.TN * 100 + pl.BK) {
        case 116: MNY_NT(1, 16); break; case 216: MNY_NT(2, 16); break; case 316: MNY_NT(3, 16); break; case 416: MNY_NT(4, 16); break;
        case 132: MNY_NT(1, 32); break; case 232: MNY_NT(2, 32); break; case 332: MNY_NT(3, 32); break; default: MNY_NT(4, 32); break;
    }
#undef MNY_NT
    return check_launch("pw_gemm_nt_kernel");
}

// what pwgemm.h shows of this unit: the partial rows of a call, and the launch (bf: the operands are bf16_t)
int pw_v1_parts(int64_t M, int K, int N) { return nt_plan(M, K, N).gx; }

int pw_v1_launch(int bf, const void* x, const float* in_scale, const float* in_shift, int in_act, const void* w, const float* bias, const void* addend,
                 void* y, float* stats, int64_t M, int K, int N, hipStream_t st) {
    if (bf) return pw_fwd_v1<bf16_t>((const bf16_t*)x, in_scale, in_shift, in_act, (const bf16_t*)w, bias, (const bf16_t*)addend, (bf16_t*)y, stats, M, K, N, st);
    return pw_fwd_v1<float>((const float*)x, in_scale, in_shift, in_act, (const float*)w, bias, (const float*)addend, (float*)y, stats, M, K, N, st);
}

}  // namespace mny
