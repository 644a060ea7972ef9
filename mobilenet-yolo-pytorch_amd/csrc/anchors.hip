// Fitting YOLO anchors to a label set on the device (include/mnyolo.h "Anchor fitting"): k-means under the shape IoU, the fitness of
// many candidate anchor sets in one launch, a mutation search on top of it, and a census of what the loss's target assignment
// (detect.hip yolo_assign_kernel) will do with a set of anchors.  The arithmetic is specified in the header; this file is compiled with
// -ffp-contract=off so that every product, sum and quotient below is an fp32 operation of its own, and every sum that crosses lanes
// or workgroups is an integer (fixed point), so no result depends on the launch geometry or on the order of the atomics.
//
// Geometry: a 256-thread workgroup owns tiles of 1024 boxes; a lane keeps four of them (two 16-byte loads) in registers with their
// areas and walks the candidate sets, whose anchors sit in LDS as (aw, ah, aw * ah) and are read at one address by all lanes (a
// broadcast).  A lane's fixed-point sum is reduced across the wave with shuffles, kept per wave in LDS over the workgroup's tiles, and
// leaves the workgroup as one 64-bit integer atomicAdd per accumulator.  The work is the IoU arithmetic (two min, two products, an
// add, a subtract and a correctly rounded division per box and anchor), not memory: the boxes are read once per launch.
#include "common.h"
#include "iou.h"

namespace mny {
namespace {

typedef unsigned long long ull;

constexpr int kAnThreads = 256;
constexpr int kAnWaves = kAnThreads / kWave;
constexpr int kAnBoxes = 4;                         // per lane
constexpr int kAnTile = kAnThreads * kAnBoxes;      // boxes per workgroup and pass
constexpr int kAnMaxGrid = 512;                     // two workgroups per CU; larger label sets take the grid-stride loop
constexpr int kAnMaxK = 32;
constexpr int kAnMaxP = 256;
constexpr int64_t kAnMaxN = (int64_t)1 << 22;
constexpr int kAnStage = 1024;                      // anchors per LDS stage (16 KB): at least 32 candidate sets
constexpr float kAnMinSide = 0x1p-20f, kAnMaxSide = 65536.f;
// workspace: kacc[32][3] | facc[256][2] | cand[P][k][2]
constexpr size_t kAnKaccOff = 0, kAnFaccOff = kAnMaxK * 3 * 8, kAnCandOff = kAnFaccOff + kAnMaxP * 2 * 8;
constexpr int kCeMaxAnchors = 64, kCeMaxHeads = 4, kCeMaxPerHead = 16, kCeMaxT = 1 << 24;

__device__ __forceinline__ long long q_shape(float x) { return __double2ll_rn((double)x * 16777216.0); }
__device__ __forceinline__ long long q_iou(float v) { return __double2ll_rn((double)v * 4294967296.0); }
__device__ __forceinline__ bool side_ok(float s) { return s >= kAnMinSide && s <= kAnMaxSide; }      // false for NaN

__device__ __forceinline__ ull wave_sum64(ull v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ ull wave_max64(ull v) {
    for (int o = 32; o; o >>= 1) {
        const ull u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the four boxes of a lane: slots 2i and 2i + 1 are the neighbours at tile0 + (i * 256 + tid) * 2.  A box past the end is neither
// present nor valid; an invalid box computes on (1, 1) and is masked out of every result.
struct Boxes {
    float w[kAnBoxes], h[kAnBoxes], area[kAnBoxes];
    uint32_t present, valid;                        // bit per slot
};
__device__ __forceinline__ int64_t box_index(int64_t tile0, int tid, int slot) { return tile0 + ((slot >> 1) * kAnThreads + tid) * 2 + (slot & 1); }
__device__ __forceinline__ void load_boxes(const float* __restrict__ wh, int64_t N, int64_t tile0, int tid, Boxes& bx) {
    bx.present = bx.valid = 0;
#pragma unroll
    for (int i = 0; i < kAnBoxes / 2; ++i) {
        const int64_t idx = box_index(tile0, tid, 2 * i);
        float4 v = f4zero();
        if (idx + 1 < N) {
            v = ld4(wh + idx * 2);
            bx.present |= 3u << (2 * i);
        } else if (idx < N) {
            const float2 t = *reinterpret_cast<const float2*>(wh + idx * 2);
            v.x = t.x; v.y = t.y;
            bx.present |= 1u << (2 * i);
        }
        bx.w[2 * i] = v.x; bx.h[2 * i] = v.y; bx.w[2 * i + 1] = v.z; bx.h[2 * i + 1] = v.w;
    }
#pragma unroll
    for (int b = 0; b < kAnBoxes; ++b) {
        const bool ok = ((bx.present >> b) & 1u) && side_ok(bx.w[b]) && side_ok(bx.h[b]);
        if (ok) bx.valid |= 1u << b; else bx.w[b] = bx.h[b] = 1.f;
        bx.area[b] = bx.w[b] * bx.h[b];
    }
}

// anchors -> LDS as (aw, ah, aw * ah, -)
__device__ __forceinline__ void stage_anchors(const float* __restrict__ src, int count, float4* A) {
    for (int i = threadIdx.x; i < count; i += kAnThreads) {
        const float aw = src[2 * i], ah = src[2 * i + 1];
        A[i] = make_float4(aw, ah, aw * ah, 0.f);
    }
}

// best = the lowest index with the largest IoU (strict >, from -inf; a NaN never wins)
__device__ __forceinline__ void best_of(const Boxes& bx, const float4* A, int k, float* bv, int* bi) {
#pragma unroll
    for (int b = 0; b < kAnBoxes; ++b) { bv[b] = -INFINITY; bi[b] = 0; }
    for (int j = 0; j < k; ++j) {
        const float4 a = A[j];
#pragma unroll
        for (int b = 0; b < kAnBoxes; ++b) {
            const float v = shape_iou(bx.w[b], bx.h[b], bx.area[b], a.x, a.y, a.z);
            if (v > bv[b]) { bv[b] = v; bi[b] = j; }
        }
    }
}

__global__ void anchor_clear_kernel(ull* __restrict__ a, int na, ull* __restrict__ b, int nb) {
    for (int i = threadIdx.x; i < na; i += blockDim.x) a[i] = 0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) b[i] = 0;
}

// ---- k-means ---------------------------------------------------------------------------------------------------------------------
// FINAL = false: one assignment pass into kacc[k][3] = (S_w, S_h, n); returns at once after convergence (state[1]), when a step is the
// identity.  FINAL = true: labels, best_iou and the skipped count.
template <bool FINAL>
__global__ __launch_bounds__(kAnThreads) void anchor_assign_kernel(const float* __restrict__ wh, int64_t N, const float* __restrict__ centres, int k,
                                                                   ull* __restrict__ kacc, long long* __restrict__ state,
                                                                   int32_t* __restrict__ labels, float* __restrict__ best_iou) {
    __shared__ float4 A[kAnMaxK];
    __shared__ ull part[kAnWaves][kAnMaxK][3];
    __shared__ uint32_t skip_s[kAnWaves];
    if (!FINAL && state[1]) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    stage_anchors(centres, k, A);
    for (int i = tid; i < kAnWaves * kAnMaxK * 3; i += kAnThreads) (&part[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t nskip = 0;
    const int64_t tiles = cdiv(N, kAnTile);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        Boxes bx;
        load_boxes(wh, N, tile * kAnTile, tid, bx);
        float bv[kAnBoxes];
        int bi[kAnBoxes];
        best_of(bx, A, k, bv, bi);
        if (FINAL) {
#pragma unroll
            for (int b = 0; b < kAnBoxes; ++b) {
                if (!((bx.present >> b) & 1u)) continue;
                const bool ok = (bx.valid >> b) & 1u;
                const int64_t idx = box_index(tile * kAnTile, tid, b);
                labels[idx] = ok ? bi[b] : -1;
                if (best_iou) best_iou[idx] = ok ? bv[b] : 0.f;
                nskip += !ok;
            }
        } else {
            long long qw[kAnBoxes], qh[kAnBoxes];
#pragma unroll
            for (int b = 0; b < kAnBoxes; ++b) {
                const bool ok = (bx.valid >> b) & 1u;
                qw[b] = ok ? q_shape(bx.w[b]) : 0;
                qh[b] = ok ? q_shape(bx.h[b]) : 0;
                if (!ok) bi[b] = -1;
            }
            for (int c = 0; c < k; ++c) {
                ull sw = 0, sh = 0;
                uint32_t n = 0;
#pragma unroll
                for (int b = 0; b < kAnBoxes; ++b) {
                    const bool mine = bi[b] == c;
                    sw += mine ? (ull)qw[b] : 0ull;
                    sh += mine ? (ull)qh[b] : 0ull;
                    n += mine;
                }
                sw = wave_sum64(sw);
                sh = wave_sum64(sh);
                n = wave_sum32(n);
                if (lane == 0) { part[wave][c][0] += sw; part[wave][c][1] += sh; part[wave][c][2] += n; }
            }
        }
    }
    if (FINAL) {
        nskip = wave_sum32(nskip);
        if (lane == 0) skip_s[wave] = nskip;
        __syncthreads();
        if (tid == 0) {
            ull s = 0;
            for (int wv = 0; wv < kAnWaves; ++wv) s += skip_s[wv];
            if (s) atomicAdd((ull*)state + 2, s);
        }
        return;
    }
    __syncthreads();
    for (int i = tid; i < k * 3; i += kAnThreads) {
        ull s = 0;
        for (int wv = 0; wv < kAnWaves; ++wv) s += (&part[wv][0][0])[i];
        if (s) atomicAdd(kacc + i, s);
    }
}

// one workgroup: the new centres from the sums, the convergence flag, and the accumulators cleared for the next step
__global__ __launch_bounds__(kWave) void anchor_update_kernel(float* __restrict__ centres, int k, ull* __restrict__ kacc, long long* __restrict__ state) {
    if (state[1]) return;
    const int c = threadIdx.x;
    int changed = 0;
    if (c < k) {
        const long long sw = (long long)kacc[c * 3], sh = (long long)kacc[c * 3 + 1], n = (long long)kacc[c * 3 + 2];
        kacc[c * 3] = kacc[c * 3 + 1] = kacc[c * 3 + 2] = 0;
        if (n > 0) {
            const float nw = (float)(((double)sw / (double)n) * 0x1p-24);
            const float nh = (float)(((double)sh / (double)n) * 0x1p-24);
            changed = __float_as_uint(nw) != __float_as_uint(centres[2 * c]) || __float_as_uint(nh) != __float_as_uint(centres[2 * c + 1]);
            centres[2 * c] = nw;
            centres[2 * c + 1] = nh;
        }
    }
    changed = __syncthreads_or(changed);
    if (c == 0) {
        state[0] += 1;
        if (!changed) state[1] = 1;
    }
}

// ---- fitness of P candidate sets -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAnThreads) void anchor_fitness_kernel(const float* __restrict__ wh, int64_t N, const float* __restrict__ cand, int P, int k,
                                                                    float thr, ull* __restrict__ acc, ull* __restrict__ valid_out) {
    __shared__ float4 A[kAnStage];
    __shared__ ull part[kAnWaves][kAnMaxP][2];
    __shared__ uint32_t valid_s[kAnWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kAnWaves * kAnMaxP * 2; i += kAnThreads) (&part[0][0][0])[i] = 0;
    const int pc = kAnStage / k;                    // candidate sets per stage
    int staged = -1;
    uint32_t nvalid = 0;
    const int64_t tiles = cdiv(N, kAnTile);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        Boxes bx;
        load_boxes(wh, N, tile * kAnTile, tid, bx);
        nvalid += __popc(bx.valid);
        for (int p0 = 0; p0 < P; p0 += pc) {
            const int np = P - p0 < pc ? P - p0 : pc;
            if (staged != p0) {                     // uniform: with P <= pc the one stage is filled once
                __syncthreads();
                stage_anchors(cand + (size_t)p0 * k * 2, np * k, A);
                staged = p0;
                __syncthreads();
            }
            for (int p = 0; p < np; ++p) {
                float bv[kAnBoxes];
                int bi[kAnBoxes];
                best_of(bx, A + p * k, k, bv, bi);
                ull s = 0;
                uint32_t hits = 0;
#pragma unroll
                for (int b = 0; b < kAnBoxes; ++b) {
                    const bool hit = ((bx.valid >> b) & 1u) && bv[b] > thr;
                    s += hit ? (ull)q_iou(bv[b]) : 0ull;
                    hits += hit;
                }
                s = wave_sum64(s);
                hits = wave_sum32(hits);
                if (lane == 0) { part[wave][p0 + p][0] += s; part[wave][p0 + p][1] += hits; }
            }
        }
    }
    nvalid = wave_sum32(nvalid);
    if (lane == 0) valid_s[wave] = nvalid;
    __syncthreads();
    for (int i = tid; i < P * 2; i += kAnThreads) {
        ull s = 0;
        for (int wv = 0; wv < kAnWaves; ++wv) s += (&part[wv][0][0])[i];
        if (s) atomicAdd(acc + i, s);
    }
    if (valid_out && tid == 0) {
        ull s = 0;
        for (int wv = 0; wv < kAnWaves; ++wv) s += valid_s[wv];
        if (s) atomicAdd(valid_out, s);
    }
}

// ---- evolution: one workgroup between two fitness launches ---------------------------------------------------------------------------
// g < 0: the parent is anchors_in.  g >= 0: the parent is the candidate of generation g with the largest F (lowest p on a tie), which
// goes to history[g].  Then the candidates of generation g + 1 are built and the accumulators cleared; after the last generation the
// parent goes to anchors_out.
__global__ __launch_bounds__(kAnThreads) void anchor_evolve_step_kernel(int g, int G, int P, int k, const float* __restrict__ factors, float min_size,
                                                                        float* __restrict__ cand, ull* __restrict__ facc,
                                                                        long long* __restrict__ history, const float* __restrict__ anchors_in,
                                                                        float* __restrict__ anchors_out) {
    __shared__ ull key_s[kAnWaves];
    __shared__ float par[kAnMaxK * 2];
    const int tid = threadIdx.x, k2 = 2 * k;
    if (g < 0) {
        if (tid < k2) par[tid] = anchors_in[tid];
    } else {
        // F < 2^55 (2^22 boxes of at most 2^32 + 1 each): F and the index share one key whose maximum is the winner
        ull key = tid < P ? (facc[2 * tid] << 8) | (ull)(255 - tid) : 0ull;
        key = wave_max64(key);
        if ((tid & 63) == 0) key_s[tid >> 6] = key;
        __syncthreads();
        key = key_s[0];
        for (int wv = 1; wv < kAnWaves; ++wv) key = key_s[wv] > key ? key_s[wv] : key;
        const int win = 255 - (int)(key & 255ull);
        if (tid == 0) { history[2 * g] = (long long)(key >> 8); history[2 * g + 1] = win; }
        if (tid < k2) par[tid] = cand[(size_t)win * k2 + tid];
    }
    __syncthreads();                                // the parent is in LDS, every read of cand and facc is done
    const int next = g + 1;
    if (next < G) {
        const float* f = factors + (size_t)next * P * k2;
        for (int i = tid; i < P * k2; i += kAnThreads) {
            const int j = i % k2;
            cand[i] = i < k2 ? par[j] : fmaxf(par[j] * f[i], min_size);
        }
    } else if (tid < k2) {
        anchors_out[tid] = par[tid];
    }
    for (int i = tid; i < 2 * P; i += kAnThreads) facc[i] = 0;
}

// ---- census ----------------------------------------------------------------------------------------------------------------------
struct CensusArgs {
    int32_t n, H, A;
    int32_t g[kCeMaxHeads];
    int32_t mask[kCeMaxHeads * kCeMaxPerHead];
    float iou_thresh;
};
constexpr int kCeSlots = kCeMaxAnchors + kCeMaxHeads * kCeMaxPerHead + 1 + kCeMaxHeads;

// one thread per target, the decisions of yolo_assign_kernel (detect.hip) line by line; out = best[n] | pos[H][A] | orphans | outside[H]
__global__ __launch_bounds__(kAnThreads) void anchor_census_kernel(const float* __restrict__ targets, int64_t T, const float* __restrict__ anchors,
                                                                   const CensusArgs a, ull* __restrict__ out) {
    __shared__ uint32_t cnt[kCeSlots];
    __shared__ float2 anc[kCeMaxAnchors];
    const int tid = threadIdx.x;
    const int pos0 = a.n, orph = a.n + a.H * a.A, out0 = orph + 1, slots = out0 + a.H;
    for (int i = tid; i < slots; i += kAnThreads) cnt[i] = 0;
    for (int i = tid; i < a.n; i += kAnThreads) anc[i] = make_float2(anchors[2 * i], anchors[2 * i + 1]);
    __syncthreads();
    for (int64_t t = (int64_t)blockIdx.x * kAnThreads + tid; t < T; t += (int64_t)gridDim.x * kAnThreads) {
        const float* q = targets + t * 5;
        const float gw = q[3], gh = q[4];
        int best_n = 0;
        float best_v = -INFINITY;
        const Box sb{0.f, 0.f, gw, gh};
        for (int k = 0; k < a.n; ++k) {
            const Box ab{0.f, 0.f, anc[k].x, anc[k].y};
            const float v = iou_ref(sb, ab);
            if (v > best_v || (v != v && best_v == best_v)) { best_v = v; best_n = k; }
        }
        atomicAdd(&cnt[best_n], 1u);
        bool any = false;
        for (int h = 0; h < a.H; ++h) {
            const int g = a.g[h];
            const int gi = (int)(q[1] * (float)g), gj = (int)(q[2] * (float)g);
            if (gi < 0 || gi >= g || gj < 0 || gj >= g) {
                atomicAdd(&cnt[out0 + h], 1u);
                continue;
            }
            for (int k = 0; k < a.A; ++k) {
                const int am = a.mask[h * a.A + k];
                const Box ab{0.f, 0.f, anc[am].x, anc[am].y};
                const bool hit = (am == best_n) || (iou_ref(sb, ab) > a.iou_thresh);
                if (hit) {
                    atomicAdd(&cnt[pos0 + h * a.A + k], 1u);
                    any = true;
                }
            }
        }
        if (!any) atomicAdd(&cnt[orph], 1u);
    }
    __syncthreads();
    for (int i = tid; i < slots; i += kAnThreads)
        if (cnt[i]) atomicAdd(out + i, (ull)cnt[i]);
}

int an_check(const char* who, const float* wh, int64_t N, int k, int P) {
    MNY_REQUIRE(k >= 1 && k <= kAnMaxK, "%s: k = %d outside 1..%d", who, k, kAnMaxK);
    MNY_REQUIRE(N >= 1 && N <= kAnMaxN, "%s: N = %lld outside 1..2^22", who, (long long)N);
    MNY_REQUIRE(P >= 1 && P <= kAnMaxP, "%s: P = %d outside 1..%d", who, P, kAnMaxP);
    MNY_REQUIRE(wh, "%s: null pointer", who);
    MNY_REQUIRE(((uintptr_t)wh & 15) == 0, "%s: wh must be 16-byte aligned", who);
    return MNY_OK;
}
int an_grid(int64_t N) {
    const int64_t tiles = cdiv(N, kAnTile);
    return (int)(tiles < kAnMaxGrid ? tiles : kAnMaxGrid);
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_anchor_ws_bytes(int k, int P) {
    if (k < 1 || k > kAnMaxK || P < 1 || P > kAnMaxP) {
        set_error("mny_anchor_ws_bytes: k = %d outside 1..%d or P = %d outside 1..%d", k, kAnMaxK, P, kAnMaxP);
        return 0;
    }
    return kAnCandOff + (size_t)P * k * 2 * sizeof(float);
}

extern "C" int mny_anchor_kmeans(const float* wh, int64_t N, float* centres, int k, int max_iter, int32_t* labels, float* best_iou,
                                 int64_t* state, void* ws, void* stream) {
    if (const int rc = an_check("mny_anchor_kmeans", wh, N, k, 1)) return rc;
    MNY_REQUIRE(max_iter >= 0 && max_iter <= 100000, "mny_anchor_kmeans: max_iter = %d outside 0..100000", max_iter);
    MNY_REQUIRE(centres && labels && state && ws, "mny_anchor_kmeans: null pointer");
    MNY_REQUIRE((((uintptr_t)state | (uintptr_t)ws) & 7) == 0, "mny_anchor_kmeans: state and ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ull* kacc = (ull*)((char*)ws + kAnKaccOff);
    long long* s = (long long*)state;
    const dim3 grid(an_grid(N)), block(kAnThreads);
    anchor_clear_kernel<<<1, 128, 0, st>>>(kacc, kAnMaxK * 3, (ull*)state, 4);
    for (int it = 0; it < max_iter; ++it) {
        anchor_assign_kernel<false><<<grid, block, 0, st>>>(wh, N, centres, k, kacc, s, nullptr, nullptr);
        anchor_update_kernel<<<1, kWave, 0, st>>>(centres, k, kacc, s);
    }
    anchor_assign_kernel<true><<<grid, block, 0, st>>>(wh, N, centres, k, kacc, s, labels, best_iou);
    return check_launch("mny_anchor_kmeans");
}

extern "C" int mny_anchor_fitness(const float* wh, int64_t N, const float* cand, int P, int k, float thr, int64_t* out, int64_t* valid,
                                  void* stream) {
    if (const int rc = an_check("mny_anchor_fitness", wh, N, k, P)) return rc;
    MNY_REQUIRE(cand && out && valid, "mny_anchor_fitness: null pointer");
    MNY_REQUIRE((((uintptr_t)out | (uintptr_t)valid) & 7) == 0, "mny_anchor_fitness: out and valid must be 8-byte aligned");
    MNY_REQUIRE(thr == thr, "mny_anchor_fitness: thr is NaN");
    hipStream_t st = (hipStream_t)stream;
    anchor_clear_kernel<<<1, 128, 0, st>>>((ull*)out, 2 * P, (ull*)valid, 1);
    anchor_fitness_kernel<<<dim3(an_grid(N)), dim3(kAnThreads), 0, st>>>(wh, N, cand, P, k, thr, (ull*)out, (ull*)valid);
    return check_launch("mny_anchor_fitness");
}

extern "C" int mny_anchor_evolve(const float* wh, int64_t N, const float* anchors_in, int k, const float* factors, int G, int P, float thr,
                                 float min_size, float* anchors_out, int64_t* history, void* ws, void* stream) {
    if (const int rc = an_check("mny_anchor_evolve", wh, N, k, P)) return rc;
    MNY_REQUIRE(G >= 1 && G <= 1000000, "mny_anchor_evolve: G = %d outside 1..1000000", G);
    MNY_REQUIRE(anchors_in && factors && anchors_out && history && ws, "mny_anchor_evolve: null pointer");
    MNY_REQUIRE((((uintptr_t)history | (uintptr_t)ws) & 7) == 0, "mny_anchor_evolve: history and ws must be 8-byte aligned");
    MNY_REQUIRE(thr == thr, "mny_anchor_evolve: thr is NaN");
    MNY_REQUIRE(min_size >= kAnMinSide && min_size <= kAnMaxSide, "mny_anchor_evolve: min_size %g outside 2^-20..65536", (double)min_size);
    hipStream_t st = (hipStream_t)stream;
    ull* facc = (ull*)((char*)ws + kAnFaccOff);
    float* cand = (float*)((char*)ws + kAnCandOff);
    const dim3 grid(an_grid(N)), block(kAnThreads);
    for (int g = -1; g < G; ++g) {
        anchor_evolve_step_kernel<<<1, block, 0, st>>>(g, G, P, k, factors, min_size, cand, facc, (long long*)history, anchors_in, anchors_out);
        if (g + 1 < G) anchor_fitness_kernel<<<grid, block, 0, st>>>(wh, N, cand, P, k, thr, facc, nullptr);
    }
    return check_launch("mny_anchor_evolve");
}

extern "C" int mny_anchor_census(const float* targets, int64_t T, const float* anchors_all, int n, const int32_t* mask, const int32_t* grids,
                                 int H, int A, float iou_thresh, int64_t* out, void* stream) {
    MNY_REQUIRE(n >= 1 && n <= kCeMaxAnchors, "mny_anchor_census: %d anchors outside 1..%d", n, kCeMaxAnchors);
    MNY_REQUIRE(H >= 1 && H <= kCeMaxHeads && A >= 1 && A <= kCeMaxPerHead, "mny_anchor_census: %d heads of %d anchors outside 1..%d x 1..%d", H, A,
                kCeMaxHeads, kCeMaxPerHead);
    MNY_REQUIRE(T >= 0 && T <= kCeMaxT, "mny_anchor_census: T = %lld outside 0..2^24", (long long)T);
    MNY_REQUIRE(anchors_all && mask && grids && out && (targets || T == 0), "mny_anchor_census: null pointer");
    MNY_REQUIRE(((uintptr_t)out & 7) == 0, "mny_anchor_census: out must be 8-byte aligned");
    MNY_REQUIRE(iou_thresh == iou_thresh, "mny_anchor_census: iou_thresh is NaN");
    CensusArgs a;
    a.n = n; a.H = H; a.A = A; a.iou_thresh = iou_thresh;
    for (int h = 0; h < H; ++h) {
        MNY_REQUIRE(grids[h] >= 1 && grids[h] <= 4096, "mny_anchor_census: grid %d of head %d outside 1..4096", grids[h], h);
        a.g[h] = grids[h];
        for (int k = 0; k < A; ++k) {
            const int am = mask[h * A + k];
            MNY_REQUIRE(am >= 0 && am < n, "mny_anchor_census: mask[%d][%d] = %d names none of the %d anchors", h, k, am, n);
            a.mask[h * A + k] = am;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    anchor_clear_kernel<<<1, 128, 0, st>>>((ull*)out, n + H * A + 1 + H, nullptr, 0);
    if (T > 0) {
        const int64_t blocks = cdiv(T, kAnThreads);
        anchor_census_kernel<<<dim3((unsigned)(blocks < kAnMaxGrid ? blocks : kAnMaxGrid)), dim3(kAnThreads), 0, st>>>(targets, T, anchors_all, a,
                                                                                                                      (ull*)out);
    }
    return check_launch("mny_anchor_census");
}
