// The loader's blur / sharpen / noise stage on the device (include/mnyolo.h: mny_aug_seq_batch), the reference's imgaug
// `seq` (folder2lmdb.py:28-42) restated as uint8 -> uint8 stencils on the packed HWC batch.  The host made every draw.
//   stage 0 : op 0 of every image, src -> dst (one op) or src -> ws (two ops); images without an op are copied dword by
//             dword, images with a malformed record are written as zeros; block 0 also validates every record and writes the
//             status word
//   stage 1 : op 1 of the two-op images, ws -> dst
// One 256-thread workgroup works on one (image, 64x16 tile) at a time.  The job list is the prefix sum of the per-image tile
// counts, which every workgroup rebuilds in LDS from the descriptors (a few hundred records); the grid is capped and walks
// the list with a grid stride, so nothing is launched per max_h x max_w.  A tile and its 2-pixel halo are staged in LDS with
// aligned dword loads (rows keep their byte phase, 3*w is rarely a multiple of 4), borders are resolved by index when the
// taps are read, and the result goes through LDS again so that every dword that lies wholly inside the tile's row segment is
// stored as a dword.  No atomics, no scratch; fp32 without contraction (-ffp-contract=off) so that the arithmetic is the one
// the header states.
#include "common.h"

static_assert(sizeof(mny_aug_seq_item) == 64, "mny_aug_seq_item layout (augment.py SEQ)");
static_assert(sizeof(mny_image_desc) == 16, "mny_image_desc layout");

namespace mny {
namespace {

constexpr int kTW = 64, kTH = 16, kHalo = 2;
constexpr int kInRows = kTH + 2 * kHalo;                       // 20
constexpr int kInRowDw = (3 * (kTW + 2 * kHalo) + 3 + 3) / 4;  // 52 dwords hold 204 bytes at any phase
constexpr int kInStrideDw = kInRowDw + 1;                      // 53: odd stride
constexpr int kInStrideB = kInStrideDw * 4;
constexpr int kOutRowDw = (3 * kTW + 3 + 3) / 4;               // 49
constexpr int kOutStrideB = kOutRowDw * 4;
constexpr int kRowF = 3 * kTW;                                 // floats per row of the horizontal Gaussian pass
constexpr int kMaxItems = 4096;
constexpr int kMaxSide = 16383;                                // tiles per image < 2^18, per batch < 2^30
constexpr size_t kWsHead = 256;                                // status word, then the intermediate images laid out like src

enum { kOk = 0, kZero = 1, kSkip = 2 };

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool addressable(const mny_image_desc& d) {
    return d.offset >= 0 && d.h >= 1 && d.w >= 1 && d.h <= kMaxSide && d.w <= kMaxSide;
}

__device__ __forceinline__ int tiles_of(const mny_image_desc& d) { return ((d.w + kTW - 1) / kTW) * ((d.h + kTH - 1) / kTH); }

// kOk: run the ops; kZero: a malformed record whose bytes can be addressed, written as zeros; kSkip: no bytes to address
__device__ int classify(const mny_image_desc& d, const mny_aug_seq_item& q, int max_h, int max_w) {
    if (!addressable(d)) return kSkip;
    if ((d.offset & 3) || d.h > max_h || d.w > max_w) return kZero;
    if (q.n_ops < 0 || q.n_ops > 2) return kZero;
    if (q.n_ops == 2 && q.op[0] == q.op[1]) return kZero;
    for (int k = 0; k < q.n_ops; ++k) {
        const int op = q.op[k];
        if (op == MNY_SEQ_GAUSS) {
            for (int i = 0; i < 5; ++i)
                if (!finite_f(q.taps[i])) return kZero;
        } else if (op == MNY_SEQ_MEDIAN) {
            if (q.median_k != 3 && q.median_k != 5) return kZero;
        } else if (op == MNY_SEQ_SHARPEN) {
            if (!finite_f(q.sharpen_c) || !finite_f(q.sharpen_s)) return kZero;
        } else if (op == MNY_SEQ_NOISE) {
            if (!finite_f(q.noise_scale)) return kZero;
        } else {
            return kZero;
        }
    }
    return kOk;
}

// BORDER_REFLECT_101 (dcb|abcd|cba), iterated so that it holds for n = 1 and 2
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
__device__ __forceinline__ int replicate(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ void cx(us2& a, us2& b) {
    const us2 lo = __builtin_elementwise_min(a, b);
    b = __builtin_elementwise_max(a, b);
    a = lo;
}

// Median of N values by forgetful selection: of N/2 + 2 values neither the smallest nor the largest can be the median, so both are
// dropped and the next value joins, down to three.  Each round is a min/max network that moves the extremes to the ends; two
// 16-bit lanes per instruction.
template <int N, typename F>
__device__ __forceinline__ us2 median_select(F get) {
    constexpr int S = N / 2 + 2;
    us2 v[S];
#pragma unroll
    for (int i = 0; i < S; ++i) v[i] = get(i);
#pragma unroll
    for (int m = S; m >= 3; --m) {
#pragma unroll
        for (int i = 0; i < m / 2; ++i) cx(v[i], v[m - 1 - i]);
#pragma unroll
        for (int i = 1; i < (m + 1) / 2; ++i) cx(v[0], v[i]);
#pragma unroll
        for (int i = m / 2; i < m - 1; ++i) cx(v[i], v[m - 1]);
        if (m > 3) v[0] = get(S + (S - m));
    }
    return v[1];
}

// Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void philox(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t* r) {
    uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
__device__ __forceinline__ float unit(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 0x1p-24f; }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int round255(float v) {
    v = rintf(v);
    return (int)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

struct seq_lds {
    uint32_t pref[kMaxItems + 1];
    uint32_t part[256];
    uint32_t in[kInRows * kInStrideDw];
    uint32_t out[kTH * kOutRowDw];
    float hp[kInRows * kRowF];
    int in_ph[kInRows];
    int out_ph[kTH];
};

// one tile of one op: `in` -> `out` (both the image's 4-byte-aligned base), op = MNY_SEQ_*
__device__ void run_tile(seq_lds& S, const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const mny_aug_seq_item& q, int op, int h, int w, int ty0,
                         int tx0) {
    const int tid = threadIdx.x;
    const int64_t nbytes = (int64_t)3 * h * w;
    const int ry0 = max(ty0 - kHalo, 0), rh = min(ty0 + kTH + kHalo, h) - ry0;
    const int cx0 = max(tx0 - kHalo, 0), cw = min(tx0 + kTW + kHalo, w) - cx0;
    if (tid < rh) S.in_ph[tid] = (int)(((int64_t)(ry0 + tid) * 3 * w + 3 * cx0) & 3);
    if (tid < kTH) S.out_ph[tid] = (int)(((int64_t)(ty0 + tid) * 3 * w + 3 * tx0) & 3);
    // ---- stage the tile + halo: aligned dwords; the last, partial dword of the image is read by bytes
    for (int idx = tid; idx < rh * kInRowDw; idx += 256) {
        const int r = idx / kInRowDw, d = idx - r * kInRowDw;
        const int64_t g0 = (int64_t)(ry0 + r) * 3 * w + 3 * cx0;
        const int ph = (int)(g0 & 3);
        if (d * 4 >= ph + 3 * cw) continue;
        const int64_t a = (g0 - ph) + 4 * d;
        uint32_t v = 0;
        if (a + 4 <= nbytes) {
            v = *(const uint32_t*)(in + a);
        } else {
            for (int b = 0; b < 4; ++b)
                if (a + b < nbytes) v |= (uint32_t)in[a + b] << (8 * b);
        }
        S.in[r * kInStrideDw + d] = v;
    }
    __syncthreads();
    const uint8_t* sb = (const uint8_t*)S.in;
    const int ty = tid >> 4, tg = tid & 15;
    const int y = min(ty0 + ty, h - 1);
    const bool rep = op == MNY_SEQ_MEDIAN;
    int rowb[5], colo[4][5];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const int yy = (rep ? replicate(y + d - 2, h) : reflect101(y + d - 2, h)) - ry0;
        rowb[d] = yy * kInStrideB + S.in_ph[yy];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = min(tx0 + 4 * tg + p, w - 1);
#pragma unroll
        for (int d = 0; d < 5; ++d) colo[p][d] = 3 * ((rep ? replicate(x + d - 2, w) : reflect101(x + d - 2, w)) - cx0);
    }
    int o[12];
    if (op == MNY_SEQ_GAUSS) {
        float t[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) t[d] = q.taps[d];
        for (int idx = tid; idx < rh * kRowF; idx += 256) {                     // horizontal pass of every staged row, unrounded
            const int r = idx / kRowF, b = idx - r * kRowF;
            const int px = b / 3, c = b - 3 * px;
            const int x = min(tx0 + px, w - 1);
            const int base = r * kInStrideB + S.in_ph[r] + c;
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < 5; ++d) acc = acc + t[d] * (float)sb[base + 3 * (reflect101(x + d - 2, w) - cx0)];
            S.hp[idx] = acc;
        }
        __syncthreads();
        int rf[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) rf[d] = (reflect101(y + d - 2, h) - ry0) * kRowF + 12 * tg;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < 5; ++d) acc = acc + t[d] * S.hp[rf[d] + k];
            o[k] = round255(acc);
        }
    } else if (op == MNY_SEQ_MEDIAN) {
        const bool five = q.median_k == 5;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p0 = (2 * j) / 3, c0 = (2 * j) % 3, p1 = (2 * j + 1) / 3, c1 = (2 * j + 1) % 3;
            us2 m;
            if (five) {
                m = median_select<25>([&](int i) {
                    const int dy = i / 5, dx = i % 5;
                    us2 v; v.x = sb[rowb[dy] + colo[p0][dx] + c0]; v.y = sb[rowb[dy] + colo[p1][dx] + c1];
                    return v;
                });
            } else {
                m = median_select<9>([&](int i) {
                    const int dy = 1 + i / 3, dx = 1 + i % 3;
                    us2 v; v.x = sb[rowb[dy] + colo[p0][dx] + c0]; v.y = sb[rowb[dy] + colo[p1][dx] + c1];
                    return v;
                });
            }
            o[2 * j] = m.x; o[2 * j + 1] = m.y;
        }
    } else if (op == MNY_SEQ_SHARPEN) {
        const float c = q.sharpen_c, s = q.sharpen_s;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int p = k / 3, ch = k % 3;
            int sum = 0;
#pragma unroll
            for (int dy = 1; dy <= 3; ++dy)
#pragma unroll
                for (int dx = 1; dx <= 3; ++dx) sum += sb[rowb[dy] + colo[p][dx] + ch];
            const int ctr = sb[rowb[2] + colo[p][2] + ch];
            o[k] = round255(c * (float)ctr + s * (float)(sum - ctr));
        }
    } else if (op == MNY_SEQ_NOISE) {
        const float scale = q.noise_scale;
        const bool per = q.noise_per_channel != 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int x = min(tx0 + 4 * tg + p, w - 1);
            uint32_t r[4];
            philox((uint32_t)y * (uint32_t)w + (uint32_t)x, q.noise_key[0], q.noise_key[1], r);
            const float u0 = unit(r[0]), u1 = unit(r[1]);
            float sn, cs;
            sincosf(6.283185307179586f * u1, &sn, &cs);
            const float R0 = sqrtf(-2.f * logf(u0));
            float z[3];
            z[0] = R0 * cs;
            if (per) {
                float sn2, cs2;
                sincosf(6.283185307179586f * unit(r[3]), &sn2, &cs2);
                z[1] = R0 * sn;
                z[2] = sqrtf(-2.f * logf(unit(r[2]))) * cs2;
            } else {
                z[1] = z[0]; z[2] = z[0];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * p + ch] = clamp255((int)sb[rowb[2] + colo[p][2] + ch] + (int)rintf(scale * z[ch]));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = 0;                                  // not reached: classify() admits the four kinds only
    }
    // ---- the tile's rows at their global byte phase, then whole dwords where the row segment allows
    uint8_t* ob = (uint8_t*)S.out;
    {
        const int base = ty * kOutStrideB + S.out_ph[ty] + 12 * tg;
#pragma unroll
        for (int k = 0; k < 12; ++k) ob[base + k] = (uint8_t)o[k];
    }
    __syncthreads();
    const int nb = 3 * min(kTW, w - tx0);
    for (int idx = tid; idx < kTH * kOutRowDw; idx += 256) {
        const int r = idx / kOutRowDw, d = idx - r * kOutRowDw;
        if (ty0 + r >= h) break;
        const int ph = S.out_ph[r];
        const int lo = ph, hi = ph + nb;
        if (4 * d + 4 <= lo || 4 * d >= hi) continue;
        const int64_t a = ((int64_t)(ty0 + r) * 3 * w + 3 * tx0 - ph) + 4 * d;
        if (4 * d >= lo && 4 * d + 4 <= hi) {
            *(uint32_t*)(out + a) = S.out[r * kOutRowDw + d];
        } else {
            for (int b = 0; b < 4; ++b)
                if (4 * d + b >= lo && 4 * d + b < hi) out[a + b] = ob[r * kOutStrideB + 4 * d + b];
        }
    }
    __syncthreads();
}

// a malformed record: its 3*h*w bytes become zeros (byte stores, the offset may be odd)
__device__ void zero_tile(uint8_t* __restrict__ out, int h, int w, int ty0, int tx0) {
    const int y = ty0 + (threadIdx.x >> 4), x = tx0 + 4 * (threadIdx.x & 15);
    if (y >= h) return;
    const int n = 3 * min(4, w - x);
    uint8_t* p = out + ((int64_t)y * w + x) * 3;
    for (int k = 0; k < n; ++k) p[k] = 0;
}

// an image without an op: job `part` of `parts` copies its share of the image's dwords, the last one also the 1..3 bytes after them
__device__ void copy_part(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t nbytes, int part, int parts) {
    const int64_t ndw = nbytes >> 2;
    const int64_t per = (ndw + parts - 1) / parts;
    const int64_t b = part * per, e = min(b + per, ndw);
    for (int64_t i = b + threadIdx.x; i < e; i += 256) ((uint32_t*)out)[i] = ((const uint32_t*)in)[i];
    if (part == parts - 1) {
        const int64_t tail = ndw * 4 + threadIdx.x;
        if (tail < nbytes) out[tail] = in[tail];
    }
}

// grid: capped; stage 0 or 1 (see the head of the file)
__global__ __launch_bounds__(256) void aug_seq_kernel(const uint8_t* __restrict__ src, const mny_image_desc* __restrict__ desc,
                                                      const mny_aug_seq_item* __restrict__ seq, int n_items, int max_h, int max_w, uint8_t* __restrict__ dst,
                                                      uint8_t* __restrict__ ws, int stage) {
    __shared__ seq_lds S;
    const int tid = threadIdx.x;
    // ---- the job list: exclusive prefix sum of the per-image tile counts
    const int per = (n_items + 255) / 256;
    const int i0 = min(tid * per, n_items), i1 = min(i0 + per, n_items);
    uint32_t local = 0;
    for (int i = i0; i < i1; ++i) {
        const mny_image_desc d = desc[i];
        uint32_t c = addressable(d) ? (uint32_t)tiles_of(d) : 0u;
        if (stage == 1 && (seq[i].n_ops != 2 || (d.offset & 3) || d.h > max_h || d.w > max_w)) c = 0;
        S.pref[i] = c;
        local += c;
    }
    S.part[tid] = local;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                                          // inclusive scan of the 256 partial sums
        const uint32_t add = tid >= s ? S.part[tid - s] : 0u;
        __syncthreads();
        S.part[tid] += add;
        __syncthreads();
    }
    uint32_t run = S.part[tid] - local;
    for (int i = i0; i < i1; ++i) {
        const uint32_t c = S.pref[i];
        S.pref[i] = run;
        run += c;
    }
    const uint32_t total = S.part[255];
    if (tid == 0) S.pref[n_items] = total;
    __syncthreads();
    // ---- status word: the lowest malformed index, by block 0 of stage 0 alone
    if (stage == 0 && blockIdx.x == 0) {
        uint32_t bad = 0xffffffffu;
        for (int i = i1 - 1; i >= i0; --i)
            if (classify(desc[i], seq[i], max_h, max_w) != kOk) bad = (uint32_t)i;
        S.part[tid] = bad;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) S.part[tid] = min(S.part[tid], S.part[tid + s]);
            __syncthreads();
        }
        if (tid == 0) *(int*)ws = S.part[0] == 0xffffffffu ? 0 : (int)S.part[0] + 1;
        __syncthreads();
    }
    for (uint32_t job = blockIdx.x; job < total; job += gridDim.x) {
        int lo = 0, hi = n_items;                                                // the last image with pref <= job
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (S.pref[mid] <= job) lo = mid; else hi = mid;
        }
        const int img = lo;
        const mny_image_desc d = desc[img];
        const mny_aug_seq_item& q = seq[img];
        const int t = (int)(job - S.pref[img]);
        const int tcols = (d.w + kTW - 1) / kTW;
        const int ty0 = (t / tcols) * kTH, tx0 = (t - (t / tcols) * tcols) * kTW;
        const int cls = classify(d, q, max_h, max_w);
        if (cls == kZero) {
            if (stage == 0) zero_tile(dst + d.offset, d.h, d.w, ty0, tx0);
            continue;
        }
        if (cls != kOk) continue;
        uint8_t* mid_img = ws + kWsHead + d.offset;
        if (stage == 0 && q.n_ops == 0)
            copy_part(src + d.offset, dst + d.offset, (int64_t)3 * d.h * d.w, t, tiles_of(d));
        else if (stage == 0)
            run_tile(S, src + d.offset, q.n_ops == 2 ? mid_img : dst + d.offset, q, q.op[0], d.h, d.w, ty0, tx0);
        else
            run_tile(S, mid_img, dst + d.offset, q, q.op[1], d.h, d.w, ty0, tx0);
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_aug_seq_ws_bytes(int n_items, int64_t src_bytes, int max_in_h, int max_in_w) {
    if (n_items < 1 || n_items > kMaxItems || src_bytes < 1 || max_in_h < 1 || max_in_w < 1 || max_in_h > kMaxSide || max_in_w > kMaxSide) return 0;
    return kWsHead + (((size_t)src_bytes + 255) & ~(size_t)255);
}

extern "C" int mny_aug_seq_batch(const uint8_t* src, const mny_image_desc* desc, const mny_aug_seq_item* seq, int n_items, int max_in_h, int max_in_w,
                                 uint8_t* dst, void* ws, void* stream) {
    MNY_REQUIRE(src && desc && seq && dst && ws, "mny_aug_seq_batch: null pointer");
    MNY_REQUIRE(src != dst, "mny_aug_seq_batch: dst must not be src");
    MNY_REQUIRE((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)ws) & 3) == 0, "mny_aug_seq_batch: src, dst and ws must be 4-byte aligned");
    MNY_REQUIRE(n_items >= 1 && n_items <= kMaxItems && max_in_h >= 1 && max_in_w >= 1 && max_in_h <= kMaxSide && max_in_w <= kMaxSide,
                "mny_aug_seq_batch: bad sizes items=%d (1..%d) max %dx%d (sides up to %d)", n_items, kMaxItems, max_in_h, max_in_w, kMaxSide);
    hipStream_t st = (hipStream_t)stream;
    const int64_t bound = (int64_t)n_items * cdiv(max_in_h, kTH) * cdiv(max_in_w, kTW);
    const unsigned grid = (unsigned)(bound < 2048 ? bound : 2048);
    aug_seq_kernel<<<grid, 256, 0, st>>>(src, desc, seq, n_items, max_in_h, max_in_w, dst, (uint8_t*)ws, 0);
    aug_seq_kernel<<<grid, 256, 0, st>>>(src, desc, seq, n_items, max_in_h, max_in_w, dst, (uint8_t*)ws, 1);
    return check_launch("mny_aug_seq_batch");
}
