// Segmentation evaluation on the device (include/mnyolo.h: mny_seg_confusion, mny_seg_upsample, mny_seg_metrics).
// The seg head's logits [N,h,w,C] are turned into probabilities, resized to each label's size with half-pixel bilinear weights (the
// rule of inference.py:64-67: cv2.resize INTER_LINEAR per class map, then > 0.5), made a single-label id map by the arg-max, and
// counted against the uint8 ground-truth id maps into an int64 confusion matrix.  The arithmetic is specified in the header; this
// file is compiled with -ffp-contract=off so that every product and sum below is an fp32 operation of its own.
//
// Geometry (DESIGN.md "Segmentation evaluator"): a 256-thread workgroup owns kSeTileRows output rows of one image and first stages
// the few head rows they touch in LDS as probabilities, so the sigmoid runs once per head element.  A lane owns 16 consecutive
// columns over a band of the tile's rows: the column weights and neighbour offsets (one correctly rounded division each) are formed
// once and reused by every row of the band, and each row costs the lane one 16-byte label load (aligned whenever the width is a
// multiple of 16; rows are not padded, so other widths load unaligned) and, with pred_out, one 16-byte store.  The last group of a
// row whose width is no multiple of 16 is read and written byte by byte: nothing is touched past a row's end.
#include "common.h"

namespace mny {
namespace {

constexpr int kSeThreads = 256;
constexpr int kSeWaves = kSeThreads / kWave;
constexpr int kSeBatch = 96;            // images per launch: their descriptors ride in the kernel arguments
constexpr int kSeTileRows = 32;
constexpr int kSeMaxSide = 16384;       // (2 * 16383 + 1) * 16384 < 2^31 and 2 * 16384 is exact in fp32
constexpr int kSeMaxC = 16;
constexpr int kSeMaxCells = (kSeMaxC + 1) * (kSeMaxC + 1);
constexpr int kSeLdsFloats = 12288;     // 48 KB of staged probabilities
constexpr int kSeRegC = 3;              // (C + 1)^2 <= 16: counters in registers

struct SegImages {
    int64_t off[kSeBatch];              // from the start of labels / pred_out (bytes) or out (floats)
    int32_t H[kSeBatch], W[kSeBatch];
    int32_t tile0[kSeBatch + 1];        // first workgroup of image i; tile0[n] = the grid
    int32_t n, first;                   // images of this launch, index of its image 0 in the head
};

__host__ __device__ inline int se_floordiv(int a, int b) {      // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline int se_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// upper bound on the head rows `tr` consecutive output rows touch: floor(a + d) - floor(a) <= ceil(d), plus the second neighbour
__host__ __device__ inline int se_stage_rows(int tr, int h, int H) {
    const int64_t r = cdiv((int64_t)(tr - 1) * h, H) + 2;
    return r < h ? (int)r : h;
}
__host__ __device__ inline int se_tile_rows(int h, int w, int C, int H) {
    int tr = kSeTileRows;
    while (tr > 1 && (int64_t)se_stage_rows(tr, h, H) * w * C > kSeLdsFloats) tr >>= 1;
    return tr;
}

// source position of output index i on an axis of `src` head cells and `dst` output pixels: n = (2i+1) src - dst,
// i0 = floor(n / 2dst) (not clamped), r = n - i0 * 2dst in [0, 2dst)
struct Axis { int i0, r; };
__device__ __forceinline__ Axis axis_at(int i, int src, int dst) {
    const int n = (2 * i + 1) * src - dst;
    Axis a;
    a.i0 = se_floordiv(n, 2 * dst);
    a.r = n - a.i0 * 2 * dst;
    return a;
}
__device__ __forceinline__ void axis_step(Axis& a, int src, int dst) {      // i -> i + 1
    a.r += 2 * src;
    if (a.r >= 2 * dst) {
        if (src <= dst) { a.r -= 2 * dst; ++a.i0; }
        else { a.i0 += a.r / (2 * dst); a.r %= 2 * dst; }
    }
}

struct Tile { int img, H, W, Y0, Y1, ylo; };

// which (image, row tile) this workgroup owns, and its head rows as probabilities in P; false: nothing to do (uniform)
__device__ __forceinline__ bool tile_stage(const float* __restrict__ head, int h, int w, int C, const SegImages& im, float* P, Tile& t) {
    int lo = 0, hi = im.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (im.tile0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    t.img = lo;
    t.H = im.H[lo];
    t.W = im.W[lo];
    const int tr = se_tile_rows(h, w, C, t.H);
    t.Y0 = ((int)blockIdx.x - im.tile0[lo]) * tr;
    if (t.Y0 >= t.H) return false;
    t.Y1 = t.Y0 + tr < t.H ? t.Y0 + tr : t.H;
    t.ylo = se_clamp(axis_at(t.Y0, h, t.H).i0, h - 1);
    const int yhi = se_clamp(axis_at(t.Y1 - 1, h, t.H).i0 + 1, h - 1);
    const int count = (yhi - t.ylo + 1) * w * C;
    if (count > kSeLdsFloats) return false;                    // se_tile_rows rules it out
    const float* src = head + ((size_t)(im.first + lo) * h + t.ylo) * w * C;
    for (int i = threadIdx.x; i < count; i += kSeThreads) P[i] = sigmoid_ref(src[i]);
    return true;
}

struct Row { int r0, r1; float ty, uy; };
__device__ __forceinline__ Row row_of(const Axis& ay, int h, int H, int ylo, int wC) {
    Row r;
    r.r0 = (se_clamp(ay.i0, h - 1) - ylo) * wC;
    r.r1 = (se_clamp(ay.i0 + 1, h - 1) - ylo) * wC;
    r.ty = (float)ay.r / (float)(2 * H);
    r.uy = 1.0f - r.ty;
    return r;
}
struct Col { int x0, x1; float tx, ux; };
__device__ __forceinline__ Col col_of(const Axis& ax, int w, int W, int C) {
    Col c;
    c.x0 = se_clamp(ax.i0, w - 1) * C;
    c.x1 = se_clamp(ax.i0 + 1, w - 1) * C;
    c.tx = (float)ax.r / (float)(2 * W);
    c.ux = 1.0f - c.tx;
    return c;
}
__device__ __forceinline__ float interp(const float* P, const Row& r, const Col& c, int ch) {
    const float a = P[r.r0 + c.x0 + ch] * c.ux + P[r.r0 + c.x1 + ch] * c.tx;
    const float b = P[r.r1 + c.x0 + ch] * c.ux + P[r.r1 + c.x1 + ch] * c.tx;
    return a * r.uy + b * r.ty;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// CT = 1..kSeRegC: C == CT, the (C+1)^2 counters live in registers; CT = 0: any C, a histogram per wave in LDS
template <int CT>
__global__ __launch_bounds__(kSeThreads) void seg_confusion_kernel(const float* __restrict__ head, int h, int w, int Crt, const SegImages im,
                                                                   const uint8_t* __restrict__ labels, uint8_t* __restrict__ pred_out,
                                                                   unsigned long long* __restrict__ conf, unsigned long long* __restrict__ ignored) {
    extern __shared__ __align__(16) float P[];
    __shared__ uint32_t hist[kSeWaves][kSeMaxCells + 1];
    __shared__ uint32_t ign_s[kSeWaves];
    const int C = CT ? CT : Crt, K = C + 1, cells = K * K;
    constexpr int NREG = CT ? (CT + 1) * (CT + 1) : 1;
    const int tid = threadIdx.x, wave = tid >> 6;
    Tile t;
    if (!tile_stage(head, h, w, C, im, P, t)) return;
    if (!CT)
        for (int k = tid; k < kSeWaves * (kSeMaxCells + 1); k += kSeThreads) (&hist[0][0])[k] = 0;
    __syncthreads();

    const int H = t.H, W = t.W, wC = w * C;
    const uint8_t* lab = labels ? labels + im.off[t.img] : nullptr;
    uint8_t* po = pred_out ? pred_out + im.off[t.img] : nullptr;
    uint32_t cnt[NREG];
#pragma unroll
    for (int k = 0; k < NREG; ++k) cnt[k] = 0;
    uint32_t nign = 0;

    // work item = (group of 16 columns, band of rows): the column terms are formed once per item and reused by every row of the band
    const int G = (W + 15) >> 4, rows = t.Y1 - t.Y0;
    int bands = kSeThreads / G;
    bands = bands < 1 ? 1 : (bands > rows ? rows : bands);
    const int per = (rows + bands - 1) / bands;
    for (int item = tid; item < G * bands; item += kSeThreads) {
        const int g = item % G, band = item / G;
        const int X0 = g << 4, nvalid = W - X0 < 16 ? W - X0 : 16;
        const int Ya = t.Y0 + band * per, Yb = Ya + per < t.Y1 ? Ya + per : t.Y1;
        uint32_t xo[16];                                        // x0 * C | x1 * C << 16 (w * C <= 6144)
        float tx[16];
        {
            Axis ax = axis_at(X0, w, W);
#pragma unroll
            for (int j = 0; j < 16; ++j) {                      // columns past the row's end repeat the last one; they are never counted or stored
                const Col c = col_of(ax, w, W, C);
                xo[j] = (uint32_t)c.x0 | ((uint32_t)c.x1 << 16);
                tx[j] = c.tx;
                if (j + 1 < nvalid) axis_step(ax, w, W);
            }
        }
        Axis ay = axis_at(Ya, h, H);
        for (int Y = Ya; Y < Yb; ++Y) {
            const Row row = row_of(ay, h, H, t.ylo, wC);
            axis_step(ay, h, H);
            const int f = Y * W + X0;
            uint32_t lw[4] = {~0u, ~0u, ~0u, ~0u};              // a byte that is not there reads as 255 = ignored, and is taken off again below
            if (lab) {
                if (nvalid == 16) {
                    __builtin_memcpy(lw, lab + f, 16);          // 16-byte aligned whenever W is a multiple of 16
                } else {
#pragma unroll
                    for (int j = 0; j < 15; ++j)
                        if (j < nvalid) lw[j >> 2] ^= (uint32_t)(lab[f + j] ^ 255u) << ((j & 3) * 8);
                }
            }
            uint32_t pw[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int o0 = xo[j] & 0xffffu, o1 = xo[j] >> 16;
                const float t1 = tx[j], u1 = 1.0f - t1;
                float m = 0.5f;
                uint32_t pred = 0;
                if constexpr (CT == 2) {
                    // both channels of a head cell in one 8-byte LDS read (every offset is even): ds_read_b64 moves the same bytes in a
                    // quarter of the LDS cycles of the ds_read2_b32 the compiler picks for two floats of unknown alignment
                    const float2* P2 = reinterpret_cast<const float2*>(P);        // indexed in cells, so that the alignment is visible
                    const float2 p00 = P2[(row.r0 + o0) >> 1], p01 = P2[(row.r0 + o1) >> 1];
                    const float2 p10 = P2[(row.r1 + o0) >> 1], p11 = P2[(row.r1 + o1) >> 1];
                    const float v0 = (p00.x * u1 + p01.x * t1) * row.uy + (p10.x * u1 + p11.x * t1) * row.ty;
                    const float v1 = (p00.y * u1 + p01.y * t1) * row.uy + (p10.y * u1 + p11.y * t1) * row.ty;
                    if (v0 > m) { m = v0; pred = 1; }
                    if (v1 > m) { m = v1; pred = 2; }
                } else {
                    for (int c = 0; c < C; ++c) {
                        const float a = P[row.r0 + o0 + c] * u1 + P[row.r0 + o1 + c] * t1;
                        const float b = P[row.r1 + o0 + c] * u1 + P[row.r1 + o1 + c] * t1;
                        const float v = a * row.uy + b * row.ty;
                        if (v > m) { m = v; pred = c + 1; }      // strict: the lowest channel keeps a tie; a NaN never wins
                    }
                }
                pw[j >> 2] |= pred << ((j & 3) * 8);
                // no branch in the pixel body: the 16 pixels stay one block of code, so their LDS reads can be issued together
                const uint32_t gt = (lw[j >> 2] >> ((j & 3) * 8)) & 255u;
                const bool ign = gt > (uint32_t)C;
                nign += ign;
                const uint32_t cell = ign ? (uint32_t)kSeMaxCells : gt * K + pred;
                if (CT) {
#pragma unroll
                    for (int k = 0; k < NREG; ++k) cnt[k] += (cell == (uint32_t)k);
                } else {
                    atomicAdd(&hist[wave][cell], 1u);           // slot kSeMaxCells collects the ignored pixels and is never read
                }
            }
            nign -= 16 - nvalid;
            if (po) {
                if (nvalid == 16) {
                    __builtin_memcpy(po + f, pw, 16);
                } else {
#pragma unroll
                    for (int j = 0; j < 15; ++j)
                        if (j < nvalid) po[f + j] = (uint8_t)(pw[j >> 2] >> ((j & 3) * 8));
                }
            }
        }
    }
    if (!lab) return;

    if (CT) {
#pragma unroll
        for (int k = 0; k < NREG; ++k) {
            const uint32_t s = wave_sum(cnt[k]);
            if ((tid & 63) == 0) hist[wave][k] = s;
        }
    }
    nign = wave_sum(nign);
    if ((tid & 63) == 0) ign_s[wave] = nign;
    __syncthreads();
    for (int k = tid; k < cells; k += kSeThreads) {
        unsigned long long s = 0;
        for (int wv = 0; wv < kSeWaves; ++wv) s += hist[wv][k];
        if (s) atomicAdd(conf + k, s);
    }
    if (tid == kSeThreads - 1) {
        unsigned long long s = 0;
        for (int wv = 0; wv < kSeWaves; ++wv) s += ign_s[wv];
        if (s) atomicAdd(ignored, s);
    }
}

__global__ __launch_bounds__(kSeThreads) void seg_upsample_kernel(const float* __restrict__ head, int h, int w, int C, const SegImages im,
                                                                  float* __restrict__ out) {
    extern __shared__ __align__(16) float P[];
    Tile t;
    if (!tile_stage(head, h, w, C, im, P, t)) return;
    __syncthreads();
    const int H = t.H, W = t.W, total = H * W;
    float* o = out + im.off[t.img];
    for (int f = t.Y0 * W + threadIdx.x; f < t.Y1 * W; f += kSeThreads) {
        const int Y = f / W, X = f - Y * W;
        const Row row = row_of(axis_at(Y, h, H), h, H, t.ylo, w * C);
        const Col col = col_of(axis_at(X, w, W), w, W, C);
        for (int c = 0; c < C; ++c) o[(size_t)c * total + f] = interp(P, row, col, c);
    }
}

// out: iou[0..C], miou, miou_fg, pixel_acc.  Counts below 2^53 are exact in fp64; every ratio is one division.
__global__ void seg_metrics_kernel(const long long* __restrict__ conf, int C, double* __restrict__ out) {
    __shared__ double iou[kSeMaxC + 1];
    __shared__ long long diag[kSeMaxC + 1], rowsum[kSeMaxC + 1];
    const int K = C + 1, k = threadIdx.x;
    if (k < K) {
        long long r = 0, c = 0;
        for (int j = 0; j < K; ++j) { r += conf[k * K + j]; c += conf[j * K + k]; }
        diag[k] = conf[k * K + k];
        rowsum[k] = r;
        iou[k] = (double)diag[k] / (double)(r + c - diag[k]);   // 0 / 0 = NaN: the class is in neither map
        out[k] = iou[k];
    }
    __syncthreads();
    if (k == 0) {
        double s = 0, sf = 0;
        int n = 0, nf = 0;
        long long tr = 0, all = 0;
        for (int j = 0; j < K; ++j) {
            if (iou[j] == iou[j]) { s += iou[j]; ++n; if (j) { sf += iou[j]; ++nf; } }
            tr += diag[j];
            all += rowsum[j];
        }
        out[K] = s / (double)n;
        out[K + 1] = sf / (double)nf;
        out[K + 2] = (double)tr / (double)all;
    }
}

// checks shared by the two resampling entries; `align`: what an offset must be a multiple of
int se_check(const char* who, const float* head, int N, int h, int w, int C, const int64_t* offsets, const int32_t* sizes, int align) {
    MNY_REQUIRE(head && offsets && sizes, "%s: null pointer", who);
    MNY_REQUIRE(C >= 1 && C <= kSeMaxC, "%s: %d seg classes outside 1..%d", who, C, kSeMaxC);
    MNY_REQUIRE(N >= 1 && h >= 1 && w >= 1 && h <= kSeMaxSide && w <= kSeMaxSide, "%s: bad head shape [%d,%d,%d,%d]", who, N, h, w, C);
    MNY_REQUIRE((int64_t)w * C * 2 <= kSeLdsFloats, "%s: head row of %d x %d floats: two of them exceed the %d floats of the LDS stage", who, w, C, kSeLdsFloats);
    for (int i = 0; i < N; ++i) {
        const int H = sizes[2 * i], W = sizes[2 * i + 1];
        MNY_REQUIRE(H >= 1 && W >= 1 && H <= kSeMaxSide && W <= kSeMaxSide, "%s: image %d has size %d x %d (1..%d per side)", who, i, H, W, kSeMaxSide);
        MNY_REQUIRE(offsets[i] >= 0 && offsets[i] % align == 0, "%s: offset %lld of image %d is not a non-negative multiple of %d", who,
                    (long long)offsets[i], i, align);
    }
    return MNY_OK;
}

// descriptors of images [first, first + n) and the dynamic LDS their tiles need
size_t se_fill(SegImages& im, int first, int n, int h, int w, int C, const int64_t* offsets, const int32_t* sizes) {
    int64_t floats = 0;
    im.n = n;
    im.first = first;
    im.tile0[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int H = sizes[2 * (first + i)], W = sizes[2 * (first + i) + 1];
        im.off[i] = offsets[first + i];
        im.H[i] = H;
        im.W[i] = W;
        const int tr = se_tile_rows(h, w, C, H);
        im.tile0[i + 1] = im.tile0[i] + (int)cdiv(H, tr);
        const int64_t f = (int64_t)se_stage_rows(tr, h, H) * w * C;
        if (f > floats) floats = f;
    }
    return (size_t)floats * sizeof(float);
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" int mny_seg_confusion(const float* head, int N, int h, int w, int C, const uint8_t* labels, const int64_t* label_offsets,
                                 const int32_t* label_sizes, int64_t* conf, int64_t* ignored, uint8_t* pred_out, void* stream) {
    if (const int rc = se_check("mny_seg_confusion", head, N, h, w, C, label_offsets, label_sizes, 16)) return rc;
    MNY_REQUIRE(labels || pred_out, "mny_seg_confusion: null pointer (labels and pred_out are both missing)");
    MNY_REQUIRE(!labels || (conf && ignored), "mny_seg_confusion: null pointer (labels without conf / ignored)");
    MNY_REQUIRE((((uintptr_t)labels | (uintptr_t)pred_out) & 15) == 0 && (((uintptr_t)conf | (uintptr_t)ignored) & 7) == 0,
                "mny_seg_confusion: labels and pred_out must be 16-byte aligned, conf and ignored 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    SegImages im;
    for (int first = 0; first < N; first += kSeBatch) {
        const int n = N - first < kSeBatch ? N - first : kSeBatch;
        const size_t lds = se_fill(im, first, n, h, w, C, label_offsets, label_sizes);
        auto* cf = (unsigned long long*)conf;
        auto* ig = (unsigned long long*)ignored;
        const dim3 grid(im.tile0[n]), block(kSeThreads);
        switch (C <= kSeRegC ? C : 0) {
            case 1: seg_confusion_kernel<1><<<grid, block, lds, st>>>(head, h, w, C, im, labels, pred_out, cf, ig); break;
            case 2: seg_confusion_kernel<2><<<grid, block, lds, st>>>(head, h, w, C, im, labels, pred_out, cf, ig); break;
            case 3: seg_confusion_kernel<3><<<grid, block, lds, st>>>(head, h, w, C, im, labels, pred_out, cf, ig); break;
            default: seg_confusion_kernel<0><<<grid, block, lds, st>>>(head, h, w, C, im, labels, pred_out, cf, ig); break;
        }
    }
    return check_launch("mny_seg_confusion");
}

extern "C" int mny_seg_upsample(const float* head, int N, int h, int w, int C, const int32_t* sizes, const int64_t* out_offsets, float* out,
                                void* stream) {
    if (const int rc = se_check("mny_seg_upsample", head, N, h, w, C, out_offsets, sizes, 4)) return rc;
    MNY_REQUIRE(out && ((uintptr_t)out & 15) == 0, "mny_seg_upsample: null pointer or out not 16-byte aligned");
    SegImages im;
    for (int first = 0; first < N; first += kSeBatch) {
        const int n = N - first < kSeBatch ? N - first : kSeBatch;
        const size_t lds = se_fill(im, first, n, h, w, C, out_offsets, sizes);
        seg_upsample_kernel<<<dim3(im.tile0[n]), dim3(kSeThreads), lds, (hipStream_t)stream>>>(head, h, w, C, im, out);
    }
    return check_launch("mny_seg_upsample");
}

extern "C" int mny_seg_metrics(const int64_t* conf, int C, double* out, void* stream) {
    MNY_REQUIRE(conf && out, "mny_seg_metrics: null pointer");
    MNY_REQUIRE(C >= 1 && C <= kSeMaxC, "mny_seg_metrics: %d seg classes outside 1..%d", C, kSeMaxC);
    seg_metrics_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const long long*)conf, C, out);
    return check_launch("mny_seg_metrics");
}
