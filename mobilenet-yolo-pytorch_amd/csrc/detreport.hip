// Validation report on the device (include/mnyolo.h: mny_det_curves, mny_det_confusion), restated in tests/report_ref.py.
//   curves   : key (class | descending score) of every counted detection, value = stored index << 1 | TP; detections that do not
//              count (label out of range, not evaluated, ignored, NaN score) get the no-class key and sort behind every class.  Pair
//              sort of pairsort.h, then a three-kernel integer scan of the TP bits over the whole sorted run (block counts, scan of
//              the block counts, positions), so a class segment of any length costs nothing extra.  One thread per (class, grid
//              point) finds by binary search how many scores of the class's segment are >= c_j; tp is a difference of two scan
//              entries, fp the rest of the segment.  Precision, recall and F1 follow there; a thread per grid point sums F1 over the
//              classes in ascending order, and one workgroup smooths (window in LDS), takes the first maximum and fills at_best.
//   confusion: a workgroup per image.  Rounds of a workgroup-wide arg-max over the free candidate pairs, key (IoU, smaller pair index
//              = smaller detection, then smaller ground truth); the loop runs min(detections, ground truths) times at most and ends
//              early when a round finds nothing.  IoUs (fp64) sit in an LDS table when detections x ground truths fit, a taken
//              pair's row and column are struck out of it; beyond the table every round recomputes the IoUs of the free pairs and
//              reads the matched words (det_gt, or the workspace) instead.  Counts go into the matrix with integer atomics.
// No host synchronisation, no floating-point atomics, the same bits run to run.
// Compiled with -ffp-contract=off: every fp64 value must round like the separate operations of the specification.
#include "boxgeo.h"
#include "common.h"
#include "pairsort.h"

namespace mny {
namespace {

constexpr uint32_t kNoClass = 255;
constexpr int kMaxGrid = 4096;
constexpr int kScanBlock = 1024;      // sorted detections per scan workgroup
constexpr int kConfThreads = 256;
constexpr int kConfTab = 4096;        // 32 KB IoU table: detections x ground truths of one image

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- curves: order -------------------------------------------------------------------------------------------------------------
__global__ void rep_key_kernel(const float* __restrict__ det_labels, const float* __restrict__ det_scores, const int32_t* __restrict__ det_match,
                               const uint8_t* __restrict__ det_ignore, int D, int n_classes, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const uint32_t c = class_of(det_labels[d], n_classes);
    const float s = det_scores[d];
    const int32_t m = det_match[d];
    const bool counted = c && m != -2 && det_ignore[d] == 0 && s == s;
    const uint32_t sb = s == 0.f ? 0u : __float_as_uint(s);
    const uint32_t asc = sb ^ ((sb >> 31) ? 0xFFFFFFFFu : 0x80000000u);          // order-preserving map of a float
    keys[d] = ((uint64_t)(counted ? c : kNoClass) << 32) | (uint32_t)~asc;
    vals[d] = ((uint32_t)d << 1) | (m >= 0 ? 1u : 0u);
}

__device__ __forceinline__ float score_of_key(uint64_t key) {
    const uint32_t asc = ~(uint32_t)key;
    return __uint_as_float((asc >> 31) ? asc ^ 0x80000000u : ~asc);
}

// ---- curves: inclusive scan of the TP bits over the sorted run -------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void rep_scan_count_kernel(const uint32_t* __restrict__ vals, int D, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_w[kScanBlock / kWave];
    const int tid = threadIdx.x, i = blockIdx.x * kScanBlock + tid;
    const unsigned long long m = __ballot(i < D && (vals[i < D ? i : 0] & 1u));
    if ((tid & 63) == 0) s_w[tid >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kScanBlock / kWave; ++w) t += s_w[w];
        bsum[blockIdx.x] = t;
    }
}

// bsum[0..nb) -> its exclusive scan, in place; one workgroup
__global__ __launch_bounds__(kScanBlock) void rep_scan_sums_kernel(uint32_t* __restrict__ bsum, int nb) {
    constexpr int NW = kScanBlock / kWave;
    __shared__ uint32_t s_w[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < nb; base += kScanBlock) {
        const int i = base + tid;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        __syncthreads();                                                          // the previous chunk's readers are done
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < NW; ++w) {
            const uint32_t s = s_w[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < nb) bsum[i] = carry + before + inc - v;
        carry += total;
    }
}

// cum[p] = TPs among the sorted positions 0..p
__global__ __launch_bounds__(kScanBlock) void rep_scan_apply_kernel(const uint32_t* __restrict__ vals, int D, const uint32_t* __restrict__ bsum,
                                                                    uint32_t* __restrict__ cum) {
    constexpr int NW = kScanBlock / kWave;
    __shared__ uint32_t s_w[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x * kScanBlock + tid;
    const unsigned long long m = __ballot(i < D && (vals[i < D ? i : 0] & 1u));
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = bsum[blockIdx.x];
    for (int w = 0; w < wave; ++w) before += s_w[w];
    if (i < D) cum[i] = before + (uint32_t)__popcll(m & (~0ull >> (63 - lane)));
}

// seg[k] = first sorted position of class k+1, k = 0..K (seg[K] = end of the last class)
__global__ void rep_bounds_kernel(const uint64_t* __restrict__ keys, int D, int K, int32_t* __restrict__ seg) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= K) seg[k] = lower_bound_key(keys, D, (uint64_t)(k + 1) << 32);
}

__global__ void rep_npos_kernel(const float* __restrict__ true_labels, const float* __restrict__ true_crowd, int T, int n_classes,
                                unsigned long long* __restrict__ npos) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint32_t c = class_of(true_labels[t], n_classes);
    if (c && true_crowd[t] == 0.f) atomicAdd(&npos[c - 1], 1ull);
}

// ---- curves: counts and derived values, a thread per (class blockIdx.y, grid point) -----------------------------------------------
__global__ void rep_count_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cum, const int32_t* __restrict__ seg,
                                 const int64_t* __restrict__ npos, int G, int64_t* __restrict__ tp, int64_t* __restrict__ fp,
                                 double* __restrict__ precision, double* __restrict__ recall, double* __restrict__ f1) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= G) return;
    const int lo = seg[k], hi = seg[k + 1];
    const double cj = (double)j / (double)(G - 1);
    int l = lo, h = hi;                                                           // first position of the segment with score < c_j
    while (l < h) {
        const int mid = (l + h) >> 1;
        if ((double)score_of_key(keys[mid]) >= cj) l = mid + 1; else h = mid;
    }
    const int64_t n = l - lo;
    const int64_t tpv = n ? (int64_t)(cum[l - 1] - (lo ? cum[lo - 1] : 0u)) : 0;
    const int64_t fpv = n - tpv, np = npos[k];
    double P = -1.0, R = -1.0, F = -1.0;
    if (np != 0) {
        P = n ? (double)tpv / (double)n : 1.0;
        R = (double)tpv / (double)np;
        F = ((2.0 * P) * R) / ((P + R) + 1e-16);
    }
    const size_t o = (size_t)k * G + j;
    tp[o] = tpv; fp[o] = fpv;
    precision[o] = P; recall[o] = R; f1[o] = F;
}

__global__ void rep_mean_kernel(const double* __restrict__ f1, const int64_t* __restrict__ npos, int K, int G, double* __restrict__ mean_f1) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    double sum = 0.0;
    int cnt = 0;
    for (int k = 0; k < K; ++k)
        if (npos[k] != 0) { sum += f1[(size_t)k * G + j]; ++cnt; }
    mean_f1[j] = cnt ? sum / (double)cnt : -1.0;
}

// one workgroup: smoothing, first maximum, at_best
__global__ __launch_bounds__(1024) void rep_best_kernel(const double* __restrict__ mean_f1, const double* __restrict__ precision,
                                                        const double* __restrict__ recall, const double* __restrict__ f1,
                                                        const int64_t* __restrict__ npos, int K, int G, int W, double* __restrict__ smooth_f1,
                                                        int32_t* __restrict__ best, double* __restrict__ best_conf, double* __restrict__ at_best) {
    __shared__ double s_mean[kMaxGrid];
    __shared__ double s_v[1024];
    __shared__ int s_j[1024];
    const int tid = threadIdx.x, half = W / 2;
    for (int j = tid; j < G; j += 1024) s_mean[j] = mean_f1[j];
    __syncthreads();
    double bv = 0.0;
    int bj = 0x7FFFFFFF;
    for (int j = tid; j < G; j += 1024) {
        double sum = 0.0;
        for (int i = j - half; i <= j + half; ++i) sum += s_mean[min(max(i, 0), G - 1)];
        const double v = sum / (double)W;
        smooth_f1[j] = v;
        if (bj == 0x7FFFFFFF || v > bv) { bv = v; bj = j; }                       // j ascends: the first maximum of this thread
    }
    s_v[tid] = bv; s_j[tid] = bj;
    __syncthreads();
    for (int o = 512; o; o >>= 1) {
        if (tid < o) {
            const double ov = s_v[tid + o];
            const int oj = s_j[tid + o];
            const int mj = s_j[tid];
            if (oj != 0x7FFFFFFF && (mj == 0x7FFFFFFF || ov > s_v[tid] || (ov == s_v[tid] && oj < mj))) { s_v[tid] = ov; s_j[tid] = oj; }
        }
        __syncthreads();
    }
    const int b = s_j[0];
    if (tid == 0) { best[0] = b; best_conf[0] = (double)b / (double)(G - 1); }
    for (int k = tid; k < K; k += 1024) {
        const size_t o = (size_t)k * G + b;
        at_best[3 * k] = precision[o]; at_best[3 * k + 1] = recall[o]; at_best[3 * k + 2] = f1[o];
    }
    if (tid < 3) {                                                                // means of P / R / F1 over the classes with positives
        const double* src = tid == 0 ? precision : (tid == 1 ? recall : f1);
        double sum = 0.0;
        int cnt = 0;
        for (int k = 0; k < K; ++k)
            if (npos[k] != 0) { sum += src[(size_t)k * G + b]; ++cnt; }
        at_best[3 * K + tid] = cnt ? sum / (double)cnt : -1.0;
    }
}

// ---- confusion -----------------------------------------------------------------------------------------------------------------
// dm[D]: -2 not considered, -1 free, else the packed index of the matched ground truth; gm[T] alike with the matched detection
__global__ __launch_bounds__(kConfThreads) void rep_confusion_kernel(const float* __restrict__ det_boxes, const float* __restrict__ det_labels,
                                                                     const float* __restrict__ det_scores, const int32_t* __restrict__ det_off,
                                                                     const float* __restrict__ true_boxes, const float* __restrict__ true_labels,
                                                                     const float* __restrict__ true_crowd, const int32_t* __restrict__ true_off,
                                                                     const float* __restrict__ image_sizes, int n_images, int n_classes, double conf,
                                                                     double thr, int32_t* dm, int32_t* gm, unsigned long long* matrix) {
    constexpr int NW = kConfThreads / kWave;
    __shared__ double s_tab[kConfTab];
    __shared__ double s_v[NW];
    __shared__ long long s_i[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = n_classes - 1;
    const double none = __longlong_as_double(0x7FF8000000000000ll);               // NaN: no candidate
    for (int img = blockIdx.x; img < n_images; img += gridDim.x) {
        const int d0 = det_off ? det_off[img] : 0, d1 = det_off ? det_off[img + 1] : 0;
        const int g0 = true_off ? true_off[img] : 0, g1 = true_off ? true_off[img + 1] : 0;
        const int nd = d1 - d0, ng = g1 - g0;
        double W, H;
        size_of(image_sizes, img, W, H);
        for (int d = d0 + tid; d < d1; d += kConfThreads) dm[d] = (class_of(det_labels[d], n_classes) && (double)det_scores[d] > conf) ? -1 : -2;
        for (int g = g0 + tid; g < g1; g += kConfThreads) gm[g] = class_of(true_labels[g], n_classes) ? -1 : -2;
        __syncthreads();
        const long long pairs = (long long)nd * ng;
        const bool use_tab = pairs <= kConfTab;
        if (use_tab) {
            for (int e = tid; e < (int)pairs; e += kConfThreads) {
                const int dd = e / ng, gg = e - dd * ng;
                double v = none;
                if (dm[d0 + dd] == -1 && gm[g0 + gg] == -1) {
                    const double u = iou_of(geo_of(det_boxes, (size_t)(d0 + dd), W, H), geo_of(true_boxes, (size_t)(g0 + gg), W, H), false);
                    if (u > thr) v = u;
                }
                s_tab[e] = v;
            }
            __syncthreads();
        }
        const int rounds = min(nd, ng);
        for (int r = 0; r < rounds; ++r) {
            double bv = 0.0;
            long long bi = -1;                                                    // pair index dd * ng + gg: smaller = earlier in the tie order
            if (use_tab) {
                for (int e = tid; e < (int)pairs; e += kConfThreads) {
                    const double v = s_tab[e];
                    if (v == v && (bi < 0 || v > bv)) { bv = v; bi = e; }         // e ascends
                }
            } else {
                for (int dd = tid; dd < nd; dd += kConfThreads) {
                    if (dm[d0 + dd] != -1) continue;
                    const geo dg = geo_of(det_boxes, (size_t)(d0 + dd), W, H);
                    for (int gg = 0; gg < ng; ++gg) {
                        if (gm[g0 + gg] != -1) continue;
                        const double v = iou_of(dg, geo_of(true_boxes, (size_t)(g0 + gg), W, H), false);
                        if (v > thr && (bi < 0 || v > bv)) { bv = v; bi = (long long)dd * ng + gg; }   // the pair index ascends
                    }
                }
            }
            for (int o = 32; o; o >>= 1) {
                const double ov = __shfl_down(bv, o);
                const long long oi = __shfl_down(bi, o);
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            __syncthreads();                                                      // the previous round's readers are done
            if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
            __syncthreads();
            bv = s_v[0]; bi = s_i[0];
            for (int w = 1; w < NW; ++w) {
                const double ov = s_v[w];
                const long long oi = s_i[w];
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (bi < 0) break;                                                    // workgroup-uniform: no candidate is left
            const int dd = (int)(bi / ng), gg = (int)(bi - (long long)dd * ng);
            if (tid == 0) { dm[d0 + dd] = g0 + gg; gm[g0 + gg] = d0 + dd; }
            if (use_tab) {
                for (int q = tid; q < ng; q += kConfThreads) s_tab[dd * ng + q] = none;
                for (int q = tid; q < nd; q += kConfThreads) s_tab[q * ng + gg] = none;
            }
            __syncthreads();
        }
        for (int g = g0 + tid; g < g1; g += kConfThreads) {
            const int m = gm[g];
            if (m == -2 || true_crowd[g] != 0.f) continue;
            const int col = (int)class_of(true_labels[g], n_classes) - 1;
            const int row = m >= 0 ? (int)class_of(det_labels[m], n_classes) - 1 : K;
            atomicAdd(&matrix[(size_t)row * (K + 1) + col], 1ull);
        }
        for (int d = d0 + tid; d < d1; d += kConfThreads)
            if (dm[d] == -1) atomicAdd(&matrix[(size_t)((int)class_of(det_labels[d], n_classes) - 1) * (K + 1) + K], 1ull);
    }
}

struct curves_ws_layout { size_t keys, vals, cum, bsum, seg, total; };

void curves_layout(int64_t D, int n_classes, curves_ws_layout& L) {
    size_t o = 0;
    const size_t n2 = (size_t)sort_size(D);
    L.keys = o; o = align256(o + n2 * 8);
    L.vals = o; o = align256(o + n2 * 4);
    L.cum = o;  o = align256(o + n2 * 4);
    L.bsum = o; o = align256(o + (size_t)cdiv((int64_t)n2, kScanBlock) * 4);
    L.seg = o;  o = align256(o + (size_t)(n_classes + 1) * 4);
    L.total = o;
}

int curves_check_sizes(const char* who, int64_t D, int64_t T, int n_classes, int G, int W) {
    MNY_REQUIRE(n_classes >= 2 && n_classes <= (int)kNoClass, "%s: n_classes %d outside 2..255 (it counts the background entry)", who, n_classes);
    MNY_REQUIRE(D >= 0 && T >= 0 && D <= ((int64_t)1 << 30) && T <= ((int64_t)1 << 30), "%s: bad sizes D=%lld T=%lld (limit 2^30)", who, (long long)D,
                (long long)T);
    MNY_REQUIRE(G >= 2 && G <= kMaxGrid, "%s: grid of %d points outside 2..%d", who, G, kMaxGrid);
    MNY_REQUIRE(W >= 1 && W <= G && (W & 1), "%s: smoothing window %d is not an odd number in 1..%d", who, W, G);
    return 0;
}

int confusion_check_sizes(const char* who, int64_t D, int64_t T, int n_images, int n_classes) {
    MNY_REQUIRE(n_classes >= 2 && n_classes <= (int)kNoClass, "%s: n_classes %d outside 2..255 (it counts the background entry)", who, n_classes);
    MNY_REQUIRE(n_images >= 0 && n_images < (1 << 24), "%s: n_images %d outside 0..2^24-1", who, n_images);
    MNY_REQUIRE(D >= 0 && T >= 0 && D <= ((int64_t)1 << 30) && T <= ((int64_t)1 << 30), "%s: bad sizes D=%lld T=%lld (limit 2^30)", who, (long long)D,
                (long long)T);
    return 0;
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_det_curves_ws_bytes(int64_t D, int64_t T, int n_classes, int G, int W) {
    if (curves_check_sizes("mny_det_curves_ws_bytes", D, T, n_classes, G, W) != 0) return 0;
    curves_ws_layout L;
    curves_layout(D, n_classes, L);
    return L.total;
}

extern "C" int mny_det_curves(const float* det_labels, const float* det_scores, const int32_t* det_match, const uint8_t* det_ignore, int64_t D,
                              const float* true_labels, const float* true_crowd, int64_t T, int n_classes, int G, int W, int64_t* tp, int64_t* fp,
                              int64_t* npos, double* precision, double* recall, double* f1, double* mean_f1, double* smooth_f1, int32_t* best,
                              double* best_conf, double* at_best, void* ws, void* stream) {
    if (int rc = curves_check_sizes("mny_det_curves", D, T, n_classes, G, W)) return rc;
    MNY_REQUIRE(tp && fp && npos && precision && recall && f1 && mean_f1 && smooth_f1 && best && best_conf && at_best && ws,
                "mny_det_curves: null output / workspace");
    MNY_REQUIRE(D == 0 || (det_labels && det_scores && det_match && det_ignore), "mny_det_curves: null detection input");
    MNY_REQUIRE(T == 0 || (true_labels && true_crowd), "mny_det_curves: null ground-truth input");
    hipStream_t st = (hipStream_t)stream;
    curves_ws_layout L;
    curves_layout(D, n_classes, L);
    char* w = (char*)ws;
    uint64_t* keys = (uint64_t*)(w + L.keys);
    uint32_t *vals = (uint32_t*)(w + L.vals), *cum = (uint32_t*)(w + L.cum), *bsum = (uint32_t*)(w + L.bsum);
    int32_t* seg = (int32_t*)(w + L.seg);
    const int K = n_classes - 1;
    if (hipMemsetAsync(npos, 0, (size_t)K * 8, st) != hipSuccess) { set_error("mny_det_curves: memset failed"); return MNY_EHIP; }
    if (T > 0) rep_npos_kernel<<<(int)cdiv(T, 256), 256, 0, st>>>(true_labels, true_crowd, (int)T, n_classes, (unsigned long long*)npos);
    if (D > 0) {
        rep_key_kernel<<<(int)cdiv(D, 256), 256, 0, st>>>(det_labels, det_scores, det_match, det_ignore, (int)D, n_classes, keys, vals);
        if (int rc = sort_pairs(keys, vals, (int)D, st)) return rc;
        const int nb = (int)cdiv(D, kScanBlock);
        rep_scan_count_kernel<<<nb, kScanBlock, 0, st>>>(vals, (int)D, bsum);
        rep_scan_sums_kernel<<<1, kScanBlock, 0, st>>>(bsum, nb);
        rep_scan_apply_kernel<<<nb, kScanBlock, 0, st>>>(vals, (int)D, bsum, cum);
    }
    rep_bounds_kernel<<<(int)cdiv(K + 1, 256), 256, 0, st>>>(keys, (int)D, K, seg);
    rep_count_kernel<<<dim3((unsigned)cdiv(G, 256), (unsigned)K), 256, 0, st>>>(keys, cum, seg, npos, G, tp, fp, precision, recall, f1);
    rep_mean_kernel<<<(int)cdiv(G, 256), 256, 0, st>>>(f1, npos, K, G, mean_f1);
    rep_best_kernel<<<1, 1024, 0, st>>>(mean_f1, precision, recall, f1, npos, K, G, W, smooth_f1, best, best_conf, at_best);
    return check_launch("mny_det_curves");
}

extern "C" size_t mny_det_confusion_ws_bytes(int64_t D, int64_t T, int n_images, int n_classes) {
    if (confusion_check_sizes("mny_det_confusion_ws_bytes", D, T, n_images, n_classes) != 0) return 0;
    return align256((size_t)(D > 0 ? D : 1) * 4) + align256((size_t)(T > 0 ? T : 1) * 4);
}

extern "C" int mny_det_confusion(const float* det_boxes, const float* det_labels, const float* det_scores, const int32_t* det_off,
                                 const float* true_boxes, const float* true_labels, const float* true_crowd, const int32_t* true_off,
                                 const float* image_sizes, int n_images, int64_t D, int64_t T, int n_classes, double conf, double iou_thr,
                                 int accumulate, int64_t* matrix, int32_t* det_gt, void* ws, void* stream) {
    if (int rc = confusion_check_sizes("mny_det_confusion", D, T, n_images, n_classes)) return rc;
    MNY_REQUIRE(conf == conf && iou_thr == iou_thr, "mny_det_confusion: conf / iou_thr is NaN");
    MNY_REQUIRE(accumulate == 0 || accumulate == 1, "mny_det_confusion: accumulate %d is neither 0 nor 1", accumulate);
    MNY_REQUIRE(matrix && ws, "mny_det_confusion: null output / workspace");
    MNY_REQUIRE(D == 0 || (det_boxes && det_labels && det_scores && det_off && n_images > 0), "mny_det_confusion: null detection input");
    MNY_REQUIRE(T == 0 || (true_boxes && true_labels && true_crowd && true_off && n_images > 0), "mny_det_confusion: null ground-truth input");
    hipStream_t st = (hipStream_t)stream;
    const int K = n_classes - 1;
    int32_t* dm = det_gt ? det_gt : (int32_t*)ws;
    int32_t* gm = (int32_t*)((char*)ws + align256((size_t)(D > 0 ? D : 1) * 4));
    if (!accumulate && hipMemsetAsync(matrix, 0, (size_t)(K + 1) * (K + 1) * 8, st) != hipSuccess) {
        set_error("mny_det_confusion: memset failed");
        return MNY_EHIP;
    }
    if (n_images > 0 && (D > 0 || T > 0))
        rep_confusion_kernel<<<n_images < 16384 ? n_images : 16384, kConfThreads, 0, st>>>(
            det_boxes, det_labels, det_scores, D > 0 ? det_off : nullptr, true_boxes, true_labels, true_crowd, T > 0 ? true_off : nullptr, image_sizes,
            n_images, n_classes, conf, iou_thr, dm, gm, (unsigned long long*)matrix);
    return check_launch("mny_det_confusion");
}
