// COCO-style detection metrics on the device (include/mnyolo.h: mny_coco_eval): AP over IoU thresholds, by object size, AR at
// detection caps — the arithmetic of pycocotools' COCOeval for iouType='bbox', restated in tests/coco_ref.py.
//   order  : key (image | class | descending score), value = stored index; the pair sort of pairsort.h.  The position inside a
//            run of equal (image, class) is the rank of the detection in its segment; ranks >= max_dets[-1] drop out.
//   match  : a workgroup per non-empty (image, class) segment, a lane per (area range, IoU threshold) pair.  Each lane runs the
//            package's sequential scan: detections in score order, ground truths in two passes over the stored order (not
//            ignored, then ignored).  IoUs (fp64) sit in an LDS table when detections x objects fit, else are recomputed per
//            pair; matched flags are one 64-bit word per object (bit = lane), in LDS up to kMaxG objects, else in the workspace.
//   accum  : second ordering (class | descending score, position in the first ordering = the package's concatenation order);
//            a workgroup per (class, area, cap, threshold): block scan of TP / FP over the class's run in chunks, precision,
//            chunk-local suffix maximum, and per recall threshold a binary search on the monotone recall of the chunk.
//            precision[r] = max of pr[i] over { i : rc[i] >= rec_thrs[r] }, which is what the package's right-to-left envelope
//            followed by searchsorted(rc, r, 'left') reads.
//   summary: fixed-order fp64 sums.
// No host synchronisation, no floating-point atomics (integer adds and ORs only), the same bits run to run.
// Compiled with -ffp-contract=off: areas and IoUs must round like the separate fp64 operations of the specification.
#include "boxgeo.h"
#include "common.h"
#include "pairsort.h"

#include <cstring>

namespace mny {
namespace {

constexpr int kMaxIou = 16, kMaxRec = 128, kMaxCaps = 4, kMaxArea = 8, kMaxStats = 32;
constexpr int kMaxG = 512;            // objects of one segment whose index / area / matched words live in LDS
constexpr int kTabDoubles = 6144;     // 48 KB IoU table: detections x objects of one segment
constexpr int kAccThreads = 1024;
constexpr uint32_t kNoSeg = 0xFFFFFFFFu;
constexpr uint32_t kNoClass = 255;

struct coco_params {
    double iou[kMaxIou], rec[kMaxRec], area[kMaxArea][2];
    int32_t maxdet[kMaxCaps];
    int n_iou, n_rec, n_area, n_maxdet;
};
struct coco_stats {
    int32_t d[kMaxStats][4];
};

// ---- order ---------------------------------------------------------------------------------------------------------------------
__global__ void coco_key_kernel(const float* __restrict__ det_labels, const float* __restrict__ det_scores, const int32_t* __restrict__ det_off,
                                int n_images, int D, int n_classes, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const uint32_t c = class_of(det_labels[d], n_classes);
    const float s = det_scores[d];
    const uint32_t sb = s == 0.f ? 0u : __float_as_uint(s);                      // -0.0 ties with 0.0
    const uint32_t asc = sb ^ ((sb >> 31) ? 0xFFFFFFFFu : 0x80000000u);          // order-preserving map of a float
    const uint32_t desc = s != s ? 0xFFFFFFFFu : ~asc;                           // NaN after every number
    const uint32_t seg = c ? ((uint32_t)image_of(det_off, n_images, d) << 8) | c : kNoSeg;
    keys[d] = ((uint64_t)seg << 32) | desc;
    vals[d] = (uint32_t)d;
}

// rank in the (image, class) segment; the key of the second ordering (class | descending score), value = position in the first
__global__ void coco_rank_kernel(const uint64_t* __restrict__ keys, int D, int cap, int32_t* __restrict__ rank, uint64_t* __restrict__ keys2,
                                 uint32_t* __restrict__ vals2) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D) return;
    const uint64_t k = keys[p];
    const uint32_t seg = (uint32_t)(k >> 32);
    int r = 0x7FFFFFFF;
    if (seg != kNoSeg) r = p - lower_bound_key(keys, D, (uint64_t)seg << 32);
    rank[p] = r;
    keys2[p] = ((uint64_t)(r < cap ? (seg & 255u) : kNoClass) << 32) | (uint32_t)k;
    vals2[p] = (uint32_t)p;
}

__global__ void coco_fill_kernel(int32_t* __restrict__ det_match, uint8_t* __restrict__ det_ignore, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (det_match) det_match[i] = -2;
        if (det_ignore) det_ignore[i] = 0;
    }
}

// npig[class-1][area range]: ground truths that are no crowd and whose area lies in the range (integer adds: order-free)
__global__ void coco_npig_kernel(const float* __restrict__ true_boxes, const float* __restrict__ true_labels, const float* __restrict__ true_crowd,
                                 const int32_t* __restrict__ true_off, const float* __restrict__ image_sizes, int n_images, int T, int n_classes,
                                 coco_params P, int32_t* __restrict__ npig) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= T) return;
    const uint32_t c = class_of(true_labels[j], n_classes);
    if (!c || true_crowd[j] != 0.f) return;
    double W, H;
    size_of(image_sizes, image_of(true_off, n_images, j), W, H);
    const double area = geo_of(true_boxes, (size_t)j, W, H).area;
    for (int a = 0; a < P.n_area; ++a)
        if (!(area < P.area[a][0] || area > P.area[a][1])) atomicAdd(&npig[(c - 1) * P.n_area + a], 1);
}

// ---- match ---------------------------------------------------------------------------------------------------------------------
// masks[(p * nw + wave) * 2 + {0, 1}]: bit (pair & 63) of word (pair >> 6) = matched / ignored, p = position in the first ordering
__global__ __launch_bounds__(128) void coco_match_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const int32_t* __restrict__ rank,
                                                         int D, const float* __restrict__ det_boxes, const float* __restrict__ true_boxes,
                                                         const float* __restrict__ true_labels, const float* __restrict__ true_crowd,
                                                         const int32_t* __restrict__ true_off, const float* __restrict__ image_sizes, int T, coco_params P,
                                                         unsigned long long* __restrict__ masks, unsigned long long* gflags,
                                                         int32_t* __restrict__ det_match, uint8_t* __restrict__ det_ignore) {
    __shared__ double s_tab[kTabDoubles];
    __shared__ double s_garea[kMaxG];
    __shared__ int s_gidx[kMaxG];                      // packed object index | crowd << 31
    __shared__ unsigned long long s_flags[2][kMaxG];
    __shared__ int s_G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const bool active = tid < P.n_area * P.n_iou;
    const int a = active ? tid / P.n_iou : 0, t = active ? tid % P.n_iou : 0;
    const double lo = P.area[a][0], hi = P.area[a][1];
    const double thr = fmin(P.iou[t], 1 - 1e-10);
    const int cap = P.maxdet[P.n_maxdet - 1];
    const unsigned long long bit = 1ull << lane;

    for (int p = blockIdx.x; p < D; p += gridDim.x) {
        if (rank[p] != 0) continue;                                               // block-uniform: p starts a segment
        const uint32_t seg = (uint32_t)(keys[p] >> 32);
        const int img = (int)(seg >> 8), c = (int)(seg & 255u);
        const int pend = lower_bound_key(keys, D, (uint64_t)(seg + 1) << 32);
        const int nd = min(pend - p, cap);
        double W, H;
        size_of(image_sizes, img, W, H);
        const int t0 = true_off[img], t1 = true_off[img + 1];
        __syncthreads();                                                          // the previous segment's readers are done
        if (wave == 0) {                                                          // the class's objects of this image, in stored order
            int G = 0;
            for (int base = t0; base < t1; base += 64) {
                const int j = base + lane;
                const bool mine = j < t1 && true_labels[j] == (float)c;
                const unsigned long long m = __ballot(mine);
                if (mine) {
                    const int k = G + __popcll(m & (bit - 1));
                    if (k < kMaxG) {
                        s_gidx[k] = j | (true_crowd[j] != 0.f ? (int)0x80000000 : 0);
                        s_garea[k] = geo_of(true_boxes, (size_t)j, W, H).area;
                    }
                }
                G += __popcll(m);
            }
            if (lane == 0) s_G = G;
        }
        __syncthreads();
        const int G = s_G;
        const bool small = G <= kMaxG;
        const int n_iter = small ? G : t1 - t0;
        const bool use_tab = small && (long long)nd * G <= kTabDoubles;
        unsigned long long* flags = small ? s_flags[wave] : gflags + (size_t)wave * T + t0;
        if (small)
            for (int k = lane; k < G; k += 64) s_flags[wave][k] = 0;
        if (use_tab)
            for (int e = tid; e < nd * G; e += blockDim.x) {
                const int dd = e / G, k = e - dd * G;
                const int gi = s_gidx[k];
                s_tab[e] = iou_of(geo_of(det_boxes, vals[p + dd], W, H), geo_of(true_boxes, (size_t)(gi & 0x7FFFFFFF), W, H), gi < 0);
            }
        __syncthreads();

        for (int dd = 0; dd < nd; ++dd) {
            const uint32_t sd = vals[p + dd];
            const geo dg = geo_of(det_boxes, sd, W, H);
            double best = thr;
            int m = -1, mj = -1;
            bool mig = false;
            for (int pass = 0; pass < 2; ++pass) {
                const bool scan = active && m < 0;                                // a match among the not-ignored ends the scan
                if (!__any(scan)) break;
                for (int k = 0; k < n_iter; ++k) {
                    int j;
                    bool crowd;
                    double garea, v;
                    if (small) {
                        const int gi = s_gidx[k];
                        j = gi & 0x7FFFFFFF; crowd = gi < 0; garea = s_garea[k];
                        v = use_tab ? s_tab[dd * G + k] : iou_of(dg, geo_of(true_boxes, (size_t)j, W, H), crowd);
                    } else {
                        j = t0 + k;
                        if (true_labels[j] != (float)c) continue;
                        crowd = true_crowd[j] != 0.f;
                        const geo gg = geo_of(true_boxes, (size_t)j, W, H);
                        garea = gg.area;
                        v = iou_of(dg, gg, crowd);
                    }
                    const bool ig = crowd || garea < lo || garea > hi;
                    if (!scan || ig != (pass == 1)) continue;
                    const unsigned long long f = __hip_atomic_load(&flags[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((f & bit) && !crowd) continue;
                    if (v < best) continue;
                    best = v; m = k; mj = j; mig = ig;                            // >=: among equal IoUs the later object wins
                }
            }
            if (active && m >= 0) atomicOr(&flags[m], bit);
            const bool ign = m >= 0 ? mig : (dg.area < lo || dg.area > hi);
            const unsigned long long mm = __ballot(active && m >= 0), im = __ballot(active && ign);
            if (lane == 0) {
                masks[((size_t)(p + dd) * nw + wave) * 2] = mm;
                masks[((size_t)(p + dd) * nw + wave) * 2 + 1] = im;
            }
            if (active && det_match) det_match[(size_t)tid * D + sd] = m >= 0 ? mj : -1;
            if (active && det_ignore) det_ignore[(size_t)tid * D + sd] = ign ? 1 : 0;
        }
    }
}

// ---- accumulate ----------------------------------------------------------------------------------------------------------------
// blockIdx.x = ((k * A + a) * M + m) * T_ + t
__global__ __launch_bounds__(kAccThreads) void coco_accum_kernel(const uint64_t* __restrict__ keys2, const uint32_t* __restrict__ vals2, int D,
                                                                 const int32_t* __restrict__ rank, const unsigned long long* __restrict__ masks, int nw,
                                                                 const int32_t* __restrict__ npig, coco_params P, int K, double* __restrict__ precision,
                                                                 double* __restrict__ recall) {
    constexpr int NW = kAccThreads / kWave;
    __shared__ int s_tp[kAccThreads];
    __shared__ double s_pr[kAccThreads];
    __shared__ uint32_t s_scan[NW];
    __shared__ double s_wmax[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int t = b % P.n_iou; b /= P.n_iou;
    const int m = b % P.n_maxdet; b /= P.n_maxdet;
    const int a = b % P.n_area;
    const int k = b / P.n_area;
    const size_t rc_at = (((size_t)t * K + k) * P.n_area + a) * P.n_maxdet + m;
    auto pr_at = [&](int r) { return ((((size_t)t * P.n_rec + r) * K + k) * P.n_area + a) * P.n_maxdet + m; };
    const int np = npig[k * P.n_area + a];
    if (np == 0) {                                                                // no object to find: undefined
        if (tid < P.n_rec) precision[pr_at(tid)] = -1.0;
        if (tid == 0) recall[rc_at] = -1.0;
        return;
    }
    const double npd = (double)np;
    const int capm = P.maxdet[m], pair = a * P.n_iou + t, word = pair >> 6, sh = pair & 63;
    const int lo = lower_bound_key(keys2, D, (uint64_t)(k + 1) << 32), hi = lower_bound_key(keys2, D, (uint64_t)(k + 2) << 32);
    const double rthr = tid < P.n_rec ? P.rec[tid] : 0.0;
    double best = 0.0;
    uint32_t ctp0 = 0, cfp0 = 0;
    for (int base = lo; base < hi; base += kAccThreads) {
        const int i = base + tid, n = min(kAccThreads, hi - base);
        uint32_t mine = 0;
        if (i < hi) {
            const uint32_t p = vals2[i];
            if (rank[p] < capm) {                                                 // beyond this cap: absent, same as ignored
                const size_t w = ((size_t)p * nw + word) * 2;
                const uint32_t mt = (uint32_t)(masks[w] >> sh) & 1u, ig = (uint32_t)(masks[w + 1] >> sh) & 1u;
                mine = (mt & ~ig & 1u) | ((~mt & ~ig & 1u) << 16);                // tp | fp << 16, chunk-local counts fit 16 bits
            }
        }
        uint32_t inc = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        __syncthreads();                                                          // the previous chunk's readers are done
        if (lane == 63) s_scan[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < NW; ++w) {
            const uint32_t s = s_scan[w];
            if (w < wave) before += s;
            total += s;
        }
        inc += before;
        const uint32_t tpi = ctp0 + (inc & 0xFFFFu), fpi = cfp0 + (inc >> 16);
        const double tp = (double)tpi, fp = (double)fpi;
        double pr = i < hi ? tp / ((fp + tp) + 2.220446049250313e-16) : 0.0;
        for (int o = 1; o < 64; o <<= 1) {                                        // maximum over this and every later element of the chunk
            const double dn = __shfl_down(pr, o);
            if (lane + o < 64) pr = fmax(pr, dn);
        }
        if (lane == 0) s_wmax[wave] = pr;
        s_tp[tid] = (int)tpi;
        __syncthreads();
        for (int w = wave + 1; w < NW; ++w) pr = fmax(pr, s_wmax[w]);
        s_pr[tid] = pr;
        __syncthreads();
        if (tid < P.n_rec) {                                                      // first element of the chunk with recall >= threshold
            int l = 0, h = n;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if ((double)s_tp[mid] / npd < rthr) l = mid + 1; else h = mid;
            }
            if (l < n) best = fmax(best, s_pr[l]);
        }
        ctp0 += total & 0xFFFFu;
        cfp0 += total >> 16;
    }
    if (tid < P.n_rec) precision[pr_at(tid)] = best;
    if (tid == 0) recall[rc_at] = (double)ctp0 / npd;
}

// ---- summary -------------------------------------------------------------------------------------------------------------------
// blocks 0..S-1: the statistics of stat_desc; blocks S..S+K-1: per_class_ap.  Mean of the entries > -1, or -1 without any.
__global__ __launch_bounds__(256) void coco_summary_kernel(const double* __restrict__ precision, const double* __restrict__ recall, coco_params P, int K,
                                                           coco_stats SD, int S, double* __restrict__ stats, double* __restrict__ per_class_ap) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const bool per_class = blk >= S;
    const int is_recall = per_class ? 0 : SD.d[blk][0], tsel = per_class ? -1 : SD.d[blk][1];
    const int a = per_class ? 0 : SD.d[blk][2], m = per_class ? P.n_maxdet - 1 : SD.d[blk][3];
    const int k0 = per_class ? blk - S : 0, nk = per_class ? 1 : K;
    const int nt = tsel < 0 ? P.n_iou : 1, nr = is_recall ? 1 : P.n_rec;
    double sum = 0.0;
    int cnt = 0;
    for (int e = tid; e < nt * nr * nk; e += 256) {
        const int k = k0 + e % nk, r = (e / nk) % nr, t = tsel < 0 ? e / (nk * nr) : tsel;
        const double v = is_recall ? recall[(((size_t)t * K + k) * P.n_area + a) * P.n_maxdet + m]
                                   : precision[((((size_t)t * P.n_rec + r) * K + k) * P.n_area + a) * P.n_maxdet + m];
        if (v > -1.0) { sum += v; ++cnt; }
    }
    s_sum[tid] = sum; s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double out = s_cnt[0] ? s_sum[0] / (double)s_cnt[0] : -1.0;
        if (per_class) per_class_ap[k0] = out; else stats[blk] = out;
    }
}

struct coco_ws_layout {
    size_t keys, vals, keys2, vals2, rank, masks, npig, gflags, total;
    int nw;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

void coco_layout(int64_t D, int64_t T, int n_classes, int n_iou, int n_area, coco_ws_layout& L) {
    size_t o = 0;
    const size_t d = (size_t)(D > 0 ? D : 1), t = (size_t)(T > 0 ? T : 1), n2 = (size_t)sort_size(D);
    L.nw = (int)cdiv((int64_t)n_iou * n_area, 64);
    L.keys = o;   o = align256(o + n2 * 8);
    L.vals = o;   o = align256(o + n2 * 4);
    L.keys2 = o;  o = align256(o + n2 * 8);
    L.vals2 = o;  o = align256(o + n2 * 4);
    L.rank = o;   o = align256(o + d * 4);
    L.masks = o;  o = align256(o + d * (size_t)L.nw * 16);
    L.npig = o;   o = align256(o + (size_t)(n_classes - 1) * n_area * 4);
    L.gflags = o; o = align256(o + t * (size_t)L.nw * 8);
    L.total = o;
}

int coco_check_sizes(const char* who, int64_t D, int64_t T, int n_images, int n_classes, int n_iou, int n_rec, int n_area, int n_maxdet) {
    MNY_REQUIRE(n_classes >= 2 && n_classes <= (int)kNoClass, "%s: n_classes %d outside 2..255 (it counts the background entry)", who, n_classes);
    MNY_REQUIRE(n_images >= 0 && n_images < (1 << 24), "%s: n_images %d outside 0..2^24-1", who, n_images);
    MNY_REQUIRE(D >= 0 && T >= 0 && D <= ((int64_t)1 << 30) && T <= ((int64_t)1 << 30), "%s: bad sizes D=%lld T=%lld (limit 2^30)", who, (long long)D,
                (long long)T);
    MNY_REQUIRE(n_iou >= 1 && n_iou <= kMaxIou, "%s: %d IoU thresholds outside 1..%d", who, n_iou, kMaxIou);
    MNY_REQUIRE(n_rec >= 1 && n_rec <= kMaxRec, "%s: %d recall thresholds outside 1..%d", who, n_rec, kMaxRec);
    MNY_REQUIRE(n_area >= 1 && n_area <= kMaxArea, "%s: %d area ranges outside 1..%d", who, n_area, kMaxArea);
    MNY_REQUIRE(n_maxdet >= 1 && n_maxdet <= kMaxCaps, "%s: %d detection caps outside 1..%d", who, n_maxdet, kMaxCaps);
    return 0;
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_coco_ws_bytes(int64_t D, int64_t T, int n_images, int n_classes, int n_iou, int n_rec, int n_area, int n_maxdet) {
    if (coco_check_sizes("mny_coco_ws_bytes", D, T, n_images, n_classes, n_iou, n_rec, n_area, n_maxdet) != 0) return 0;
    coco_ws_layout L;
    coco_layout(D, T, n_classes, n_iou, n_area, L);
    return L.total;
}

extern "C" int mny_coco_eval(const float* det_boxes, const float* det_labels, const float* det_scores, const int32_t* det_off, const float* true_boxes,
                             const float* true_labels, const float* true_crowd, const int32_t* true_off, const float* image_sizes, int n_images, int64_t D,
                             int64_t T, int n_classes, const double* iou_thrs, int n_iou, const double* rec_thrs, int n_rec, const int32_t* max_dets,
                             int n_maxdet, const double* area_rngs, int n_area, const int32_t* stat_desc, int S, double* precision, double* recall,
                             double* stats, double* per_class_ap, int32_t* det_match, uint8_t* det_ignore, void* ws, void* stream) {
    if (int rc = coco_check_sizes("mny_coco_eval", D, T, n_images, n_classes, n_iou, n_rec, n_area, n_maxdet)) return rc;
    MNY_REQUIRE(iou_thrs && rec_thrs && max_dets && area_rngs, "mny_coco_eval: null parameter array");
    MNY_REQUIRE(S >= 0 && S <= kMaxStats && (S == 0 || (stat_desc && stats)), "mny_coco_eval: %d statistics outside 0..%d, or null stat_desc / stats", S,
                kMaxStats);
    MNY_REQUIRE(precision && recall && per_class_ap && ws, "mny_coco_eval: null output / workspace");
    MNY_REQUIRE(D == 0 || (det_boxes && det_labels && det_scores && det_off && true_off && n_images > 0), "mny_coco_eval: null detection input");
    MNY_REQUIRE(T == 0 || (true_boxes && true_labels && true_crowd && true_off && n_images > 0), "mny_coco_eval: null ground-truth input");
    coco_params P;
    memset(&P, 0, sizeof(P));
    P.n_iou = n_iou; P.n_rec = n_rec; P.n_area = n_area; P.n_maxdet = n_maxdet;
    for (int i = 0; i < n_iou; ++i) P.iou[i] = iou_thrs[i];
    for (int i = 0; i < n_rec; ++i) P.rec[i] = rec_thrs[i];
    for (int i = 0; i < n_area; ++i) { P.area[i][0] = area_rngs[2 * i]; P.area[i][1] = area_rngs[2 * i + 1]; }
    for (int i = 0; i < n_maxdet; ++i) {
        MNY_REQUIRE(max_dets[i] >= 1 && (i == 0 || max_dets[i] >= max_dets[i - 1]), "mny_coco_eval: max_dets must be positive and ascending");
        P.maxdet[i] = max_dets[i];
    }
    coco_stats SD;
    memset(&SD, 0, sizeof(SD));
    for (int s = 0; s < S; ++s) {
        const int32_t* d = stat_desc + 4 * s;
        MNY_REQUIRE(d[1] >= -1 && d[1] < n_iou && d[2] >= 0 && d[2] < n_area && d[3] >= 0 && d[3] < n_maxdet,
                    "mny_coco_eval: stat_desc row %d (%d, %d, %d, %d) names a threshold, area range or cap that does not exist", s, d[0], d[1], d[2], d[3]);
        for (int q = 0; q < 4; ++q) SD.d[s][q] = d[q];
    }
    hipStream_t st = (hipStream_t)stream;
    coco_ws_layout L;
    coco_layout(D, T, n_classes, n_iou, n_area, L);
    char* w = (char*)ws;
    uint64_t *keys = (uint64_t*)(w + L.keys), *keys2 = (uint64_t*)(w + L.keys2);
    uint32_t *vals = (uint32_t*)(w + L.vals), *vals2 = (uint32_t*)(w + L.vals2);
    int32_t *rank = (int32_t*)(w + L.rank), *npig = (int32_t*)(w + L.npig);
    unsigned long long *masks = (unsigned long long*)(w + L.masks), *gflags = (unsigned long long*)(w + L.gflags);
    const int K = n_classes - 1;
    if (hipMemsetAsync(npig, 0, (size_t)K * n_area * 4, st) != hipSuccess) { set_error("mny_coco_eval: memset failed"); return MNY_EHIP; }
    if (T > 0) {
        if (hipMemsetAsync(gflags, 0, (size_t)T * L.nw * 8, st) != hipSuccess) { set_error("mny_coco_eval: memset failed"); return MNY_EHIP; }
        coco_npig_kernel<<<(int)cdiv(T, 256), 256, 0, st>>>(true_boxes, true_labels, true_crowd, true_off, image_sizes, n_images, (int)T, n_classes, P, npig);
    }
    if (D > 0) {
        const int blocks = (int)cdiv(D, 256);
        if (det_match || det_ignore) {
            const size_t n = (size_t)n_area * n_iou * (size_t)D;
            coco_fill_kernel<<<(int)(cdiv((int64_t)n, 256) < 4096 ? cdiv((int64_t)n, 256) : 4096), 256, 0, st>>>(det_match, det_ignore, n);
        }
        coco_key_kernel<<<blocks, 256, 0, st>>>(det_labels, det_scores, det_off, n_images, (int)D, n_classes, keys, vals);
        if (int rc = sort_pairs(keys, vals, (int)D, st)) return rc;
        coco_rank_kernel<<<blocks, 256, 0, st>>>(keys, (int)D, P.maxdet[n_maxdet - 1], rank, keys2, vals2);
        if (int rc = sort_pairs(keys2, vals2, (int)D, st)) return rc;
        coco_match_kernel<<<(int)(D < 4096 ? D : 4096), 64 * L.nw, 0, st>>>(keys, vals, rank, (int)D, det_boxes, true_boxes, true_labels, true_crowd, true_off,
                                                                          image_sizes, (int)T, P, masks, gflags, det_match, det_ignore);
    }
    coco_accum_kernel<<<K * n_area * n_maxdet * n_iou, kAccThreads, 0, st>>>(keys2, vals2, (int)D, rank, masks, L.nw, npig, P, K, precision, recall);
    coco_summary_kernel<<<S + K, 256, 0, st>>>(precision, recall, P, K, SD, S, stats, per_class_ap);
    return check_launch("mny_coco_eval");
}
