// Device-side training augmentation (include/mnyolo.h: mny_aug_photometric / mny_aug_batch / mny_aug_seg_batch).
// Replaces the pixel half of the reference's train-phase sample path (image_augmentation.py transform_od + Mosaic,
// folder2lmdb.py collate_fn); the host made every random draw.  Launch sequence of mny_aug_batch:
//   lsum    : per item with a contrast op, the integer sum of L over the image after the ops before it
//   photo   : the whole photometric chain at source resolution, uint8 -> uint8, once into the workspace
//   hpass<bicubic, tile> / vpass<tile> : mosaic members -> their tile rectangle of the uint8 canvas (+ channel sums)
//   fill    : each mask rectangle outside its tile <- trunc(sum / count) of the resized tile
//   hpass<bilinear, sample> / vpass<sample> : the geometric view (single image) or the canvas -> [3,out_h,out_w] fp32
// The resample passes read the source THROUGH the geometry (expand canvas + filler 127, crop window, flip) and compute
// their Pillow taps (Resample.c precompute_coeffs + normalize_coeffs_8bpc, fp64) per output index in the thread that
// uses them.  An axis whose size does not change gets the taps {1 << 22, 0, ...}: bit-identical to Pillow skipping it.
// mny_aug_seg_batch (one launch, aug_seg_kernel) gives the same items' id maps the geometric trip and OpenCV's INTER_AREA
// resize per class; see the section below.
// Integer work throughout; the fp32/fp64 arithmetic mirrors Pillow's C statement by statement, so the file is compiled
// with -ffp-contract=off.
#include "common.h"

static_assert(sizeof(mny_aug_item) == 392, "mny_aug_item layout (augment.py ITEM)");
static_assert(sizeof(mny_aug_sample) == 16, "mny_aug_sample layout");

namespace mny {
namespace {

constexpr int kPrec = 32 - 8 - 2;
constexpr uint8_t kFiller = 127;             // torch.ones * 0.5 -> to_pil_image mul(255).byte()

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct aug_layout {
    size_t lsum, tsum, photo, photo_stride, tmp, tmp_stride, canvas, canvas_stride, total;
};

aug_layout make_layout(int n_items, int n_out, int n_mosaic, int max_h, int max_w, int canvas, int out_h, int out_w) {
    aug_layout L;
    size_t o = 256;
    L.lsum = o; o = al(o + (size_t)n_items * 8);
    L.tsum = o; o = al(o + (size_t)n_items * 3 * 8);
    L.photo_stride = al((size_t)max_h * max_w * 3);
    L.photo = o; o += L.photo_stride * n_items;
    const size_t view_h = (size_t)(n_mosaic > 0 && canvas > max_h ? canvas : max_h);
    size_t t = view_h * out_w * 3;
    if (n_mosaic > 0 && (size_t)max_h * canvas * 3 > t) t = (size_t)max_h * canvas * 3;
    L.tmp_stride = al(t);
    L.tmp = o; o += L.tmp_stride * (size_t)(n_items > n_out ? n_items : n_out);
    L.canvas_stride = al((size_t)canvas * canvas * 3);
    L.canvas = o; o += n_mosaic > 0 ? L.canvas_stride * n_mosaic : 0;
    L.total = o;
    return L;
}

__device__ __forceinline__ void flag(char* ws, int v) { atomicCAS((int*)ws, 0, v); }

// ---- photometric ops (Pillow C, statement by statement) ----------------------------------------------------------
__device__ __forceinline__ int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }   // Convert.c rgb2l

__device__ __forceinline__ int blend(int deg, int v, float a) {                                               // Blend.c
    const float t = (float)deg + a * (float)(v - deg);
    if (a >= 0.f && a <= 1.0f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ void hue_px(int& r, int& g, int& b, int shift) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = mx;
    if (mx != mn) {                                                                                            // Convert.c rgb2hsv_row
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
        float h;
        if (r == mx) h = bc - gc;
        else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
        uh = clip255((int)((double)h * 255.0));
        us = clip255((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) { r = g = b = uv; return; }                                                                   // Convert.c hsv2rgb
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double vf = (double)(float)uv;
    const int p = clip255((int)round(vf * (1.0 - (double)fs)));
    const int q = clip255((int)round(vf * (1.0 - (double)(fs * f))));
    const int t = clip255((int)round(vf * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// ops [0, upto) of the item's chain on one pixel; `cmean` = contrast's grey level
__device__ __forceinline__ void apply_ops(const mny_aug_item& it, int upto, int cmean, int& r, int& g, int& b) {
    for (int k = 0; k < upto; ++k) {
        const int op = it.op[k];
        const float a = it.factor[k];
        if (op == MNY_AUG_BRIGHTNESS) { r = blend(0, r, a); g = blend(0, g, a); b = blend(0, b, a); }
        else if (op == MNY_AUG_CONTRAST) { r = blend(cmean, r, a); g = blend(cmean, g, a); b = blend(cmean, b, a); }
        else if (op == MNY_AUG_SATURATION) { const int l = lum(r, g, b); r = blend(l, r, a); g = blend(l, g, a); b = blend(l, b, a); }
        else if (op == MNY_AUG_HUE) hue_px(r, g, b, it.hue_shift);
        else { r = it.gamma_map[r]; g = it.gamma_map[g]; b = it.gamma_map[b]; }
    }
}

__device__ __forceinline__ int contrast_at(const mny_aug_item& it) {
    for (int k = 0; k < it.n_ops; ++k)
        if (it.op[k] == MNY_AUG_CONTRAST) return k;
    return -1;
}

__device__ bool src_ok(const mny_aug_item& it, int max_h, int max_w) {
    if (it.src.h < 1 || it.src.w < 1 || it.src.h > max_h || it.src.w > max_w || (it.src.offset & 3) || it.src.offset < 0) return false;
    if (it.n_ops < 0 || it.n_ops > 5) return false;
    for (int k = 0; k < it.n_ops; ++k)
        if (it.op[k] < 0 || it.op[k] > MNY_AUG_GAMMA) return false;
    return true;
}

__device__ bool geo_ok(const mny_aug_item& it, int max_h, int max_w) {
    if (!src_ok(it, max_h, max_w)) return false;
    if (it.exp_h < it.src.h || it.exp_w < it.src.w || it.exp_h > max_h || it.exp_w > max_w) return false;
    if (it.exp_top < 0 || it.exp_left < 0 || it.exp_top + it.src.h > it.exp_h || it.exp_left + it.src.w > it.exp_w) return false;
    if (it.crop_h < 1 || it.crop_w < 1 || it.crop_top < 0 || it.crop_left < 0) return false;
    return it.crop_top + it.crop_h <= it.exp_h && it.crop_left + it.crop_w <= it.exp_w;
}

__device__ bool tile_ok(const mny_aug_item& it, int canvas) {
    return it.tile_w >= 1 && it.tile_h >= 1 && it.mask_x0 >= 0 && it.mask_y0 >= 0 && it.mask_x1 <= canvas && it.mask_y1 <= canvas &&
           it.tile_x >= it.mask_x0 && it.tile_y >= it.mask_y0 && it.tile_x + it.tile_w <= it.mask_x1 && it.tile_y + it.tile_h <= it.mask_y1;
}

// 4 pixels = 12 bytes per thread, 3 dword loads / stores when the group is whole
__device__ __forceinline__ void load4(const uint8_t* p, int n, int* px) {
    if (n == 4) {
        const uint32_t* q = (const uint32_t*)p;
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        const uint32_t w[3] = {w0, w1, w2};
#pragma unroll
        for (int i = 0; i < 12; ++i) px[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
    } else {
        for (int i = 0; i < 3 * n; ++i) px[i] = p[i];
    }
}

__device__ __forceinline__ void store4(uint8_t* p, int n, const int* px) {
    if (n == 4) {
        uint32_t w[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i >> 2] |= (uint32_t)px[i] << (8 * (i & 3));
        uint32_t* q = (uint32_t*)p;
        q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
    } else {
        for (int i = 0; i < 3 * n; ++i) p[i] = (uint8_t)px[i];
    }
}

// grid (cdiv(max_h*max_w, 1024), n_items), 256 threads x 4 pixels
__global__ __launch_bounds__(256) void aug_lsum_kernel(const uint8_t* __restrict__ src, const mny_aug_item* __restrict__ items, int max_h, int max_w,
                                                       char* __restrict__ ws, size_t lsum_off) {
    const mny_aug_item& it = items[blockIdx.y];
    if (!src_ok(it, max_h, max_w)) return;
    const int c = contrast_at(it);
    if (c < 0) return;
    const int npx = it.src.h * it.src.w;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if ((int64_t)blockIdx.x * 1024 >= npx) return;
    unsigned s = 0;
    if (p0 < npx) {
        const int n = min(4, npx - p0);
        int px[12];
        load4(src + it.src.offset + (size_t)p0 * 3, n, px);
        for (int i = 0; i < n; ++i) {
            int r = px[3 * i], g = px[3 * i + 1], b = px[3 * i + 2];
            apply_ops(it, c, 0, r, g, b);
            s += lum(r, g, b);
        }
    }
    __shared__ unsigned red;
    if (threadIdx.x == 0) red = 0;
    __syncthreads();
    atomicAdd(&red, s);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd((unsigned long long*)(ws + lsum_off) + blockIdx.y, (unsigned long long)red);
}

// grid (cdiv(max_h*max_w, 1024), n_items): the full chain; dst = dst_base + (per_item ? item * stride : src.offset)
__global__ __launch_bounds__(256) void aug_photo_kernel(const uint8_t* __restrict__ src, const mny_aug_item* __restrict__ items, int max_h, int max_w,
                                                        char* __restrict__ ws, size_t lsum_off, uint8_t* __restrict__ dst_base, size_t stride) {
    const mny_aug_item& it = items[blockIdx.y];
    if (!src_ok(it, max_h, max_w)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) flag(ws, blockIdx.y + 1);
        return;
    }
    const int npx = it.src.h * it.src.w;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npx) return;
    int cmean = 0;
    if (contrast_at(it) >= 0) {
        const unsigned long long S = ((const unsigned long long*)(ws + lsum_off))[blockIdx.y];
        cmean = (int)((double)S / (double)npx + 0.5);                                           // int(ImageStat mean + 0.5)
    }
    const int n = min(4, npx - p0);
    int px[12];
    load4(src + it.src.offset + (size_t)p0 * 3, n, px);
    for (int i = 0; i < n; ++i) apply_ops(it, it.n_ops, cmean, px[3 * i], px[3 * i + 1], px[3 * i + 2]);
    uint8_t* dst = dst_base + (stride ? stride * blockIdx.y : (size_t)it.src.offset);
    store4(dst + (size_t)p0 * 3, n, px);
}

// ---- resample ------------------------------------------------------------------------------------------------------
template <int BICUBIC>
__device__ __forceinline__ double filt(double x) {
    if (x < 0.0) x = -x;
    if (BICUBIC) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

template <int BICUBIC>
struct axis_taps {
    int lo, n;
    double center, ss, ww;
    __device__ __forceinline__ axis_taps(int in_size, int out_size, int xx) {
        const double scale = (double)in_size / (double)out_size;
        const double fs = scale < 1.0 ? 1.0 : scale;
        const double support = (BICUBIC ? 2.0 : 1.0) * fs;
        ss = 1.0 / fs;
        center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        lo = xmin;
        n = xmax - xmin;
        ww = 0.0;
        for (int x = 0; x < n; ++x) ww += filt<BICUBIC>((x + lo - center + 0.5) * ss);
    }
    __device__ __forceinline__ int k(int x) const {
        double w = filt<BICUBIC>((x + lo - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        return w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrec)) : (int)(0.5 + w * (double)(1 << kPrec));
    }
};

__device__ __forceinline__ int clip8(int v) {
    v >>= kPrec;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// A readable image: either an item's geometric view over its photometric buffer, or a canvas.
struct view {
    const uint8_t* base;
    int w;                            // row length of `base` in pixels
    int vh, vw;                       // view size
    int ox, oy;                       // crop origin minus expand origin: source = (ox + x', oy + y)
    int sh, sw;                       // source bounds (outside -> filler)
    int flip;
    __device__ __forceinline__ const uint8_t* at(int x, int y) const {
        const int xx = (flip ? vw - 1 - x : x) + ox, yy = y + oy;
        if (xx < 0 || yy < 0 || xx >= sw || yy >= sh) return nullptr;
        return base + ((size_t)yy * w + xx) * 3;
    }
};

__device__ __forceinline__ view item_view(const mny_aug_item& it, const char* ws, const aug_layout& L, int item) {
    view v;
    v.base = (const uint8_t*)ws + L.photo + L.photo_stride * item;
    v.w = it.src.w;
    v.vh = it.crop_h; v.vw = it.crop_w;
    v.ox = it.crop_left - it.exp_left; v.oy = it.crop_top - it.exp_top;
    v.sh = it.src.h; v.sw = it.src.w;
    v.flip = it.flip;
    return v;
}

__device__ __forceinline__ view canvas_view(const char* ws, const aug_layout& L, int slot, int canvas) {
    view v;
    v.base = (const uint8_t*)ws + L.canvas + L.canvas_stride * slot;
    v.w = v.vh = v.vw = v.sh = v.sw = canvas;
    v.ox = v.oy = 0;
    v.flip = 0;
    return v;
}

// 0 = the sample can be drawn; otherwise the status value: 1 + the first bad item, or -(1 + sample) for a bad record
__device__ int sample_check(const mny_aug_sample& s, const mny_aug_item* items, int n_items, int n_mosaic, int idx, int max_h, int max_w, int canvas) {
    if (s.n_items < 1 || s.n_items > 4 || s.first_item < 0 || s.first_item + s.n_items > n_items) return -(1 + idx);
    if (s.n_items > 1 && (s.canvas_slot < 0 || s.canvas_slot >= n_mosaic)) return -(1 + idx);
    for (int k = 0; k < s.n_items; ++k) {
        const mny_aug_item& it = items[s.first_item + k];
        if (it.sample != idx) return -(1 + idx);
        if (!geo_ok(it, max_h, max_w) || (s.n_items > 1 && !tile_ok(it, canvas))) return 1 + s.first_item + k;
    }
    return 0;
}

__device__ __forceinline__ bool sample_ok(const mny_aug_sample& s, const mny_aug_item* items, int n_items, int n_mosaic, int idx, int max_h, int max_w,
                                          int canvas) {
    return sample_check(s, items, n_items, n_mosaic, idx, max_h, max_w, canvas) == 0;
}

// Job = a mosaic member (TILE: view -> [tile_h, tile_w] into the canvas, bicubic) or an output sample (view -> [out_h,
// out_w] fp32, bilinear).  Resolves the job's view and output size; false = nothing to do.
template <int TILE>
__device__ __forceinline__ bool job(int j, const mny_aug_item* items, int n_items, const mny_aug_sample* samples, int n_mosaic, int max_h, int max_w,
                                    int canvas, int out_h, int out_w, const char* ws, const aug_layout& L, view& v, int& oh, int& ow, bool& ok) {
    ok = true;
    if (TILE) {
        const mny_aug_item& it = items[j];
        if (it.sample < 0) return false;
        const mny_aug_sample& s = samples[it.sample];
        if (s.n_items < 2 || s.first_item > j || j >= s.first_item + s.n_items) return false;
        if (!geo_ok(it, max_h, max_w) || !tile_ok(it, canvas) || s.canvas_slot < 0 || s.canvas_slot >= n_mosaic) return false;
        v = item_view(it, ws, L, j);
        oh = it.tile_h; ow = it.tile_w;
        return true;
    }
    const mny_aug_sample& s = samples[j];
    oh = out_h; ow = out_w;
    const int bad = sample_check(s, items, n_items, n_mosaic, j, max_h, max_w, canvas);
    ok = bad == 0;
    if (!ok) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) flag((char*)ws, bad);
        return true;
    }
    v = s.n_items == 1 ? item_view(items[s.first_item], ws, L, s.first_item) : canvas_view(ws, L, s.canvas_slot, canvas);
    return true;
}

// Horizontal pass: thread = one output column x, 4 rows.  Block 64 x 4 threads -> 64 columns x 16 rows.
// grid (cdiv(max out w, 64), cdiv(max view h, 16), jobs)
template <int TILE>
__global__ __launch_bounds__(256) void aug_hpass_kernel(const mny_aug_item* __restrict__ items, int n_items, const mny_aug_sample* __restrict__ samples,
                                                        int n_mosaic, int max_h, int max_w, int canvas, int out_h, int out_w, aug_layout L,
                                                        char* __restrict__ ws) {
    view v; int oh, ow; bool ok;
    const int j = blockIdx.z;
    if (!job<TILE>(j, items, n_items, samples, n_mosaic, max_h, max_w, canvas, out_h, out_w, ws, L, v, oh, ow, ok) || !ok) return;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y0 = (blockIdx.y * 4 + threadIdx.y) * 4;
    if (x >= ow || y0 >= v.vh) return;
    const int nr = min(4, v.vh - y0);
    const axis_taps<TILE> tp(v.vw, ow, x);
    int acc[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (kPrec - 1);
    for (int t = 0; t < tp.n; ++t) {
        const int c = tp.k(t);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < nr) {
                const uint8_t* p = v.at(tp.lo + t, y0 + r);
                const int pr = p ? p[0] : kFiller, pg = p ? p[1] : kFiller, pb = p ? p[2] : kFiller;
                acc[r][0] += pr * c; acc[r][1] += pg * c; acc[r][2] += pb * c;
            }
        }
    }
    uint8_t* tmp = (uint8_t*)ws + L.tmp + L.tmp_stride * j;
    for (int r = 0; r < nr; ++r) {
        uint8_t* o = tmp + ((size_t)(y0 + r) * ow + x) * 3;
        o[0] = (uint8_t)clip8(acc[r][0]); o[1] = (uint8_t)clip8(acc[r][1]); o[2] = (uint8_t)clip8(acc[r][2]);
    }
}

// Vertical pass: thread = one output row y, 4 consecutive columns.  Block 64 x 4 threads -> 256 columns x 4 rows.
// grid (cdiv(max out w, 256), cdiv(max out h, 4), jobs).  TILE: uint8 into the canvas + per-channel sums of the tile;
// otherwise fp32 (u8/255 - mean)/std into the sample's three planes (zeros for a rejected sample).
template <int TILE>
__global__ __launch_bounds__(256) void aug_vpass_kernel(const mny_aug_item* __restrict__ items, int n_items, const mny_aug_sample* __restrict__ samples,
                                                        int n_mosaic, int max_h, int max_w, int canvas, int out_h, int out_w, aug_layout L,
                                                        char* __restrict__ ws, float3 mean, float3 stdv, float* __restrict__ out) {
    view v; int oh, ow; bool ok;
    const int j = blockIdx.z;
    if (!job<TILE>(j, items, n_items, samples, n_mosaic, max_h, max_w, canvas, out_h, out_w, ws, L, v, oh, ow, ok)) return;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    const bool live = x0 < ow && y < oh;
    const int nc = live ? min(4, ow - x0) : 0;
    int acc[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 1 << (kPrec - 1);
    if (live && ok) {
        const axis_taps<TILE> tp(v.vh, oh, y);
        const uint8_t* tmp = (const uint8_t*)ws + L.tmp + L.tmp_stride * j;
        for (int t = 0; t < tp.n; ++t) {
            const int k = tp.k(t);
            const uint8_t* q = tmp + ((size_t)(tp.lo + t) * ow + x0) * 3;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < nc) { acc[c][0] += q[3 * c] * k; acc[c][1] += q[3 * c + 1] * k; acc[c][2] += q[3 * c + 2] * k; }
        }
    }
    if (TILE) {
        const mny_aug_item& it = items[j];
        unsigned s0 = 0, s1 = 0, s2 = 0;
        if (live) {
            uint8_t* cv = (uint8_t*)ws + L.canvas + L.canvas_stride * samples[it.sample].canvas_slot;
            uint8_t* o = cv + ((size_t)(it.tile_y + y) * canvas + it.tile_x + x0) * 3;
            for (int c = 0; c < nc; ++c) {
                const int r = clip8(acc[c][0]), g = clip8(acc[c][1]), b = clip8(acc[c][2]);
                o[3 * c] = (uint8_t)r; o[3 * c + 1] = (uint8_t)g; o[3 * c + 2] = (uint8_t)b;
                s0 += r; s1 += g; s2 += b;
            }
        }
        __shared__ unsigned red[3];
        const int tid = threadIdx.y * 64 + threadIdx.x;
        if (tid < 3) red[tid] = 0;
        __syncthreads();
        if (live) { atomicAdd(&red[0], s0); atomicAdd(&red[1], s1); atomicAdd(&red[2], s2); }
        __syncthreads();
        if (tid < 3) atomicAdd((unsigned long long*)(ws + L.tsum) + 3 * j + tid, (unsigned long long)red[tid]);
        return;
    }
    if (!live) return;
    const size_t plane = (size_t)oh * ow;
    float* o = out + (size_t)j * 3 * plane + (size_t)y * ow + x0;
    const float m[3] = {mean.x, mean.y, mean.z}, sd[3] = {stdv.x, stdv.y, stdv.z};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = ok ? ((float)clip8(acc[c][ch]) / 255.f - m[ch]) / sd[ch] : 0.f;     // ToTensor .div(255); Normalize
        float* p = o + ch * plane;
        if (nc == 4 && ((uintptr_t)p & 15) == 0) *(float4*)p = make_float4(r[0], r[1], r[2], r[3]);
        else
            for (int c = 0; c < nc; ++c) p[c] = r[c];
    }
}

// Mask fill: grid (cdiv(canvas*canvas, 256), n_out); each pixel of a mosaic canvas lies in exactly one member's mask.
__global__ __launch_bounds__(256) void aug_fill_kernel(const mny_aug_item* __restrict__ items, int n_items, const mny_aug_sample* __restrict__ samples,
                                                       int n_mosaic, int max_h, int max_w, int canvas, aug_layout L, char* __restrict__ ws) {
    const int si = blockIdx.y;
    const mny_aug_sample& s = samples[si];
    if (s.n_items < 2 || !sample_ok(s, items, n_items, n_mosaic, si, max_h, max_w, canvas)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= canvas * canvas) return;
    const int y = i / canvas, x = i - y * canvas;
    uint8_t* o = (uint8_t*)ws + L.canvas + L.canvas_stride * s.canvas_slot + (size_t)i * 3;
    for (int k = 0; k < s.n_items; ++k) {
        const int j = s.first_item + k;
        const mny_aug_item& it = items[j];
        if (x < it.mask_x0 || x >= it.mask_x1 || y < it.mask_y0 || y >= it.mask_y1) continue;
        if (x >= it.tile_x && x < it.tile_x + it.tile_w && y >= it.tile_y && y < it.tile_y + it.tile_h) return;     // written by the tile pass
        const unsigned long long* S = (const unsigned long long*)(ws + L.tsum) + 3 * j;
        const double cnt = (double)it.tile_w * (double)it.tile_h;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(int)((double)S[c] / cnt);                               // np.mean -> astype(uint8)
        return;
    }
    o[0] = o[1] = o[2] = 0;                                                                                 // np.zeros background
}

// ---- segmentation maps (mny_aug_seg_batch) -----------------------------------------------------------------------
// The id map makes the image's geometric trip (expand border 0, crop window, flip); per class c = 1..C the 0/255 image
// (id == c) is resized with OpenCV's INTER_AREA (resize.cpp computeResizeAreaTab / ResizeArea_, ResizeAreaFast_) and
// divided by 255.  One block per (sample, destination row): the threads split the band's (source row, dx) pairs, each
// reads its ids ONCE for all classes and forms the horizontal sums in tap order into LDS; then one thread per (dx, c)
// runs the vertical accumulation in row order.  Bands taller than the LDS buffer are walked in chunks, `sum` carried.
constexpr int kSegLds = 8192;                // floats: per (dx, c) the carried sum, then R rows of horizontal sums
constexpr int kSegMaxClasses = MNY_AUG_SEG_MAX_CLASSES;

__device__ __forceinline__ double area_scale(int ssize, int dsize) { return 1.0 / ((double)dsize / (double)ssize); }

__device__ __forceinline__ bool area_fast(int ssize, int dsize) {
    const double scale = area_scale(ssize, dsize);
    return fabs(scale - (double)(int)scale) < 2.220446049250313e-16;                           // DBL_EPSILON
}

// The taps of one destination index in emission order: source indices start .. start + n - 1, the first / last one
// partial (lo / hi).  `fast`: the integer-scale cell, weights unused.
struct area_taps {
    int start, n, lo, hi;
    float a_lo, a_mid, a_hi;
    __device__ __forceinline__ area_taps(int ssize, int dsize, int d, bool fast) {
        const double scale = area_scale(ssize, dsize);
        lo = hi = 0;
        a_lo = a_mid = a_hi = 0.f;
        if (fast) {
            n = (int)scale;
            start = d * n;
            return;
        }
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = fmin(scale, ssize - f1);
        int s1 = (int)ceil(f1);
        const int s2 = min((int)floor(f2), ssize - 1);
        s1 = min(s1, s2);
        lo = s1 - f1 > 1e-3;
        hi = f2 - s2 > 1e-3;
        a_lo = (float)((s1 - f1) / cell);
        a_mid = (float)(1.0 / cell);
        a_hi = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
        start = s1 - lo;
        n = lo + (s2 - s1) + hi;
    }
    __device__ __forceinline__ float k(int t) const { return (lo && t == 0) ? a_lo : ((hi && t == n - 1) ? a_hi : a_mid); }
};

__device__ bool seg_geo_ok(const mny_aug_item& it, int64_t off, int max_h, int max_w, int out_h, int out_w) {
    if (it.src.h < 1 || it.src.w < 1 || it.src.h > max_h || it.src.w > max_w || (off & 3) || off < 0) return false;
    if (it.exp_h < it.src.h || it.exp_w < it.src.w || it.exp_h > max_h || it.exp_w > max_w) return false;
    if (it.exp_top < 0 || it.exp_left < 0 || it.exp_top + it.src.h > it.exp_h || it.exp_left + it.src.w > it.exp_w) return false;
    if (it.crop_top < 0 || it.crop_left < 0 || it.crop_h < out_h || it.crop_w < out_w) return false;      // scale < 1: another OpenCV path
    return it.crop_top + it.crop_h <= it.exp_h && it.crop_left + it.crop_w <= it.exp_w;
}

// grid (out_h, n_out), 256 threads
__global__ __launch_bounds__(256) void aug_seg_kernel(const uint8_t* __restrict__ seg, const int64_t* __restrict__ offs,
                                                      const mny_aug_item* __restrict__ items, int n_items, const mny_aug_sample* __restrict__ samples,
                                                      int C, int max_h, int max_w, int out_h, int out_w, float* __restrict__ out, char* __restrict__ ws) {
    __shared__ float lds[kSegLds];
    const int si = blockIdx.y, dy = blockIdx.x, tid = threadIdx.x;
    const int WC = out_w * C;
    float* o = out + ((size_t)si * out_h + dy) * WC;
    const mny_aug_sample s = samples[si];
    int bad = 0;
    if (s.n_items != 1 || s.first_item < 0 || s.first_item >= n_items) bad = -(1 + si);
    else if (items[s.first_item].sample != si) bad = -(1 + si);
    else if (!seg_geo_ok(items[s.first_item], offs[s.first_item], max_h, max_w, out_h, out_w)) bad = 1 + s.first_item;
    if (bad) {                                                                      // block-uniform: the row is zeros, nothing is read
        if (dy == 0 && tid == 0) flag(ws, bad);
        for (int e = tid; e < WC; e += 256) o[e] = 0.f;
        return;
    }
    const mny_aug_item& it = items[s.first_item];
    const int64_t off = offs[s.first_item];
    const int h = it.src.h, w = it.src.w, ch = it.crop_h, cw = it.crop_w;
    const int ox = it.crop_left - it.exp_left, oy = it.crop_top - it.exp_top, flip = it.flip;
    const bool fast = area_fast(ch, out_h) && area_fast(cw, out_w);
    const area_taps ty(ch, out_h, dy, fast);
    const uint32_t* words = (const uint32_t*)seg;                                   // seg and every offset are 4-byte aligned
    float* sum = lds;
    float* buf = lds + WC;
    const int R = (kSegLds - WC) / WC;                                              // >= 1 (checked on the host)
    for (int e = tid; e < WC; e += 256) sum[e] = 0.f;                               // the bits of int 0 too; owner-only from here on
    for (int r0 = 0; r0 < ty.n; r0 += R) {
        const int nr = min(R, ty.n - r0);
        __syncthreads();                                                            // the previous chunk has been consumed
        for (int p = tid; p < nr * out_w; p += 256) {
            const int r = p / out_w, dx = p - r * out_w;
            const area_taps tx(cw, out_w, dx, fast);
            const int y = ty.start + r0 + r, yy = y + oy;
            float acc[kSegMaxClasses];
            int cnt[kSegMaxClasses];
#pragma unroll
            for (int c = 0; c < kSegMaxClasses; ++c) { acc[c] = 0.f; cnt[c] = 0; }
            if (y >= 0 && y < ch && yy >= 0 && yy < h) {
                const int64_t row = off + (int64_t)yy * w;
                int64_t have = -1;
                uint32_t word = 0;
                for (int t = 0; t < tx.n; ++t) {
                    const int x = tx.start + t;
                    const int xx = (flip ? cw - 1 - x : x) + ox;
                    if (x < 0 || x >= cw || xx < 0 || xx >= w) continue;            // border: 0 in every class
                    const int64_t a = row + xx;
                    if ((a >> 2) != have) { have = a >> 2; word = words[have]; }
                    const int id = (word >> (8 * (int)(a & 3))) & 255;
                    if (fast) {
#pragma unroll
                        for (int c = 0; c < kSegMaxClasses; ++c) cnt[c] += id == c + 1;
                    } else {
                        const float v = 255.f * tx.k(t);
#pragma unroll
                        for (int c = 0; c < kSegMaxClasses; ++c) acc[c] = acc[c] + (id == c + 1 ? v : 0.f);
                    }
                }
            }
            float* b = buf + (size_t)p * C;
#pragma unroll
            for (int c = 0; c < kSegMaxClasses; ++c)
                if (c < C) b[c] = fast ? __int_as_float(cnt[c]) : acc[c];
        }
        __syncthreads();
        for (int e = tid; e < WC; e += 256) {
            if (fast) {
                int isum = __float_as_int(sum[e]);
                for (int r = 0; r < nr; ++r) isum += __float_as_int(buf[r * WC + e]);
                sum[e] = __int_as_float(isum);
            } else {
                float v = sum[e];
                for (int r = 0; r < nr; ++r) {
                    const float beta = ty.k(r0 + r), bv = buf[r * WC + e];
                    v = r0 + r == 0 ? beta * bv : v + beta * bv;
                }
                sum[e] = v;
            }
        }
    }
    const area_taps tx0(cw, out_w, 0, fast);
    for (int e = tid; e < WC; e += 256) {
        float v = sum[e];
        if (fast) v = (float)(255 * __float_as_int(v)) * (1.f / (float)(tx0.n * ty.n));
        v = rintf(v);                                                               // saturate_cast<uchar>: nearest even, clamped
        v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
        o[e] = v / 255.0f;
    }
}

}  // namespace
}  // namespace mny

using namespace mny;

extern "C" size_t mny_aug_ws_bytes(int n_items, int n_out, int n_mosaic, int max_in_h, int max_in_w, int canvas, int out_h, int out_w) {
    if (n_items < 1 || n_out < 0 || n_mosaic < 0 || max_in_h < 1 || max_in_w < 1 || out_h < 1 || out_w < 1 || (n_mosaic > 0 && canvas < 1)) return 0;
    return make_layout(n_items, n_out, n_mosaic, max_in_h, max_in_w, canvas, out_h, out_w).total;
}

extern "C" int mny_aug_photometric(const uint8_t* src, const mny_aug_item* items, int n, int max_in_h, int max_in_w, uint8_t* dst, void* ws, void* stream) {
    MNY_REQUIRE(src && items && dst && ws, "mny_aug_photometric: null pointer");
    MNY_REQUIRE(n >= 1 && n <= 65535 && max_in_h >= 1 && max_in_w >= 1 && (int64_t)max_in_h * max_in_w < ((int64_t)1 << 31) / 4,
                "mny_aug_photometric: bad sizes n=%d max %dx%d", n, max_in_h, max_in_w);
    hipStream_t st = (hipStream_t)stream;
    const aug_layout L = make_layout(n, 0, 0, max_in_h, max_in_w, 0, 1, 1);
    if (hipMemsetAsync(ws, 0, L.lsum + (size_t)n * 8, st) != hipSuccess) { set_error("mny_aug_photometric: memset failed"); return MNY_EHIP; }
    const dim3 g((unsigned)cdiv((int64_t)max_in_h * max_in_w, 1024), n);
    aug_lsum_kernel<<<g, 256, 0, st>>>(src, items, max_in_h, max_in_w, (char*)ws, L.lsum);
    aug_photo_kernel<<<g, 256, 0, st>>>(src, items, max_in_h, max_in_w, (char*)ws, L.lsum, dst, 0);
    return check_launch("mny_aug_photometric");
}

extern "C" int mny_aug_batch(const uint8_t* src, const mny_aug_item* items, int n_items, const mny_aug_sample* samples, int n_out, int max_in_h, int max_in_w,
                             int canvas, int n_mosaic, int out_h, int out_w, const float* mean3, const float* std3, float* out, void* ws, void* stream) {
    MNY_REQUIRE(src && items && samples && mean3 && std3 && out && ws, "mny_aug_batch: null pointer");
    MNY_REQUIRE(n_items >= 1 && n_items <= 65535 && n_out >= 1 && n_out <= 65535 && n_mosaic >= 0 && max_in_h >= 1 && max_in_w >= 1 && out_h >= 1 &&
                    out_w >= 1 && (n_mosaic == 0 || canvas >= 1),
                "mny_aug_batch: bad sizes items=%d out=%d mosaics=%d in<=%dx%d canvas=%d out=%dx%d", n_items, n_out, n_mosaic, max_in_h, max_in_w, canvas,
                out_h, out_w);
    const int64_t vh = n_mosaic > 0 && canvas > max_in_h ? canvas : max_in_h;
    MNY_REQUIRE((int64_t)max_in_h * max_in_w < ((int64_t)1 << 31) / 4 && (int64_t)canvas * canvas < ((int64_t)1 << 31) / 4 &&
                    vh * out_w < ((int64_t)1 << 31) / 4 && (int64_t)max_in_h * canvas < ((int64_t)1 << 31) / 4,
                "mny_aug_batch: images too large");
    MNY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "mny_aug_batch: std must be non-zero");
    hipStream_t st = (hipStream_t)stream;
    const aug_layout L = make_layout(n_items, n_out, n_mosaic, max_in_h, max_in_w, canvas, out_h, out_w);
    char* w = (char*)ws;
    if (hipMemsetAsync(ws, 0, L.photo, st) != hipSuccess) { set_error("mny_aug_batch: memset failed"); return MNY_EHIP; }   // status + sums
    const dim3 gp((unsigned)cdiv((int64_t)max_in_h * max_in_w, 1024), n_items);
    aug_lsum_kernel<<<gp, 256, 0, st>>>(src, items, max_in_h, max_in_w, w, L.lsum);
    aug_photo_kernel<<<gp, 256, 0, st>>>(src, items, max_in_h, max_in_w, w, L.lsum, (uint8_t*)w + L.photo, L.photo_stride);
    const dim3 blk(64, 4);
    if (n_mosaic > 0) {
        aug_hpass_kernel<1><<<dim3((unsigned)cdiv(canvas, 64), (unsigned)cdiv(max_in_h, 16), n_items), blk, 0, st>>>(
            items, n_items, samples, n_mosaic, max_in_h, max_in_w, canvas, out_h, out_w, L, w);
        aug_vpass_kernel<1><<<dim3((unsigned)cdiv(canvas, 256), (unsigned)cdiv(canvas, 4), n_items), blk, 0, st>>>(
            items, n_items, samples, n_mosaic, max_in_h, max_in_w, canvas, out_h, out_w, L, w, make_float3(0, 0, 0), make_float3(1, 1, 1), out);
        aug_fill_kernel<<<dim3((unsigned)cdiv((int64_t)canvas * canvas, 256), n_out), 256, 0, st>>>(items, n_items, samples, n_mosaic, max_in_h, max_in_w,
                                                                                                   canvas, L, w);
    }
    aug_hpass_kernel<0><<<dim3((unsigned)cdiv(out_w, 64), (unsigned)cdiv(vh, 16), n_out), blk, 0, st>>>(items, n_items, samples, n_mosaic, max_in_h,
                                                                                                        max_in_w, canvas, out_h, out_w, L, w);
    aug_vpass_kernel<0><<<dim3((unsigned)cdiv(out_w, 256), (unsigned)cdiv(out_h, 4), n_out), blk, 0, st>>>(
        items, n_items, samples, n_mosaic, max_in_h, max_in_w, canvas, out_h, out_w, L, w, make_float3(mean3[0], mean3[1], mean3[2]),
        make_float3(std3[0], std3[1], std3[2]), out);
    return check_launch("mny_aug_batch");
}

extern "C" size_t mny_aug_seg_ws_bytes(int n_items, int n_out, int n_classes, int max_in_h, int max_in_w, int out_h, int out_w) {
    if (n_items < 1 || n_out < 1 || n_classes < 1 || n_classes > kSegMaxClasses || max_in_h < 1 || max_in_w < 1 || out_h < 1 || out_w < 1) return 0;
    return 256;                                                                     // the status word
}

extern "C" int mny_aug_seg_batch(const uint8_t* seg_src, const int64_t* seg_offsets, const mny_aug_item* items, int n_items, const mny_aug_sample* samples,
                                 int n_out, int n_classes, int max_in_h, int max_in_w, int out_h, int out_w, float* out, void* ws, void* stream) {
    MNY_REQUIRE(seg_src && seg_offsets && items && samples && out && ws, "mny_aug_seg_batch: null pointer");
    MNY_REQUIRE(((uintptr_t)seg_src & 3) == 0, "mny_aug_seg_batch: seg_src must be 4-byte aligned");
    MNY_REQUIRE(n_classes >= 1 && n_classes <= kSegMaxClasses, "mny_aug_seg_batch: n_classes=%d outside 1..%d", n_classes, kSegMaxClasses);
    MNY_REQUIRE(n_items >= 1 && n_items <= 65535 && n_out >= 1 && n_out <= 65535 && max_in_h >= 1 && max_in_w >= 1 && out_h >= 1 && out_w >= 1 &&
                    (int64_t)max_in_h * max_in_w < ((int64_t)1 << 31),
                "mny_aug_seg_batch: bad sizes items=%d out=%d in<=%dx%d out=%dx%d", n_items, n_out, max_in_h, max_in_w, out_h, out_w);
    MNY_REQUIRE((int64_t)out_w * n_classes * 2 <= kSegLds, "mny_aug_seg_batch: out_w * n_classes = %lld exceeds %d", (long long)out_w * n_classes,
                kSegLds / 2);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, 256, st) != hipSuccess) { set_error("mny_aug_seg_batch: memset failed"); return MNY_EHIP; }
    aug_seg_kernel<<<dim3(out_h, n_out), 256, 0, st>>>(seg_src, seg_offsets, items, n_items, samples, n_classes, max_in_h, max_in_w, out_h, out_w, out,
                                                       (char*)ws);
    return check_launch("mny_aug_seg_batch");
}
