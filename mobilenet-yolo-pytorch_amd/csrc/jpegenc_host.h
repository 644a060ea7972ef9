// Host half of the baseline JPEG encoder (include/mnyolo.h: mny_jpeg_enc_layout, mny_jpeg_huffman_batch): the item records with
// their quantisation tables, and the serial part of an encode, headers and Huffman coding of the quantised coefficients that
// mny_jpeg_coef_batch (csrc/jpegenc.hip) left.  Plain C++17 like csrc/jpeg_host.h, whose threading contract it follows: image i
// goes to thread i mod T, each thread owns its code tables on its stack, nothing is allocated.  The stream is the file libjpeg
// writes with its defaults (JFIF 1.01 without density, one DQT per table, SOF0, the four typical Huffman tables of Annex K.3 one
// DHT each, one interleaved scan); csrc/jpegenc.hip exports the entry points, everything here has internal linkage.
#pragma once
#include "jpeg_host.h"

namespace mny_jpegenc_host {

using mny_jpeg_host::kMaxSide;
using mny_jpeg_host::kZigzag;

// ITU-T T.81 Annex K.1, natural order
static const uint8_t kQBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: bits[l - 1] = codes of length l; index 0 luminance, 1 chrominance.  The DC symbols are 0..11.
static const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// the padded block grids of an h x w frame with luma sampling hs x vs; `own` = the blocks of each component's own grid
struct Grid {
    int bw[3], bh[3], obw[3], obh[3];
    int64_t plane_off[3], n_coef;
};
static inline Grid grid(int h, int w, int hs, int vs) {
    Grid g;
    const int mcux = (w + 8 * hs - 1) / (8 * hs), mcuy = (h + 8 * vs - 1) / (8 * vs);
    const int cw = (w + hs - 1) / hs, ch = (h + vs - 1) / vs;
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = mcux * (c == 0 ? hs : 1);
        g.bh[c] = mcuy * (c == 0 ? vs : 1);
        g.obw[c] = ((c == 0 ? w : cw) + 7) / 8;
        g.obh[c] = ((c == 0 ? h : ch) + 7) / 8;
        g.plane_off[c] = off;
        off += (int64_t)g.bw[c] * g.bh[c] * 64;
    }
    g.n_coef = off;
    return g;
}

static inline void qtable(int t, int quality, uint16_t* q) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int v = (kQBase[t][k] * s + 50) / 100;
        q[k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// the records of n frames, coefficient slices one after the other from element 0 -> the int16 count of them all
static inline int64_t enc_layout(const mny_image_desc* desc, int n, int quality, int hs, int vs, mny_jpeg_item* items) {
    uint16_t q[2][64];
    qtable(0, quality, q[0]);
    qtable(1, quality, q[1]);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        mny_jpeg_item* it = items + i;
        memset(it, 0, sizeof(*it));
        const int h = desc[i].h, w = desc[i].w;
        it->h = h;
        it->w = w;
        it->coef_off = total;
        if (h < 1 || w < 1) { it->status = MNY_JPEG_EHEADER; continue; }
        if (h > kMaxSide || w > kMaxSide) { it->status = MNY_JPEG_ETOOLARGE; continue; }
        const Grid g = grid(h, w, hs, vs);
        it->ncomp = 3;
        it->hs = hs;
        it->vs = vs;
        for (int c = 0; c < 3; ++c) {
            it->bw[c] = g.bw[c];
            it->bh[c] = g.bh[c];
            it->plane_off[c] = g.plane_off[c];
            memcpy(it->q[c], q[c ? 1 : 0], sizeof(it->q[c]));
        }
        it->n_coef = g.n_coef;
        total += g.n_coef;
    }
    return total;
}

// what an encoder record must be: a good status, three components, a supported sampling, grids and offsets that follow from the sizes
static inline int check_item(const mny_jpeg_item& it, int64_t coef_elems) {
    if (it.status != MNY_JPEG_OK) return it.status;
    if (it.ncomp != 3) return MNY_JPEG_ECOLORSPACE;
    if (it.h < 1 || it.w < 1) return MNY_JPEG_EHEADER;
    if (it.h > kMaxSide || it.w > kMaxSide) return MNY_JPEG_ETOOLARGE;
    if (!((it.hs == 1 || it.hs == 2) && it.vs >= 1 && it.vs <= it.hs)) return MNY_JPEG_ESAMPLING;
    const Grid g = grid(it.h, it.w, it.hs, it.vs);
    for (int c = 0; c < 3; ++c)
        if (it.bw[c] != g.bw[c] || it.bh[c] != g.bh[c] || it.plane_off[c] != g.plane_off[c]) return MNY_JPEG_EHEADER;
    if (it.n_coef != g.n_coef) return MNY_JPEG_EHEADER;
    if (it.coef_off < 0 || it.coef_off > coef_elems || it.n_coef > coef_elems - it.coef_off) return MNY_JPEG_ECAPACITY;
    for (int k = 0; k < 64; ++k) {
        if (it.q[0][k] < 1 || it.q[0][k] > 255 || it.q[1][k] < 1 || it.q[1][k] > 255) return MNY_JPEG_EPRECISION;
        if (it.q[2][k] != it.q[1][k]) return MNY_JPEG_EHEADER;                    // the stream carries one chrominance table
    }
    return MNY_JPEG_OK;
}

struct HuffEnc {
    uint16_t code[256];
    uint8_t len[256];   // 0: the symbol has no code
};
static inline void build(const uint8_t* bits, const uint8_t* vals, HuffEnc& E) {
    memset(&E, 0, sizeof(E));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            E.code[vals[k]] = (uint16_t)code;
            E.len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}
struct Tables {
    HuffEnc dc[2], ac[2];
};
static inline void build_all(Tables& T) {
    uint8_t dcv[12];
    for (int k = 0; k < 12; ++k) dcv[k] = (uint8_t)k;
    for (int t = 0; t < 2; ++t) {
        build(kDcBits[t], dcv, T.dc[t]);
        build(kAcBits[t], kAcVals[t], T.ac[t]);
    }
}

struct Out {
    uint8_t* p;
    int64_t cap, n;
    uint64_t acc;   // the low nacc bits wait for their byte
    int nacc;
    bool over;      // a byte did not fit: nothing is written from then on
};
static inline void byte(Out& o, int b) {
    if (o.n < o.cap) o.p[o.n++] = (uint8_t)b;
    else o.over = true;
}
static inline void bytes(Out& o, const uint8_t* s, int n) {
    for (int k = 0; k < n; ++k) byte(o, s[k]);
}
static inline void put(Out& o, uint32_t code, int n) {   // n <= 16
    o.acc = (o.acc << n) | code;
    o.nacc += n;
    while (o.nacc >= 8) {
        const int b = (int)((o.acc >> (o.nacc - 8)) & 255);
        byte(o, b);
        if (b == 255) byte(o, 0);
        o.nacc -= 8;
    }
}
static inline void segment(Out& o, int marker, int body) {
    byte(o, 0xFF);
    byte(o, marker);
    byte(o, (body + 2) >> 8);
    byte(o, (body + 2) & 255);
}
static inline int nbits(int v) {   // v >= 0
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

static inline void header(Out& o, const mny_jpeg_item& it) {
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    byte(o, 0xFF);
    byte(o, 0xD8);
    segment(o, 0xE0, 14);
    bytes(o, jfif, 14);
    for (int t = 0; t < 2; ++t) {
        segment(o, 0xDB, 65);
        byte(o, t);
        for (int k = 0; k < 64; ++k) byte(o, it.q[t][kZigzag[k]]);
    }
    const uint8_t sof[15] = {8, (uint8_t)(it.h >> 8), (uint8_t)it.h, (uint8_t)(it.w >> 8), (uint8_t)it.w, 3,
                             1, (uint8_t)((it.hs << 4) | it.vs), 0, 2, 0x11, 1, 3, 0x11, 1};
    segment(o, 0xC0, 15);
    bytes(o, sof, 15);
    uint8_t dcv[12];
    for (int k = 0; k < 12; ++k) dcv[k] = (uint8_t)k;
    for (int t = 0; t < 2; ++t) {
        segment(o, 0xC4, 1 + 16 + 12);
        byte(o, t);
        bytes(o, kDcBits[t], 16);
        bytes(o, dcv, 12);
        segment(o, 0xC4, 1 + 16 + 162);
        byte(o, 0x10 | t);
        bytes(o, kAcBits[t], 16);
        bytes(o, kAcVals[t], 162);
    }
    static const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    segment(o, 0xDA, 10);
    bytes(o, sos, 10);
}

// one block: blk in natural order, or NULL for a padding block (DC `dc`, no AC).  -> false: a value baseline has no category for
static inline bool block(Out& o, const HuffEnc& D, const HuffEnc& A, const int16_t* blk, int dc, int& pred) {
    int diff = dc - pred;
    pred = dc;
    int n = nbits(diff < 0 ? -diff : diff);
    if (n > 11) return false;
    put(o, D.code[n], D.len[n]);
    if (n) put(o, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1), n);
    if (!blk) {
        put(o, A.code[0], A.len[0]);
        return true;
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int a = blk[kZigzag[k]];
        if (a == 0) { ++run; continue; }
        for (; run > 15; run -= 16) put(o, A.code[0xF0], A.len[0xF0]);
        n = nbits(a < 0 ? -a : a);
        if (n > 10) return false;
        put(o, A.code[(run << 4) | n], A.len[(run << 4) | n]);
        put(o, (uint32_t)(a < 0 ? a - 1 : a) & ((1u << n) - 1), n);
        run = 0;
    }
    if (run) put(o, A.code[0], A.len[0]);
    return true;
}

// one image into out[0 .. cap) -> status; *len = the bytes of the stream, 0 unless the status is MNY_JPEG_OK
static inline int encode(const int16_t* coef, int64_t coef_elems, const mny_jpeg_item& it, uint8_t* out, int64_t cap, int64_t* len, const Tables& T) {
    *len = 0;
    int status = check_item(it, coef_elems);
    if (status != MNY_JPEG_OK) return status;
    const Grid g = grid(it.h, it.w, it.hs, it.vs);
    Out o{out, cap, 0, 0, 0, false};
    header(o, it);
    const int16_t* base = coef + it.coef_off;
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < g.bh[1] && !o.over; ++my)
        for (int mx = 0; mx < g.bw[1] && !o.over; ++mx)
            for (int c = 0; c < 3; ++c) {
                const int ch = c == 0 ? it.hs : 1, cv = c == 0 ? it.vs : 1, t = c ? 1 : 0;
                int last = 0;
                for (int v = 0; v < cv; ++v)
                    for (int u = 0; u < ch; ++u) {
                        const int by = my * cv + v, bx = mx * ch + u;
                        const int16_t* blk = by < g.obh[c] && bx < g.obw[c] ? base + g.plane_off[c] + ((int64_t)by * g.bw[c] + bx) * 64 : nullptr;
                        if (blk) last = blk[0];
                        if (!block(o, T.dc[t], T.ac[t], blk, last, pred[c])) return MNY_JPEG_EHUFFMAN;
                    }
            }
    if (o.nacc) put(o, (1u << (8 - o.nacc)) - 1, 8 - o.nacc);
    byte(o, 0xFF);
    byte(o, 0xD9);
    if (o.over) return MNY_JPEG_ECAPACITY;
    *len = o.n;
    return MNY_JPEG_OK;
}

struct Job {
    const int16_t* coef;
    int64_t coef_elems;
    const mny_jpeg_item* items;
    int n;
    uint8_t* out;
    const int64_t* out_off;
    const int64_t* out_cap;
    int64_t* out_len;
    int32_t* status;
    int first, stride;
};

static inline void* worker(void* arg) {
    const Job& j = *(const Job*)arg;
    Tables T;
    build_all(T);
    for (int i = j.first; i < j.n; i += j.stride) {
        if (j.out_off[i] < 0 || j.out_cap[i] < 0) {
            j.out_len[i] = 0;
            j.status[i] = MNY_JPEG_ECAPACITY;
            continue;
        }
        j.status[i] = encode(j.coef, j.coef_elems, j.items[i], j.out + j.out_off[i], j.out_cap[i], &j.out_len[i], T);
    }
    return nullptr;
}

static inline void batch(const int16_t* coef, int64_t coef_elems, const mny_jpeg_item* items, int n, uint8_t* out, const int64_t* out_off,
                         const int64_t* out_cap, int64_t* out_len, int32_t* status, int n_threads) {
    int T = n_threads < 1 ? 1 : (n_threads > 16 ? 16 : n_threads);
    if (T > n) T = n;
    Job jobs[16];
    pthread_t tid[16];
    bool started[16] = {false};
    for (int t = 0; t < T; ++t) {
        jobs[t] = Job{coef, coef_elems, items, n, out, out_off, out_cap, out_len, status, t, T};
        if (t) started[t] = pthread_create(&tid[t], nullptr, worker, &jobs[t]) == 0;
    }
    worker(&jobs[0]);
    for (int t = 1; t < T; ++t) {
        if (started[t]) pthread_join(tid[t], nullptr);
        else worker(&jobs[t]);                                                    // no thread to be had: the caller does that share
    }
}

}  // namespace mny_jpegenc_host
