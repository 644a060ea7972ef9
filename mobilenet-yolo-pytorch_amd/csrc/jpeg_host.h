// Host half of the baseline JPEG decoder (include/mnyolo.h: mny_jpeg_probe, mny_jpeg_entropy_batch): marker parsing and
// Huffman decoding into quantised DCT coefficients, the serial and branchy part of a decode.  Plain C++17: no HIP, no
// common.h, so a stand-alone program can compile it (tools/jpeg_host_check.cpp does, under the address and undefined-behaviour
// sanitizers).  csrc/jpeg.hip exports the two entry points; everything here has internal linkage.
//   parse()   : SOI .. SOS.  Every read is bounded by `len`; a stream this decoder does not take leaves with a status of
//               its own (MNY_JPEG_*), with h and w filled in when a frame header was seen.
//   decode()  : the one interleaved scan.  A 64-bit bit buffer is refilled a byte at a time (FF 00 unstuffed, fill bytes
//               skipped, a marker or the end of the data feeds zero bits that are counted: an MCU that consumed one of
//               them is an error), codes up to 9 bits resolve in one table look-up, longer ones by the maxcode walk of
//               the standard.  Blocks are written de-zigzagged, plane after plane, row-major over the padded block grid.
//   batch()   : images are dealt to pthreads by index (image i goes to thread i mod T), so the output is independent of
//               timing; each thread owns its Huffman tables on its stack and allocates nothing.
#pragma once
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mnyolo.h"

namespace mny_jpeg_host {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const int kMaxSide = 16383;   // what the stages behind the decoder address
static const int kLook = 9;          // bits of the one-step Huffman table

struct HuffSpec {
    uint8_t bits[17];   // bits[l] = number of codes of length l
    uint8_t vals[256];
    bool set;
};

struct Header {
    int h, w, ncomp;
    int hs[3], vs[3], tq[3], cid[3], td[3], ta[3];
    uint16_t q[4][64];   // natural order
    bool qset[4];
    HuffSpec dc[4], ac[4];
    int restart;
    bool sof, jfif, adobe;
    int adobe_tf;
    int64_t scan_pos;   // first byte of entropy-coded data
};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// the geometry of a supported frame: luma sampling, blocks per row and column of each padded plane, coefficients in all
static inline void geometry(const Header& H, mny_jpeg_info* info) {
    const int hmax = H.ncomp == 1 ? 1 : H.hs[0], vmax = H.ncomp == 1 ? 1 : H.vs[0];
    const int mcux = (H.w + 8 * hmax - 1) / (8 * hmax), mcuy = (H.h + 8 * vmax - 1) / (8 * vmax);
    info->hs = hmax;
    info->vs = vmax;
    int64_t total = 0;
    for (int c = 0; c < 3; ++c) {
        const bool live = c < H.ncomp;
        info->bw[c] = live ? mcux * (c == 0 ? hmax : 1) : 0;
        info->bh[c] = live ? mcuy * (c == 0 ? vmax : 1) : 0;
        total += (int64_t)info->bw[c] * info->bh[c] * 64;
    }
    info->n_coef = total;
}

// SOI .. SOS.  -> MNY_JPEG_* status; H.h / H.w / H.ncomp are valid whenever H.sof is set.
static inline int parse(const uint8_t* d, int64_t len, Header& H) {
    memset(&H, 0, sizeof(H));
    if (len < 2) return len <= 0 || d[0] == 0xFF ? MNY_JPEG_ETRUNCATED : MNY_JPEG_ENOTJPEG;
    if (d[0] != 0xFF || d[1] != 0xD8) return MNY_JPEG_ENOTJPEG;
    int64_t pos = 2;
    int pending = 0;   // the status of an unsupported frame type, reported once its sizes are known
    for (;;) {
        if (pos >= len) return MNY_JPEG_ETRUNCATED;
        if (d[pos] != 0xFF) return MNY_JPEG_EMARKER;
        while (pos < len && d[pos] == 0xFF) ++pos;
        if (pos >= len) return MNY_JPEG_ETRUNCATED;
        const int m = d[pos++];
        if (m == 0x01) continue;                                                  // TEM stands alone
        if (m == 0x00 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return MNY_JPEG_EMARKER;
        if (pos + 2 > len) return MNY_JPEG_ETRUNCATED;
        const int L = be16(d + pos);
        if (L < 2) return MNY_JPEG_EHEADER;
        if (pos + L > len) return MNY_JPEG_ETRUNCATED;
        const uint8_t* s = d + pos + 2;
        int n = L - 2;
        pos += L;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {      // SOFn
            if (H.sof) return MNY_JPEG_EMARKER;
            if (n < 6) return MNY_JPEG_EHEADER;
            const int P = s[0], nc = s[5];
            H.h = be16(s + 1);
            H.w = be16(s + 3);
            if (n != 6 + 3 * nc) return MNY_JPEG_EHEADER;
            if (H.h == 0 || H.w == 0) { H.h = H.w = 0; return MNY_JPEG_EHEADER; }
            H.sof = true;
            H.ncomp = nc;
            if (m == 0xC2) return MNY_JPEG_EPROGRESSIVE;
            if (m == 0xC1) return MNY_JPEG_EEXTENDED;
            if (m != 0xC0) return MNY_JPEG_EARITHMETIC;                           // lossless, differential and arithmetic frames
            if (P != 8) return MNY_JPEG_EPRECISION;
            if (nc != 1 && nc != 3) return MNY_JPEG_ECOLORSPACE;
            for (int c = 0; c < nc; ++c) {
                H.cid[c] = s[6 + 3 * c];
                H.hs[c] = s[7 + 3 * c] >> 4;
                H.vs[c] = s[7 + 3 * c] & 15;
                H.tq[c] = s[8 + 3 * c];
                if (H.hs[c] < 1 || H.hs[c] > 4 || H.vs[c] < 1 || H.vs[c] > 4 || H.tq[c] > 3) return MNY_JPEG_EHEADER;
            }
            if (nc == 3) {
                const bool chroma1 = H.hs[1] == 1 && H.vs[1] == 1 && H.hs[2] == 1 && H.vs[2] == 1;
                const bool luma = (H.hs[0] == 1 || H.hs[0] == 2) && H.vs[0] <= H.hs[0];   // 1x1, 2x1, 2x2
                if (!chroma1 || !luma) pending = MNY_JPEG_ESAMPLING;
            }
            if (!pending && (H.h > kMaxSide || H.w > kMaxSide)) pending = MNY_JPEG_ETOOLARGE;
        } else if (m == 0xDB) {                                                   // DQT
            while (n > 0) {
                const int pq = s[0] >> 4, t = s[0] & 15;
                if (t > 3 || pq > 1) return MNY_JPEG_EHEADER;
                if (pq == 1) return MNY_JPEG_EPRECISION;
                if (n < 65) return MNY_JPEG_EHEADER;
                for (int k = 0; k < 64; ++k) H.q[t][kZigzag[k]] = s[1 + k];
                H.qset[t] = true;
                s += 65;
                n -= 65;
            }
        } else if (m == 0xC4) {                                                   // DHT
            while (n > 0) {
                if (n < 17) return MNY_JPEG_EHEADER;
                const int tc = s[0] >> 4, t = s[0] & 15;
                if (tc > 1 || t > 3) return MNY_JPEG_EHEADER;
                int count = 0;
                for (int l = 1; l <= 16; ++l) count += s[l];
                if (count > 256 || n < 17 + count) return MNY_JPEG_EHEADER;
                HuffSpec& T = tc ? H.ac[t] : H.dc[t];
                T.bits[0] = 0;
                memcpy(T.bits + 1, s + 1, 16);
                memset(T.vals, 0, sizeof(T.vals));
                memcpy(T.vals, s + 17, count);
                T.set = true;
                s += 17 + count;
                n -= 17 + count;
            }
        } else if (m == 0xCC) {                                                   // DAC: arithmetic conditioning
            return MNY_JPEG_EARITHMETIC;
        } else if (m == 0xDD) {                                                   // DRI
            if (n != 2) return MNY_JPEG_EHEADER;
            H.restart = be16(s);
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) H.jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { H.adobe = true; H.adobe_tf = s[11]; }
        } else if (m == 0xDA) {                                                   // SOS
            if (!H.sof) return MNY_JPEG_EMARKER;
            if (pending) return pending;
            if (n < 1) return MNY_JPEG_EHEADER;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return MNY_JPEG_EHEADER;
            if (ns != H.ncomp) return MNY_JPEG_EMULTISCAN;
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != H.cid[c]) return MNY_JPEG_EHEADER;
                H.td[c] = s[2 + 2 * c] >> 4;
                H.ta[c] = s[2 + 2 * c] & 15;
                if (H.td[c] > 3 || H.ta[c] > 3) return MNY_JPEG_EHEADER;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MNY_JPEG_EHEADER;
            if (H.ncomp == 3) {                                                   // libjpeg's guess of the colour space
                if (!H.jfif && H.adobe && H.adobe_tf != 1) return MNY_JPEG_ECOLORSPACE;
                if (!H.jfif && !H.adobe && H.cid[0] == 'R' && H.cid[1] == 'G' && H.cid[2] == 'B') return MNY_JPEG_ECOLORSPACE;
            }
            for (int c = 0; c < ns; ++c)
                if (!H.qset[H.tq[c]] || !H.dc[H.td[c]].set || !H.ac[H.ta[c]].set) return MNY_JPEG_EMARKER;   // a table segment is missing
            H.scan_pos = pos;
            return MNY_JPEG_OK;
        }
        // every other segment (APPn, COM, DNL, ...) is skipped by its length
    }
}

struct HuffDec {
    uint16_t look[1 << kLook];   // (length << 8) | symbol, 0 = longer than kLook bits
    int32_t maxcode[18];         // -1: no code of this length
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
};

static inline bool build(const HuffSpec& S, HuffDec& D) {
    memset(D.look, 0, sizeof(D.look));
    memcpy(D.vals, S.vals, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        D.valptr[l] = k;
        D.mincode[l] = code;
        const int cnt = S.bits[l];
        if (code + cnt > (1 << l)) return false;                                  // more codes than the length holds
        if (l <= kLook)
            for (int i = 0; i < cnt; ++i) {
                const int first = (code + i) << (kLook - l);
                for (int j = 0; j < (1 << (kLook - l)); ++j) D.look[first + j] = (uint16_t)((l << 8) | S.vals[k + i]);
            }
        k += cnt;
        code += cnt;
        D.maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    D.maxcode[17] = 0x7fffffff;
    return true;
}

struct Bits {
    const uint8_t* d;
    int64_t len, pos;
    uint64_t buf;   // the low n bits are valid, the next bit of the stream is the highest of them
    int n;
    int fake;       // how many of the newest bits in buf are zeros invented after a marker or the end of the data
    bool marker;    // pos stands on the FF of a marker
};

static inline void fill(Bits& b) {
    while (b.n <= 56) {
        int c = 0;
        if (!b.marker && b.pos < b.len) {
            c = b.d[b.pos];
            if (c != 0xFF) {
                ++b.pos;
            } else {
                int64_t p = b.pos + 1;
                while (p < b.len && b.d[p] == 0xFF) ++p;                          // fill bytes
                if (p < b.len && b.d[p] == 0x00) {
                    b.pos = p + 1;                                                // FF 00: a data byte FF
                } else if (p >= b.len) {
                    b.pos = b.len;                                                // the data ends inside a marker
                    c = -1;
                } else {
                    b.marker = true;
                    c = -1;
                }
            }
        } else {
            c = -1;
        }
        if (c < 0) {
            c = 0;
            b.fake = b.fake < 4096 ? b.fake + 8 : b.fake;
        }
        b.buf = (b.buf << 8) | (uint64_t)c;
        b.n += 8;
    }
}

static inline int peek(const Bits& b, int k) { return (int)((b.buf >> (b.n - k)) & ((1u << k) - 1)); }

// -> symbol, or -1 for a code that is not in the table.  At least 16 bits are in the buffer.
static inline int symbol(Bits& b, const HuffDec& D) {
    const int e = D.look[peek(b, kLook)];
    if (e) {
        b.n -= e >> 8;
        return e & 255;
    }
    for (int l = kLook + 1; l <= 16; ++l) {
        const int code = peek(b, l);
        if (code <= D.maxcode[l]) {
            if (code < D.mincode[l]) return -1;
            b.n -= l;
            return D.vals[(D.valptr[l] + code - D.mincode[l]) & 255];
        }
    }
    return -1;
}

static inline int extend(Bits& b, int s) {   // s in 1..15
    const int v = peek(b, s);
    b.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// one block into blk[64] (natural order).  -> MNY_JPEG_OK or MNY_JPEG_EHUFFMAN
static inline int block(Bits& b, const HuffDec& dc, const HuffDec& ac, int& pred, int16_t* blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    fill(b);
    int s = symbol(b, dc);
    if (s < 0 || s > 15) return MNY_JPEG_EHUFFMAN;
    if (s) pred = sat16(pred + extend(b, s));
    blk[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
        fill(b);
        const int rs = symbol(b, ac);
        if (rs < 0) return MNY_JPEG_EHUFFMAN;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                                                   // EOB
            k += 16;
            if (k > 63) return MNY_JPEG_EHUFFMAN;                                 // a run past coefficient 63
            continue;
        }
        k += r;
        if (k > 63) return MNY_JPEG_EHUFFMAN;
        blk[kZigzag[k]] = (int16_t)extend(b, s);
        ++k;
    }
    return MNY_JPEG_OK;
}

struct Tables {
    HuffDec dc[4], ac[4];
};

static inline void fill_item(const Header& H, const mny_jpeg_info& info, int status, int64_t coef_off, mny_jpeg_item* it) {
    memset(it, 0, sizeof(*it));
    it->status = status;
    it->h = H.sof ? H.h : 0;
    it->w = H.sof ? H.w : 0;
    it->ncomp = H.sof ? H.ncomp : 0;
    it->coef_off = coef_off;
    if (status != MNY_JPEG_OK) return;
    it->hs = info.hs;
    it->vs = info.vs;
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        it->bw[c] = info.bw[c];
        it->bh[c] = info.bh[c];
        it->plane_off[c] = off;
        off += (int64_t)info.bw[c] * info.bh[c] * 64;
        if (c < H.ncomp) memcpy(it->q[c], H.q[H.tq[c]], sizeof(it->q[c]));
    }
    it->n_coef = info.n_coef;
}

static inline void probe(const uint8_t* d, int64_t len, mny_jpeg_info* info) {
    Header H;
    memset(info, 0, sizeof(*info));
    info->status = parse(d, len, H);
    if (H.sof) {
        info->h = H.h;
        info->w = H.w;
        info->ncomp = H.ncomp;
    }
    if (info->status == MNY_JPEG_OK) geometry(H, info);
}

// one image: coefficients into coef[0 .. cap), its record into *it.  Never reads d[len..], never writes coef[cap..].
static inline void decode(const uint8_t* d, int64_t len, int16_t* coef, int64_t coef_off, int64_t cap, mny_jpeg_item* it, Tables& T) {
    Header H;
    mny_jpeg_info info;
    memset(&info, 0, sizeof(info));
    int status = parse(d, len, H);
    if (status == MNY_JPEG_OK) {
        geometry(H, &info);
        if (info.n_coef > cap) status = MNY_JPEG_ECAPACITY;
    }
    if (status == MNY_JPEG_OK) {
        bool dc_built[4] = {false, false, false, false}, ac_built[4] = {false, false, false, false};
        for (int c = 0; c < H.ncomp && status == MNY_JPEG_OK; ++c) {
            if (!dc_built[H.td[c]] && !build(H.dc[H.td[c]], T.dc[H.td[c]])) status = MNY_JPEG_EHUFFMAN;
            dc_built[H.td[c]] = true;
            if (!ac_built[H.ta[c]] && !build(H.ac[H.ta[c]], T.ac[H.ta[c]])) status = MNY_JPEG_EHUFFMAN;
            ac_built[H.ta[c]] = true;
        }
    }
    if (status == MNY_JPEG_OK) {
        Bits b;
        b.d = d; b.len = len; b.pos = H.scan_pos; b.buf = 0; b.n = 0; b.fake = 0; b.marker = false;
        const int mcux = info.bw[0] / info.hs, mcuy = info.bh[0] / info.vs;
        int64_t plane[3], off = 0;
        for (int c = 0; c < 3; ++c) {
            plane[c] = off;
            off += (int64_t)info.bw[c] * info.bh[c] * 64;
        }
        int pred[3] = {0, 0, 0};
        int64_t done = 0;
        int next_rst = 0;
        for (int my = 0; my < mcuy && status == MNY_JPEG_OK; ++my) {
            for (int mx = 0; mx < mcux && status == MNY_JPEG_OK; ++mx, ++done) {
                if (H.restart && done && done % H.restart == 0) {                 // RSTn: byte-align, reset the predictors
                    b.buf = 0; b.n = 0; b.fake = 0;
                    int64_t p = b.pos;
                    if (p >= len) { status = MNY_JPEG_ETRUNCATED; break; }
                    if (d[p] != 0xFF) { status = MNY_JPEG_EMARKER; break; }
                    while (p < len && d[p] == 0xFF) ++p;
                    if (p >= len) { status = MNY_JPEG_ETRUNCATED; break; }
                    if (d[p] != 0xD0 + next_rst) { status = MNY_JPEG_EMARKER; break; }
                    next_rst = (next_rst + 1) & 7;
                    b.pos = p + 1;
                    b.marker = false;
                    pred[0] = pred[1] = pred[2] = 0;
                }
                for (int c = 0; c < H.ncomp && status == MNY_JPEG_OK; ++c) {
                    const int ch = c == 0 ? info.hs : 1, cv = c == 0 ? info.vs : 1;
                    for (int v = 0; v < cv && status == MNY_JPEG_OK; ++v)
                        for (int u = 0; u < ch && status == MNY_JPEG_OK; ++u) {
                            const int64_t blk = (int64_t)(my * cv + v) * info.bw[c] + (mx * ch + u);
                            status = block(b, T.dc[H.td[c]], T.ac[H.ta[c]], pred[c], coef + plane[c] + blk * 64);
                        }
                }
                if (status == MNY_JPEG_OK && b.n < b.fake)                        // the MCU used bits that are not in the stream
                    status = b.marker ? MNY_JPEG_EMARKER : MNY_JPEG_ETRUNCATED;
            }
        }
    }
    fill_item(H, info, status, coef_off, it);
}

struct Job {
    const uint8_t* const* data;
    const int64_t* len;
    int n;
    int16_t* coef;
    const int64_t* coef_off;
    const int64_t* coef_cap;
    mny_jpeg_item* items;
    int first, stride;
};

static inline void* worker(void* arg) {
    const Job& j = *(const Job*)arg;
    Tables T;
    for (int i = j.first; i < j.n; i += j.stride) {
        const bool args_ok = j.data[i] && j.len[i] >= 0 && j.coef_off[i] >= 0 && j.coef_cap[i] >= 0;
        if (args_ok) {
            decode(j.data[i], j.len[i], j.coef + j.coef_off[i], j.coef_off[i], j.coef_cap[i], &j.items[i], T);
        } else {
            memset(&j.items[i], 0, sizeof(mny_jpeg_item));
            j.items[i].status = MNY_JPEG_ECAPACITY;
        }
    }
    return nullptr;
}

static inline void batch(const uint8_t* const* data, const int64_t* len, int n, int16_t* coef, const int64_t* coef_off, const int64_t* coef_cap,
                         mny_jpeg_item* items, int n_threads) {
    int T = n_threads < 1 ? 1 : (n_threads > 16 ? 16 : n_threads);
    if (T > n) T = n;
    Job jobs[16];
    pthread_t tid[16];
    bool started[16] = {false};
    for (int t = 0; t < T; ++t) {
        jobs[t] = Job{data, len, n, coef, coef_off, coef_cap, items, t, T};
        if (t) started[t] = pthread_create(&tid[t], nullptr, worker, &jobs[t]) == 0;
    }
    worker(&jobs[0]);
    for (int t = 1; t < T; ++t) {
        if (started[t]) pthread_join(tid[t], nullptr);
        else worker(&jobs[t]);                                                    // no thread to be had: the caller does that share
    }
}

}  // namespace mny_jpeg_host
