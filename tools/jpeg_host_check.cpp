// Stand-alone memory-safety check of the JPEG host stage (csrc/jpeg_host.h): no HIP, no Python.  Build it with the address
// and undefined-behaviour sanitizers and run it on the streams that tools/gen_golden_jpeg.py --dump DIR writes:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_host_check.cpp -o jpeg_host_check
//     ./jpeg_host_check DIR
// Every stream is copied into a heap block of exactly its length and every coefficient slice is a heap block of exactly its
// capacity, so a read past `len` or a write outside the slice is a sanitizer report.  It runs
//   every prefix length of the 37x53 4:2:0 stream,
//   4000 seeded single-byte corruptions of it and 300 of voc_like.jpg,
//   every case of the manifest in one batch at 1 and at 4 threads (the two outputs must be equal),
// and exits 0 when nothing was reported.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../mobilenet-yolo-pytorch_amd/csrc/jpeg_host.h"

namespace jh = mny_jpeg_host;
typedef std::vector<uint8_t> Bytes;

static bool read_file(const std::string& path, Bytes& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t n;
    out.clear();
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

// decode one stream from exact-size heap blocks -> status
static int run_one(const uint8_t* src, int64_t len, int64_t cap) {
    uint8_t* d = (uint8_t*)malloc(len ? len : 1);
    memcpy(d, src, len);
    int16_t* coef = (int16_t*)malloc(cap ? cap * sizeof(int16_t) : 1);
    mny_jpeg_info info;
    jh::probe(d, len, &info);
    mny_jpeg_item item;
    const uint8_t* dp = d;
    const int64_t off = 0;
    jh::batch(&dp, &len, 1, coef, &off, &cap, &item, 1);
    const int status = item.status;
    if (info.status != MNY_JPEG_OK && status != info.status) {   // what the probe refuses, the decoder refuses for the same reason
        fprintf(stderr, "probe and decode disagree: %d vs %d\n", info.status, status);
        exit(2);
    }
    free(coef);
    free(d);
    return status;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static int64_t capacity_of(const Bytes& s) {
    mny_jpeg_info info;
    jh::probe(s.data(), (int64_t)s.size(), &info);
    return info.status == MNY_JPEG_OK ? info.n_coef : 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DIR (written by tools/gen_golden_jpeg.py --dump DIR)\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    {
        Bytes m;
        if (!read_file(dir + "/manifest.txt", m)) { fprintf(stderr, "no manifest in %s\n", dir.c_str()); return 2; }
        std::string cur;
        for (uint8_t c : m) {
            if (c == '\n') { if (!cur.empty()) names.push_back(cur); cur.clear(); } else cur.push_back((char)c);
        }
    }
    std::vector<Bytes> streams(names.size());
    int base = -1, voc = -1;
    for (size_t i = 0; i < names.size(); ++i) {
        if (!read_file(dir + "/" + names[i] + ".jpg", streams[i])) { fprintf(stderr, "cannot read %s\n", names[i].c_str()); return 2; }
        if (names[i] == "ok_420_37x53") base = (int)i;
        if (names[i] == "voc_like") voc = (int)i;
    }
    if (base < 0 || voc < 0) { fprintf(stderr, "the manifest lacks ok_420_37x53 or voc_like\n"); return 2; }

    // 1. every prefix
    const Bytes& B = streams[base];
    const int64_t cap = capacity_of(B);
    int hist[16] = {0};
    for (size_t len = 0; len <= B.size(); ++len) hist[run_one(B.data(), (int64_t)len, cap) & 15]++;
    if (run_one(B.data(), (int64_t)B.size(), cap) != MNY_JPEG_OK) { fprintf(stderr, "the whole stream does not decode\n"); return 1; }
    if (run_one(B.data(), (int64_t)B.size(), cap - 64) != MNY_JPEG_ECAPACITY) { fprintf(stderr, "a short slice was not refused\n"); return 1; }

    // 2. single-byte corruptions
    int corrupt_ok = 0;
    for (int k = 0; k < 4300; ++k) {
        const Bytes& S = k < 4000 ? B : streams[voc];
        Bytes c = S;
        c[rnd() % c.size()] ^= (uint8_t)(1 + rnd() % 255);
        corrupt_ok += run_one(c.data(), (int64_t)c.size(), capacity_of(S)) == MNY_JPEG_OK;
    }

    // 3. the whole manifest as one batch, 1 thread and 4 threads
    const int n = (int)streams.size();
    std::vector<const uint8_t*> ptr(n);
    std::vector<int64_t> len(n), off(n), cp(n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        ptr[i] = streams[i].data();
        len[i] = (int64_t)streams[i].size();
        off[i] = total;
        cp[i] = capacity_of(streams[i]);
        total += cp[i];
    }
    std::vector<int16_t> c1(total, 0), c4(total, 0);
    std::vector<mny_jpeg_item> i1(n), i4(n);
    jh::batch(ptr.data(), len.data(), n, c1.data(), off.data(), cp.data(), i1.data(), 1);
    jh::batch(ptr.data(), len.data(), n, c4.data(), off.data(), cp.data(), i4.data(), 4);
    if (memcmp(c1.data(), c4.data(), total * sizeof(int16_t)) != 0 || memcmp(i1.data(), i4.data(), n * sizeof(mny_jpeg_item)) != 0) {
        fprintf(stderr, "1 thread and 4 threads disagree\n");
        return 1;
    }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        const bool want_ok = names[i].compare(0, 3, "ok_") == 0 || names[i] == "voc_like";
        if (want_ok && i1[i].status != MNY_JPEG_OK) { fprintf(stderr, "%s: status %d\n", names[i].c_str(), i1[i].status); return 1; }
        ok += i1[i].status == MNY_JPEG_OK;
    }
    printf("jpeg_host_check: %zu prefixes (%d decode), 4300 corruptions (%d still decode), %d streams x {1,4} threads (%d ok): clean\n", B.size() + 1,
           hist[0], corrupt_ok, n, ok);
    return 0;
}
