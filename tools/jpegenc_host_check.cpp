// Stand-alone check of the encoder's host half (csrc/jpegenc_host.h) under the address and undefined-behaviour sanitizers: random
// frames at every sampling, coefficient and output buffers sized exactly, coefficients inside and outside baseline's range, output
// capacities from nothing up to the worst case, 1 to 4 threads.  No GPU, no Python.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpegenc_host_check.cpp -o jpegenc_host_check
//     ./jpegenc_host_check
#include "../mobilenet-yolo-pytorch_amd/csrc/jpegenc_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
int main() {
    using namespace mny_jpegenc_host;
    srand(1);
    int fails = 0;
    for (int trial = 0; trial < 300; ++trial) {
        const int n = 1 + rand() % 5;
        std::vector<mny_image_desc> desc(n);
        for (auto& d : desc) { d.offset = 0; d.h = 1 + rand() % 70; d.w = 1 + rand() % 70; }
        const int hs = 1 + rand() % 2, vs = hs == 2 ? 1 + rand() % 2 : 1;
        std::vector<mny_jpeg_item> items(n);
        const int64_t total = enc_layout(desc.data(), n, 1 + rand() % 100, hs, vs, items.data());
        std::vector<int16_t> coef(total);      // exactly sized: ASan sees any read past it
        const int range = trial % 3 == 0 ? 4096 : (trial % 3 == 1 ? 64 : 2);
        for (auto& c : coef) c = (int16_t)(rand() % (2 * range + 1) - range);
        std::vector<int64_t> off(n), cap(n), len(n);
        std::vector<int32_t> st(n);
        int64_t o = 0;
        for (int i = 0; i < n; ++i) {
            off[i] = o;
            const int64_t blocks = ((int64_t)items[i].bw[0] * items[i].bh[0] + 2 * (int64_t)items[i].bw[1] * items[i].bh[1]);
            cap[i] = trial % 2 ? 700 + 420 * blocks : rand() % 3000;
            o += cap[i];
        }
        std::vector<uint8_t> out(o);           // exactly sized
        batch(coef.data(), total, items.data(), n, out.data(), off.data(), cap.data(), len.data(), st.data(), 1 + rand() % 4);
        for (int i = 0; i < n; ++i) {
            if (st[i] == MNY_JPEG_OK && (len[i] < 625 || len[i] > cap[i])) ++fails;
            if (trial % 2 && range <= 64 && st[i] != MNY_JPEG_OK) ++fails;   // the worst-case bound always fits
            if (st[i] != MNY_JPEG_OK && len[i] != 0) ++fails;
        }
    }
    printf("jpegenc_host_check: 300 batches, %d contract violations%s\n", fails, fails ? "" : ": clean");
    return fails != 0;
}
