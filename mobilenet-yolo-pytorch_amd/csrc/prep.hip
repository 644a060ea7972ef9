// Device-side batch input preparation (include/mnyolo.h: mny_prep_batch).
// Replaces the image half of folder2lmdb.py:223-256 (collate_fn): per image transforms.Resize(size, BILINEAR) on the decoded
// PIL image (= Pillow's ImagingResample: antialiased triangle filter, 22-bit fixed-point taps, horizontal pass then vertical
// pass, each rounded to uint8), ToTensor (/255), Normalize ((x-mean)/std), stack — for a whole batch of differently sized
// RGB uint8 images in three launches, writing the NCHW fp32 batch the stem kernel reads.  The kernels live in prep_kernels.h
// (shared with mny_prep_tiles, slice.hip); here every window is a whole dense image.
// Integer work: bit-exact against Pillow.  Compiled with -ffp-contract=off (the taps must round like the host library's).
#include "prep_kernels.h"

using namespace mny;

extern "C" size_t mny_prep_ws_bytes(int N, int max_in_h, int max_in_w, int out_h, int out_w) {
    if (N < 1 || max_in_h < 1 || max_in_w < 1 || out_h < 1 || out_w < 1) return 0;
    return make_layout(N, max_in_h, max_in_w, out_h, out_w).total;
}

extern "C" int mny_prep_batch(const uint8_t* src, const mny_image_desc* desc, int N, int max_in_h, int max_in_w, int out_h, int out_w, const float* mean3,
                              const float* std3, float* out, void* ws, void* stream) {
    MNY_REQUIRE(src && desc && mean3 && std3 && out && ws, "mny_prep_batch: null pointer");
    MNY_REQUIRE(N >= 1 && max_in_h >= 1 && max_in_w >= 1 && out_h >= 1 && out_w >= 1, "mny_prep_batch: bad sizes N=%d in<=%dx%d out=%dx%d", N, max_in_h,
                max_in_w, out_h, out_w);
    MNY_REQUIRE((int64_t)max_in_h * out_w < ((int64_t)1 << 31) / 3 && N <= 65535, "mny_prep_batch: image too large / batch > 65535");
    MNY_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "mny_prep_batch: std must be non-zero");
    return prep_launch<mny_image_desc>("mny_prep_batch", src, desc, N, max_in_h, max_in_w, out_h, out_w, mean3, std3, out, ws, (hipStream_t)stream);
}
