"""Writes tests/golden/jpegenc_cases.npz: seeded numpy images and the JPEG file Pillow writes for each with
Image.save(f, "JPEG", quality=q, subsampling=s).  Pillow only; no reference code.  The encoder tests compare the stored streams
byte for byte, so the pin survives a Pillow build whose libjpeg writes other bytes.

    python tools/gen_golden_jpegenc.py

Keys of the npz: `names`; per case `x_<name>` (the pixels, uint8 [h,w,3]) and `s_<name>` (Pillow's stream, uint8).  A name is
<sampling>_<h>x<w>_q<quality>_<content>."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
SAMPLING = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}
# (sampling, h, w, quality, content): heights 6, 8, 24 and 40 at 4:2:0 hold the rule for the rows below the last down-sampled one
CASES = [("420", 1, 1, 75, "noise"), ("420", 6, 6, 75, "smooth"), ("420", 8, 8, 90, "noise"), ("420", 24, 8, 75, "smooth"),
         ("420", 40, 8, 50, "noise"), ("420", 37, 53, 75, "smooth"), ("422", 3, 5, 95, "noise"), ("422", 9, 7, 5, "smooth"),
         ("422", 17, 33, 75, "smooth"), ("444", 5, 8, 100, "noise"), ("444", 16, 16, 50, "smooth"), ("444", 7, 8, 75, "noise")]


def image(rng, h, w, content):
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    low = Image.fromarray(rng.integers(0, 256, (h // 6 + 2, w // 6 + 2, 3), dtype=np.uint8))
    a = np.asarray(low.resize((w, h), Image.BICUBIC), np.float64) + rng.normal(0, 4.0, (h, w, 3))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20260611)
    arrays, names = {}, []
    for key, h, w, q, content in CASES:
        name = "%s_%dx%d_q%d_%s" % (key, h, w, q, content)
        x = image(rng, h, w, content)
        b = io.BytesIO()
        Image.fromarray(x).save(b, "JPEG", quality=q, subsampling=SAMPLING[key])
        names.append(name)
        arrays["x_" + name] = x
        arrays["s_" + name] = np.frombuffer(b.getvalue(), np.uint8)
    arrays["names"] = np.array(names)
    path = os.path.join(GOLDEN, "jpegenc_cases.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 40000
    print("jpegenc_cases.npz %d bytes, %d cases" % (os.path.getsize(path), len(names)))


if __name__ == "__main__":
    main()
