"""Writes tests/golden/jpeg_cases.npz and tests/golden/voc_like.jpg: JPEG streams written by Pillow from seeded numpy images, and
Pillow's own decode of each (Image.open(...).convert("RGB")) as the expected pixels.  Pillow only; no reference code.

    python tools/gen_golden_jpeg.py                 # the two fixtures
    python tools/gen_golden_jpeg.py --dump DIR      # also every stream as DIR/<name>.jpg and DIR/manifest.txt, the input of
                                                    # tools/jpeg_host_check.cpp

Keys of the npz: `names`; per case `s_<name>` (the stream, uint8) and, where pixels are pinned, `p_<name>` (uint8 [h,w,3]) or,
for the cases of HASHED (restart intervals and optimised tables change the byte stream, not the pixels), `h_<name>`, their SHA-256.
  ok_*      streams the decoder takes: sampling x size, table variety, content
  route_*   streams it hands to the fallback (progressive, CMYK): the status is pinned, Pillow's RGB feeds the fallback test
  hostile_* the 37x53 4:2:0 stream truncated inside the headers, mid-scan and before EOI, and with one scan byte flipped
`voc_like_sha256`: SHA-256 of Pillow's RGB of voc_like.jpg (500x375, 4:2:0, quality 90)."""
import argparse
import hashlib
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
SIZES = [(1, 1), (3, 5), (4, 9), (8, 8), (9, 7), (16, 16), (17, 33), (37, 53)]            # w x h
HASHED = ("ok_rst_blocks", "ok_rst_rows", "ok_optimize", "ok_noise_q100")
SAMPLING = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}


def smooth(rng, w, h, cell=6, noise=6.0):
    """A colourful low-frequency field with a little noise: strong chroma gradients at every size."""
    gw, gh = max(2, w // cell + 2), max(2, h // cell + 2)
    low = Image.fromarray(rng.integers(0, 256, (gh, gw, 3), dtype=np.uint8))
    a = np.asarray(low.resize((w, h), Image.BICUBIC), np.float64) + rng.normal(0, noise, (h, w, 3))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def encode(arr, **kw):
    mode = "L" if arr.ndim == 2 else ("CMYK" if arr.shape[2] == 4 else "RGB")
    b = io.BytesIO()
    Image.fromarray(arr, mode).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow_rgb(stream):
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def scan_start(stream):
    """Offset of the first entropy-coded byte of a single-scan stream."""
    i = stream.index(b"\xff\xda")
    return i + 2 + ((stream[i + 2] << 8) | stream[i + 3])


def cases():
    rng = np.random.default_rng(20240531)
    out = {}
    for w, h in SIZES:
        img = smooth(rng, w, h)
        for key, sub in SAMPLING.items():
            out["ok_%s_%dx%d" % (key, w, h)] = encode(img, quality=90, subsampling=sub)
        out["ok_gray_%dx%d" % (w, h)] = encode(img[..., 1].copy(), quality=90)
    img = smooth(rng, 37, 53)
    out["ok_optimize"] = encode(img, quality=85, subsampling="4:2:0", optimize=True)
    out["ok_rst_blocks"] = encode(img, quality=85, subsampling="4:2:0", restart_marker_blocks=2)
    out["ok_rst_rows"] = encode(img, quality=85, subsampling="4:2:0", restart_marker_rows=1)
    qt = [[int(v) for v in rng.integers(1, 40, 64)], [int(v) for v in rng.integers(1, 90, 64)]]
    out["ok_qtables"] = encode(img, qtables=qt, subsampling="4:2:0")
    noise = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
    out["ok_noise_q100"] = encode(noise, quality=100, subsampling="4:2:0")
    out["ok_noise_q50"] = encode(noise, quality=50, subsampling="4:2:0")
    yy, xx = np.mgrid[0:32, 0:40]
    board = np.where(((yy + xx) % 2 == 0)[..., None], np.array([255, 0, 255], np.uint8), np.array([0, 255, 0], np.uint8)).astype(np.uint8)
    out["ok_checker_q5"] = encode(board, quality=5, subsampling="4:2:0")
    out["route_progressive"] = encode(img, quality=85, subsampling="4:2:0", progressive=True)
    out["route_cmyk"] = encode(np.concatenate([255 - img, rng.integers(0, 64, (53, 37, 1), dtype=np.uint8)], axis=2), quality=85)
    base = out["ok_420_37x53"]
    s0 = scan_start(base)
    mid = s0 + (len(base) - s0) // 2
    out["hostile_cut_headers"] = base[:s0 // 2]
    out["hostile_cut_scan"] = base[:mid]
    out["hostile_cut_eoi"] = base[:-2]
    flipped = bytearray(base)
    flipped[mid] ^= 0x5A
    out["hostile_flip"] = bytes(flipped)
    return out


def voc_like():
    rng = np.random.default_rng(7)
    return encode(smooth(rng, 500, 375, cell=40, noise=2.0), quality=90, subsampling="4:2:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="also write every stream as <dir>/<name>.jpg and <dir>/manifest.txt")
    args = ap.parse_args()
    streams = cases()
    voc = voc_like()
    assert len(voc) < 40000, len(voc)
    arrays = {"names": np.array(sorted(streams))}
    for name, s in streams.items():
        arrays["s_" + name] = np.frombuffer(s, np.uint8)
        if name in HASHED:
            arrays["h_" + name] = np.array(hashlib.sha256(pillow_rgb(s).tobytes()).hexdigest())
        elif not name.startswith("hostile_"):
            arrays["p_" + name] = pillow_rgb(s)
    arrays["voc_like_sha256"] = np.array(hashlib.sha256(pillow_rgb(voc).tobytes()).hexdigest())
    np.savez_compressed(os.path.join(GOLDEN, "jpeg_cases.npz"), **arrays)
    with open(os.path.join(GOLDEN, "voc_like.jpg"), "wb") as f:
        f.write(voc)
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_cases.npz")) + len(voc) < 150000
    print("jpeg_cases.npz %d bytes, voc_like.jpg %d bytes, %d cases" % (os.path.getsize(os.path.join(GOLDEN, "jpeg_cases.npz")), len(voc), len(streams)))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        with open(os.path.join(args.dump, "manifest.txt"), "w") as m:
            for name in sorted(streams):
                with open(os.path.join(args.dump, name + ".jpg"), "wb") as f:
                    f.write(streams[name])
                m.write(name + "\n")
            with open(os.path.join(args.dump, "voc_like.jpg"), "wb") as f:
                f.write(voc)
            m.write("voc_like\n")


if __name__ == "__main__":
    main()
