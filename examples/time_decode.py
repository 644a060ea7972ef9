#!/usr/bin/env python3
"""Times the JPEG decoder (jpeg.JpegDecoder: host entropy stage, one upload of coefficients, two HIP launches) against the path
it replaces: Pillow decode on a 16-thread pool, BatchPrep.pack, one upload of RGB.

    python examples/time_decode.py [--batch 256] [--rounds 5] [--warmup 2] [--threads 8]

The batch is `--batch` copies of tests/golden/voc_like.jpg (500x375, 4:2:0, quality 90).  The streams are IDENTICAL, so the
host stage's branches and tables repeat from image to image and the figures are data-independent except for cache effects; a
real batch will be somewhat slower on the host.  Every figure is the median of `rounds` windows after `warmup` unrecorded ones,
the variants taking turns inside a round.  Host figures are wall-clock; `h2d_us` and `kernels_us` are HIP-event times; the
end-to-end figures are wall-clock around the call plus a device synchronise.  Prints one JSON line.
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mobilenet_yolo_pytorch_amd import _lib, jpeg, prep  # noqa: E402


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3          # milliseconds


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_decode.py needs the MI355X"
    dev = torch.device("cuda:0")
    stream = open(os.path.join(ROOT, "tests", "golden", "voc_like.jpg"), "rb").read()
    batch = [stream] * a.batch
    dec = jpeg.JpegDecoder(device=dev, threads=a.threads)

    # the pieces, on buffers that stay put
    items, used, coef_elems = dec.host_stage(batch)
    assert (items["status"] == 0).all()
    n = a.batch
    desc = np.zeros(n, prep.DESC)
    off = 0
    for i in range(n):
        desc[i] = (off, items[i]["h"], items[i]["w"])
        off += (3 * int(items[i]["h"]) * int(items[i]["w"]) + 15) // 16 * 16
    stage_dev = dec._stage[:used].to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    dst = torch.empty(off, dtype=torch.uint8, device=dev)
    ws = torch.empty(_lib.query("mny_jpeg_ws_bytes", n, coef_elems), dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    base = stage_dev.data_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def kernels():
        _lib.call("mny_jpeg_pixels_batch", ctypes.c_void_p(base + n * jpeg.ITEM.itemsize), ctypes.c_void_p(base), n, p(dst), p(d_dev), 375, 500, p(ws), st)

    def end_to_end():
        dec(batch)
        torch.cuda.synchronize()

    variants = {"host_ms@1": lambda: wall(lambda: dec.host_stage(batch, threads=1)),
                "host_ms@8": lambda: wall(lambda: dec.host_stage(batch, threads=8)),
                "host_ms@16": lambda: wall(lambda: dec.host_stage(batch, threads=16)),
                "h2d_us": lambda: events(lambda: dec._stage[:used].to(dev, non_blocking=True)),
                "kernels_us": lambda: events(kernels),
                "decoder_ms": lambda: wall(end_to_end)}
    have_pillow = True
    try:
        from PIL import Image
    except ImportError:
        have_pillow = False
    if have_pillow:
        pool = ThreadPoolExecutor(16)
        packer = prep.BatchPrep([(352, 352)], [0, 0, 0], [1, 1, 1], device=dev)
        one = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))

        def pillow_path():
            stage, _, _, _ = packer.pack(list(pool.map(one, batch)))
            stage.to(dev, non_blocking=True)
            torch.cuda.synchronize()
        variants["pillow16_ms"] = lambda: wall(pillow_path)
        variants["pillow_decode_1thread_ms"] = lambda: wall(lambda: [one(b) for b in batch])

    times = {k: [] for k in variants}
    for r in range(a.warmup + a.rounds):
        for k, fn in variants.items():
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"batch": n, "image": "500x375 4:2:0 q90, %d bytes, identical streams" % len(stream), "rounds": a.rounds, "warmup": a.warmup,
           "threads": dec.threads, "upload_bytes": used, "rgb_bytes": off,
           "host_us_per_image_per_thread": round(med["host_ms@1"] * 1e3 / n, 1),
           "host_ms": {t: round(med["host_ms@%s" % t], 2) for t in ("1", "8", "16")},
           "h2d_us": round(med["h2d_us"], 1), "kernels_us": round(med["kernels_us"], 1),
           "decoder_images_per_s": round(n / med["decoder_ms"] * 1e3), "decoder_ms": round(med["decoder_ms"], 2)}
    if have_pillow:
        res["pillow16_images_per_s"] = round(n / med["pillow16_ms"] * 1e3)
        res["pillow16_ms"] = round(med["pillow16_ms"], 2)
        res["pillow_us_per_image_per_thread"] = round(med["pillow_decode_1thread_ms"] * 1e3 / n, 1)
        res["decoder_over_pillow16"] = round(med["pillow16_ms"] / med["decoder_ms"], 3)
    res["spread_pct"] = {k: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
