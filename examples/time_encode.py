#!/usr/bin/env python3
"""Times the way out of the device pipeline: the JPEG encoder (mny_jpeg_coef_batch, the copy of the coefficients, the threaded
mny_jpeg_huffman_batch, and jpeg.JpegEncoder end to end) against Pillow's Image.save on a 16-thread pool fed the same pixels
from host memory, and the annotation kernel (mny_viz_compose).

    python examples/time_encode.py [--batch 256] [--rounds 7] [--warmup 2] [--reps 50]

Encode: `--batch` VOC-sized RGB photos (375x500, synthetic.photos), 4:2:0, quality 75, already packed on the device.
`coef_kernel_us` is the HIP-event time of `--reps` back-to-back launches divided by `--reps`; `copy_ms` (coefficients to pageable
host memory, synchronised), `huffman_ms` (the host stage at 16 threads) and `end_to_end_ms` (JpegEncoder.__call__: layout, launch,
copy, host stage, the list of bytes) are wall-clock.  The Pillow figure is wall-clock around save() of every image into BytesIO on
the pool; it does not include bringing the pixels down from the device, which that path would need first (`download_ms`).
Compose: 64 images of 352x352 from a normalised fp32 batch, 300 detection rows each, thickness 2; HIP-event time as above, `gbps`
counting the fp32 read plus the uint8 write.  Every figure is the median of `rounds` windows after `warmup` unrecorded ones, the
variants taking turns inside a round.  Prints one JSON line."""
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
from mobilenet_yolo_pytorch_amd import _lib, jpeg, prep, synthetic, viz  # noqa: E402


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3          # milliseconds


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps           # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_encode.py needs the MI355X"
    dev = torch.device("cuda:0")
    n, h, w = a.batch, 375, 500
    distinct = synthetic.photos([(h, w)] * min(n, 32), seed=0)
    photos = [distinct[i % len(distinct)] for i in range(n)]
    stage, desc, _, _ = prep.BatchPrep([(352, 352)], [0, 0, 0], [1, 1, 1], device=dev).pack(photos)
    src = stage.to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    enc = jpeg.JpegEncoder(quality=75, subsampling="4:2:0", device=dev, threads=16)
    items, total = jpeg.enc_layout(desc, 75, "4:2:0")
    coef = torch.empty(total, dtype=torch.int16, device=dev)
    ws = torch.empty(_lib.query("mny_jpeg_enc_ws_bytes", n), dtype=torch.uint8, device=dev)
    i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    kernel = lambda: _lib.call("mny_jpeg_coef_batch", p(src), p(d_dev), p(i_dev), n, h, w, p(coef), p(ws), st)
    kernel()
    coef_h = coef.cpu().numpy()
    files = enc(src, desc)
    variants = {"coef_kernel_us": lambda: events(kernel, a.reps),
                "copy_ms": lambda: wall(lambda: coef.cpu()),
                "huffman_ms": lambda: wall(lambda: jpeg.encode_host(coef_h, items, 16, jpeg.HEADER_BYTES + 3 * h * w + np.zeros(n, np.int64))),
                "end_to_end_ms": lambda: wall(lambda: enc(src, desc)),
                "download_ms": lambda: wall(lambda: src.cpu())}
    have_pillow = True
    try:
        from PIL import Image
    except ImportError:
        have_pillow = False
    if have_pillow:
        pool = ThreadPoolExecutor(16)

        def one(im):
            b = io.BytesIO()
            Image.fromarray(im).save(b, "JPEG", quality=75, subsampling="4:2:0")
            return b.getvalue()

        variants["pillow16_ms"] = lambda: wall(lambda: list(pool.map(one, photos)))
        variants["pillow_1thread_ms"] = lambda: wall(lambda: [one(im) for im in photos[:32]])
        for i in (0, n // 2, n - 1):                                              # the two paths write the same files
            assert files[i] == one(photos[i]), i
    # the compose kernel: 64 images of 352 x 352, 300 boxes each
    cn, cs, ck = 64, 352, 300
    g = torch.Generator().manual_seed(0)
    x = torch.randn(cn, 3, cs, cs, generator=g).to(dev)
    lo, hi = torch.rand(cn * ck, 2, generator=g) * 0.8, torch.rand(cn * ck, 2, generator=g) * 0.2 + 0.02
    rows = torch.cat([lo, lo + hi, torch.full((cn * ck, 2), 0.9), torch.randint(0, 20, (cn * ck, 1), generator=g).float()], 1).to(dev)
    ann = viz.Annotator(thickness=2)
    sizes = [(cs, cs)] * cn
    begin = torch.arange(cn, dtype=torch.int32, device=dev) * ck
    count = torch.full((cn,), ck, dtype=torch.int32, device=dev)
    rec, _, _, K = ann.boxes((rows, begin, count), 0, sizes, dev)
    citems = np.zeros(cn, viz.ITEM)
    for i in range(cn):
        citems[i] = (i * 3 * cs * cs, 3 * cs, 0, cs, cs)
    ci_dev = torch.from_numpy(citems.view(np.uint8).copy()).to(dev)
    dst = torch.empty(cn * 3 * cs * cs, dtype=torch.uint8, device=dev)
    cws = torch.empty(_lib.query("mny_viz_ws_bytes", cn), dtype=torch.uint8, device=dev)
    m3, s3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)

    def compose(boxes):
        return lambda: _lib.call("mny_viz_compose", p(x), cs, cs, m3, s3, None, None, p(ci_dev), cn, p(rec) if boxes else None, p(begin), p(count), K,
                                 None, 0, None, p(dst), p(cws), st)

    variants["compose_us/300_boxes"] = lambda: events(compose(True), a.reps)
    variants["compose_us/no_boxes"] = lambda: events(compose(False), a.reps)
    variants["boxes_us"] = lambda: events(lambda: ann.boxes((rows, begin, count), 0, sizes, dev), a.reps)

    times = {k: [] for k in variants}
    for r in range(a.warmup + a.rounds):
        for k, fn in variants.items():
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    med = {k: statistics.median(v) for k, v in times.items()}
    cbytes = cn * cs * cs * (12 + 3)
    res = {"batch": n, "image": "%dx%d RGB" % (h, w), "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "stream_bytes_per_image": round(sum(len(f) for f in files) / n), "coef_bytes": 2 * total,
           "coef_kernel_us": round(med["coef_kernel_us"], 1), "coef_kernel_images_per_s": round(n / med["coef_kernel_us"] * 1e6),
           "copy_ms": round(med["copy_ms"], 2), "huffman16_ms": round(med["huffman_ms"], 2), "end_to_end_ms": round(med["end_to_end_ms"], 2),
           "end_to_end_images_per_s": round(n / med["end_to_end_ms"] * 1e3), "download_ms": round(med["download_ms"], 2),
           "compose": {"images": cn, "size": cs, "boxes_per_image": ck, "us_300_boxes": round(med["compose_us/300_boxes"], 1),
                       "us_no_boxes": round(med["compose_us/no_boxes"], 1), "gbps_300_boxes": round(cbytes / med["compose_us/300_boxes"] / 1e3, 1),
                       "images_per_s_300_boxes": round(cn / med["compose_us/300_boxes"] * 1e6), "boxes_call_us": round(med["boxes_us"], 1)}}
    if have_pillow:
        res["pillow16_ms"] = round(med["pillow16_ms"], 2)
        res["pillow16_images_per_s"] = round(n / med["pillow16_ms"] * 1e3)
        res["pillow_us_per_image_per_thread"] = round(med["pillow_1thread_ms"] * 1e3 / 32, 1)
    res["spread_pct"] = {k: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
