#!/usr/bin/env python3
"""Times the random-perspective kernel (mny_aug_warp_batch) against the host path it replaces: Pillow's Image.transform with the
same coefficients on a 16-thread pool, BatchPrep.pack, one upload of RGB.

    python examples/time_warp.py [--batch 256] [--rounds 7] [--warmup 2] [--reps 20]

The batch is `--batch` VOC-sized RGB photos (375x500, synthetic.photos).  Three plans: `default` (RandomPerspective's defaults:
scale and translation only, the affine path), `full` (rotation, shear and perspective as well: the division path) and
`identity` (every item copied: the floor of the launch).  `kernel_us` is the HIP-event time of `--reps` back-to-back launches
divided by `--reps`; `gbps` counts the image bytes read plus written (2 * 3 * h * w per image) over that time.  The Pillow
figures are wall-clock around transform + pack + upload + synchronise.  Every figure is the median of `rounds` windows after
`warmup` unrecorded ones, the variants taking turns inside a round.  Prints one JSON line.
"""
import argparse
import ctypes
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
from mobilenet_yolo_pytorch_amd import _lib, augment, prep, synthetic  # noqa: E402

FULL = dict(degrees=10.0, translate=0.1, scale=0.5, shear=5.0, perspective=2e-4)


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
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_warp.py needs the MI355X"
    dev = torch.device("cuda:0")
    n, h, w = a.batch, 375, 500
    distinct = synthetic.photos([(h, w)] * min(n, 32), seed=0)
    photos = [distinct[i % len(distinct)] for i in range(n)]
    packer = prep.BatchPrep([(352, 352)], [0, 0, 0], [1, 1, 1], device=dev)
    stage, desc, _, _ = packer.pack(photos)
    src = stage.to(dev)
    dst = torch.empty_like(src)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    ws = torch.empty(_lib.query("mny_aug_warp_ws_bytes", n, 3, h, w), dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    plans = {"default": augment.RandomPerspective(1).plan([(h, w)] * n), "full": augment.RandomPerspective(1, **FULL).plan([(h, w)] * n),
             "identity": augment.RandomPerspective(1, p=0.0).plan([(h, w)] * n)}
    assert not plans["default"]["identity"].any() and np.all(plans["default"]["records"]["c"][:, 6:] == 0)
    assert np.all(plans["full"]["records"]["c"][:, 6:] != 0) and plans["identity"]["identity"].all()
    recs = {k: torch.from_numpy(v["records"].view(np.uint8).copy()).to(dev) for k, v in plans.items()}

    def kernel(k):
        return lambda: _lib.call("mny_aug_warp_batch", p(src), p(d_dev), p(recs[k]), n, 3, h, w, p(dst), p(ws), st)

    variants = {"kernel_us/" + k: (lambda k=k: events(kernel(k), a.reps)) for k in plans}
    have_pillow = True
    try:
        from PIL import Image
    except ImportError:
        have_pillow = False
    if have_pillow:
        pool = ThreadPoolExecutor(16)

        def one(args):
            im, c = args
            return np.asarray(Image.fromarray(im).transform((w, h), Image.Transform.PERSPECTIVE, tuple(c), Image.Resampling.BILINEAR, fillcolor=(127, 127, 127)))

        def pillow_path(k):
            jobs = [(im, r["c"].tolist()) for im, r in zip(photos, plans[k]["records"])]

            def run():
                s, _, _, _ = packer.pack(list(pool.map(one, jobs)))
                s.to(dev, non_blocking=True)
                torch.cuda.synchronize()
            return run
        for k in ("default", "full"):
            variants["pillow16_ms/" + k] = (lambda k=k: wall(pillow_path(k)))
        variants["pillow_1thread_ms/full"] = lambda: wall(lambda: [one(j) for j in [(im, r["c"].tolist()) for im, r in zip(photos, plans["full"]["records"])]])
        # the two paths agree on this batch
        kernel("full")()
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        for i in (0, n // 2, n - 1):
            o = int(desc["offset"][i])
            assert np.array_equal(got[o:o + 3 * h * w].reshape(h, w, 3), one((photos[i], plans["full"]["records"]["c"][i].tolist()))), i

    times = {k: [] for k in variants}
    for r in range(a.warmup + a.rounds):
        for k, fn in variants.items():
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = 2 * 3 * h * w * n
    res = {"batch": n, "image": "%dx%d RGB" % (h, w), "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps, "image_bytes_read_plus_written": nbytes,
           "kernel_us": {k: round(med["kernel_us/" + k], 1) for k in plans},
           "gbps": {k: round(nbytes / med["kernel_us/" + k] / 1e3, 1) for k in plans},
           "share_of_6400_gbps_pct": {k: round(100 * nbytes / med["kernel_us/" + k] / 1e3 / 6400, 1) for k in plans},
           "kernel_images_per_s": {k: round(n / med["kernel_us/" + k] * 1e6) for k in plans}}
    if have_pillow:
        res["pillow16_ms"] = {k: round(med["pillow16_ms/" + k], 2) for k in ("default", "full")}
        res["pillow16_images_per_s"] = {k: round(n / med["pillow16_ms/" + k] * 1e3) for k in ("default", "full")}
        res["pillow_us_per_image_per_thread"] = round(med["pillow_1thread_ms/full"] * 1e3 / n, 1)
    res["spread_pct"] = {k: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
