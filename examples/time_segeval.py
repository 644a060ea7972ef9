#!/usr/bin/env python3
"""Times the segmentation evaluator's confusion pass (`mny_seg_confusion` through segeval.SegEvaluator.add) on label maps that are
already on the device, with and without the predicted id maps written out, and one image of the numpy restatement
tests/segeval_ref.py on the host.

    python examples/time_segeval.py [--images 64,256] [--windows 5] [--min-window 1.0] [--warmup 3] [--no-ref]

Shape: the BDD100K drivable-area head, 45x80x2 logits per image against 720x1280 uint8 id maps (scale 16).  A figure is a host
clock around `reps` calls that ends in a device synchronise, divided by `reps`; `reps` is chosen after the warm-up so that a window
lasts at least `--min-window` seconds; the median of `--windows` windows is reported with their spread (max - min).  The pass is
bound by the label bytes (1 B per pixel; the head is 256x smaller; pred_out adds 1 B per pixel of writes), so the rate reported is
label bytes per second, next to the HBM figure the other rooflines of LAB_NOTES.md use (6.4 TB/s read-only stream, measured).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mobilenet_yolo_pytorch_amd import segeval  # noqa: E402

H, W, SCALE, C = 720, 1280, 16, 2
HBM_READ_TBS = 6.4


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(fn, windows, min_window, warmup, label_bytes):
    for _ in range(warmup):
        fn()
    reps = max(1, int(np.ceil(min_window / max(timed(fn, 3), 1e-6))))
    ts = [timed(fn, reps) * 1e3 for _ in range(windows)]
    ms = statistics.median(ts)
    tbs = label_bytes / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "spread_ms": round(max(ts) - min(ts), 4), "reps": reps, "label_TBps": round(tbs, 3),
            "share_of_hbm_read": round(tbs / HBM_READ_TBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="64,256")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true", help="skip the host pass of the restatement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_segeval.py needs the MI355X"
    res = {"label": [H, W], "head": [H // SCALE, W // SCALE, C], "hbm_read_TBps": HBM_READ_TBS, "windows": a.windows,
           "min_window_s": a.min_window, "warmup": a.warmup}
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in [int(v) for v in a.images.split(",")]:
        logits = torch.randn(n, H // SCALE, W // SCALE, C, device="cuda", generator=g) * 2
        labels = torch.randint(0, C + 1, (n, H, W), device="cuda", generator=g, dtype=torch.uint8)
        labels[:, -16:] = 255
        ev = segeval.SegEvaluator(C, device="cuda")
        r = {"label_bytes": n * H * W}
        r["confusion"] = measure(lambda: ev.add(logits, labels), a.windows, a.min_window, a.warmup, n * H * W)
        r["confusion_pred_out"] = measure(lambda: ev.add(logits, labels, pred_out=True), a.windows, a.min_window, a.warmup, n * H * W)
        ev.reset()
        ev.add(logits, labels)
        m = ev.compute()
        assert int(ev.confusion.sum()) + int(ev.ignored.item()) == n * H * W
        r["miou"], r["pixel_acc"] = round(m["miou"], 6), round(m["pixel_acc"], 6)
        res["n%d" % n] = r
    if not a.no_ref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import segeval_ref
        x, lab = logits[:1].cpu().numpy(), labels[0].cpu().numpy()
        t0 = time.perf_counter()
        ref = segeval_ref.evaluate(x, [lab], C)
        res["numpy_restatement_one_image_s"] = round(time.perf_counter() - t0, 3)
        one = segeval.SegEvaluator(C, device="cuda")
        pred = one.add(logits[:1], labels[:1], pred_out=True)[0].cpu().numpy()
        res["pred_mismatch_outside_ambiguous"] = int((pred != ref["preds"][0])[~ref["ambiguous"][0]].sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
