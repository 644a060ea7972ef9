#!/usr/bin/env python3
"""Times the two evaluation entries, `coco_eval` (COCO-style AP / AR) and `map_eval` (VOC07 11-point mAP), on packed detections that
are already on the device, and one pass of the pure-numpy restatement tests/coco_ref.py over the same sets on the host.

    python examples/time_eval.py [--sets voc,bdd] [--windows 5] [--min-window 1.0] [--warmup 3] [--no-ref]

Sets: voc = synthetic.map_case(4952, 21, seed=0) (VOC07-test sized), bdd = synthetic.map_case(10000, 11, seed=1, mean_gt=18.5,
clutter=30.0) (BDD100K-val sized); image sizes 1280x720.  A figure is a host clock around `reps` calls that ends in a device
synchronise, divided by `reps`; `reps` is chosen after the warm-up so that a window lasts at least `--min-window` seconds; the median
of `--windows` windows is reported with their spread (max - min).  The host baseline is the restatement, NOT pycocotools (which is not
installed here): one pass, wall clock.  Prints one JSON line.
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
from mobilenet_yolo_pytorch_amd import evalmap, synthetic  # noqa: E402

SETS = {"voc": dict(n_images=4952, n_classes=21, seed=0), "bdd": dict(n_images=10000, n_classes=11, seed=1, mean_gt=18.5, clutter=30.0)}


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(fn, windows, min_window, warmup):
    for _ in range(warmup):
        fn()
    reps = max(1, int(np.ceil(min_window / max(timed(fn, 3), 1e-6))))
    ts = [timed(fn, reps) * 1e3 for _ in range(windows)]
    return {"ms": round(statistics.median(ts), 4), "spread_ms": round(max(ts) - min(ts), 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="voc,bdd")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true", help="skip the host pass of the restatement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_eval.py needs the MI355X"
    res = {"windows": a.windows, "min_window_s": a.min_window, "warmup": a.warmup}
    for name in a.sets.split(","):
        kw = dict(SETS[name])
        n_img, nc = kw.pop("n_images"), kw.pop("n_classes")
        case = synthetic.map_case(n_img, nc, **kw)
        sizes = np.tile(np.array([[1280, 720]], np.float32), (n_img, 1))
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in case]
        dsz = torch.from_numpy(sizes).cuda()
        r = {"images": n_img, "classes": nc - 1, "detections": int(case[1].size), "objects": int(case[5].size)}
        r["coco_eval"] = measure(lambda: evalmap.coco_eval(*dev, nc, image_sizes=dsz), a.windows, a.min_window, a.warmup)
        r["map_eval"] = measure(lambda: evalmap.map_eval(*dev, nc), a.windows, a.min_window, a.warmup)
        out = evalmap.coco_eval(*dev, nc, image_sizes=dsz)
        r["AP"], r["AP50"] = [round(v, 6) for v in out["stats"][:2].tolist()]
        if not a.no_ref:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import coco_ref
            t0 = time.perf_counter()
            ref = coco_ref.evaluate(*case, nc, image_sizes=sizes)
            r["numpy_restatement_s"] = round(time.perf_counter() - t0, 2)
            r["stats_max_abs_diff"] = float(np.abs(ref["stats"] - out["stats"].cpu().numpy()).max())
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
