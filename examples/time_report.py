#!/usr/bin/env python3
"""Times the two validation-report entries, `det_curves` (P / R / F1 curves, best confidence) and `det_confusion` (detection confusion
matrix), on packed detections that are already on the device, and one pass of the pure-numpy restatement tests/report_ref.py over the
same sets on the host.

    python examples/time_report.py [--sets voc,bdd] [--windows 5] [--min-window 1.0] [--warmup 3] [--no-ref]

Sets and method are those of examples/time_eval.py: voc = synthetic.map_case(4952, 21, seed=0) (VOC07-test sized), bdd =
synthetic.map_case(10000, 11, seed=1, mean_gt=18.5, clutter=30.0) (BDD100K-val sized); image sizes 1280x720.  A figure is a host clock
around `reps` calls that ends in a device synchronise, divided by `reps`; `reps` is chosen after the warm-up so that a window lasts
at least `--min-window` seconds; the median of `--windows` windows is reported with their spread (max - min).  The match flags the
curves consume come from one `coco_eval(iou_thrs=[0.5], area_rngs=[[0, 1e10]], max_dets=[100], matches=True)` call, timed beside them
("coco_flags"); "report" is the three calls in a row, what `Evaluator.compute_report_device` does after packing.  The host baseline is
the restatement (written for reading, not speed) on the device's flags: one pass, wall clock; its outputs are compared with the
device's, integers for equality and fp64 values bit for bit.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from mobilenet_yolo_pytorch_amd import evalmap, synthetic  # noqa: E402
from time_eval import SETS, measure  # noqa: E402

FLAGS = dict(iou_thrs=[0.5], area_rngs=[[0, 1e10]], max_dets=[100], stat_desc=[[0, 0, 0, 0]], matches=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="voc,bdd")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--smooth", type=int, default=101)
    ap.add_argument("--no-ref", action="store_true", help="skip the host pass of the restatement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_report.py needs the MI355X"
    res = {"windows": a.windows, "min_window_s": a.min_window, "warmup": a.warmup, "grid": a.grid, "smooth": a.smooth}
    for name in a.sets.split(","):
        kw = dict(SETS[name])
        n_img, nc = kw.pop("n_images"), kw.pop("n_classes")
        case = synthetic.map_case(n_img, nc, **kw)
        sizes = np.tile(np.array([[1280, 720]], np.float32), (n_img, 1))
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in case]
        dsz = torch.from_numpy(sizes).cuda()
        flags = lambda: evalmap.coco_eval(*dev, nc, image_sizes=dsz, **FLAGS)
        f = flags()
        m, ig = f["det_match"][0, 0].contiguous(), f["det_ignore"][0, 0].contiguous()
        curves = lambda m=m, ig=ig: evalmap.det_curves(dev[1], dev[2], m, ig, dev[5], dev[6], nc, grid=a.grid, smooth=a.smooth)
        confusion = lambda: evalmap.det_confusion(*dev, nc, image_sizes=dsz)

        def report():
            g = flags()
            return curves(g["det_match"][0, 0], g["det_ignore"][0, 0]), confusion()

        r = {"images": n_img, "classes": nc - 1, "detections": int(case[1].size), "objects": int(case[5].size)}
        for key, fn in (("det_curves", curves), ("det_confusion", confusion), ("coco_flags", flags), ("report", report)):
            r[key] = measure(fn, a.windows, a.min_window, a.warmup)
        c, x = curves(), confusion()
        torch.cuda.synchronize()
        r["best_conf"], r["F1_at_best"] = round(float(c["best_conf"][0]), 6), round(float(c["at_best"][-1, 2]), 6)
        r["matched"], r["considered"] = int((x["det_gt"] >= 0).sum()), int((x["det_gt"] != -2).sum())
        if not a.no_ref:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import report_ref
            mh, ih = m.cpu().numpy(), ig.cpu().numpy()
            t0 = time.perf_counter()
            rc = report_ref.curves(case[1], case[2], mh, ih, case[5], case[6], nc, grid=a.grid, smooth=a.smooth)
            r["numpy_curves_s"] = round(time.perf_counter() - t0, 2)
            t0 = time.perf_counter()
            rx = report_ref.confusion(*case, nc, image_sizes=sizes)
            r["numpy_confusion_s"] = round(time.perf_counter() - t0, 2)
            bits = lambda t: np.ascontiguousarray(t.cpu().numpy(), np.float64).reshape(-1).view(np.int64)
            r["curves_equal"] = bool(all(np.array_equal(c[k].cpu().numpy().reshape(-1), np.asarray(rc[k]).reshape(-1)) for k in ("tp", "fp", "npos", "best"))
                                     and all(np.array_equal(bits(c[k]), np.asarray(rc[k], np.float64).reshape(-1).view(np.int64))
                                             for k in ("precision", "recall", "f1", "mean_f1", "smooth_f1", "best_conf", "at_best")))
            r["confusion_equal"] = bool(np.array_equal(x["matrix"].cpu().numpy(), rx["matrix"]) and np.array_equal(x["det_gt"].cpu().numpy(), rx["det_gt"]))
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
