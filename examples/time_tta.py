#!/usr/bin/env python3
"""Times test-time augmentation (tta.TTA) at N = 64, 352x352 with default_views(352) = 352 plain, 320 mirrored, 256 plain, on procedural
weights: each of the three kernels of csrc/tta.hip alone, the whole TTA call, and beside it three plain `model(x)` calls at the three
sizes (what the same views cost one by one, each with its own NMS and host sync).

    python examples/time_tta.py [--batch 64] [--size 352] [--windows 5] [--min-window 1.0] [--warmup 3] [--val-conf 0.1]

Method of examples/time_eval.py: a figure is a host clock around `reps` calls that ends in a device synchronise, divided by `reps`;
`reps` is chosen after the warm-up so that a window lasts at least `--min-window` seconds; the median of `--windows` windows is
reported with their spread (max - min).  tta_view: the largest non-identity view (mirror + resize).  det_append: the identity view's
candidates into a zeroed joint buffer (the figure includes the 4*N-byte memset of the counts).  nms_merge: on the joint candidates of
a finished TTA call.  No accuracy is measured: the weights are procedural.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from mobilenet_yolo_pytorch_amd import ops, yolo  # noqa: E402
from mobilenet_yolo_pytorch_amd.tta import TTA, default_views  # noqa: E402
from oracle import procedural  # noqa: E402
from time_eval import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--val-conf", type=float, default=0.1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_tta.py needs the MI355X"
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = a.val_conf
    views = default_views(a.size)
    x = procedural.images(a.batch, a.size, a.size, seed=3).cuda()
    tta = TTA(m, views=views, merge=True)
    det = tta(x)
    b = next(iter(tta._bufs.values()))
    res = {"batch": a.batch, "views": views, "val_conf": a.val_conf, "windows": a.windows, "min_window_s": a.min_window, "warmup": a.warmup,
           "joint_candidates_per_image": round(float(b["counts"].float().mean()), 1), "kept_per_image": round(sum(len(d) for d in det) / a.batch, 1)}
    big = max(views[1:], key=lambda v: v[0])
    xv = torch.empty(a.batch, 3, big[0], big[0], device=x.device)
    res["tta_view"] = measure(lambda: ops.tta_view(x, big[0], big[0], big[1], out=xv), a.windows, a.min_window, a.warmup)
    plan0 = m._plan(a.batch, a.size, a.size, False)
    plan0.forward_eval(x, [a.val_conf] * 2, nms=False)
    joint, counts = torch.zeros_like(b["rows"]), torch.zeros_like(b["counts"])

    def append():
        counts.zero_()
        ops.det_append(plan0.rows, plan0.cnt1, joint, counts, flip=True)

    res["det_append"] = measure(append, a.windows, a.min_window, a.warmup)
    res["det_append"]["rows_copied_per_image"] = round(float(plan0.cnt1.float().mean()), 1)
    res["det_append"]["src_stride"] = plan0.cap
    tta(x)
    N = a.batch
    res["nms_merge"] = measure(lambda: ops.nms_merge(b["rows"].view(-1, 7), b["seg_begin"], b["counts"], b["out_idx"], b["out"][:N], b["prefix"],
                                                     b["out_rows"], thr=tta.nms_thr), a.windows, a.min_window, a.warmup)
    res["tta_call"] = measure(lambda: tta(x), a.windows, a.min_window, a.warmup)
    plain = TTA(m, views=views, merge=False)
    res["tta_call_no_merge"] = measure(lambda: plain(x), a.windows, a.min_window, a.warmup)
    xs = [x if (s, f) == views[0] else ops.tta_view(x, s, s, f) for s, f in views]
    single = [measure(lambda t=t: m(t), a.windows, a.min_window, a.warmup) for t in xs]
    res["model_calls"] = single
    res["model_calls_sum_ms"] = round(sum(s["ms"] for s in single), 4)
    res["tta_over_sum"] = round(res["tta_call"]["ms"] / res["model_calls_sum_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
