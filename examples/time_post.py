#!/usr/bin/env python3
"""Times the post-processing options (postprocess.Detector) at N = 64, 352x352 on procedural weights, next to plain `model(x)`: the
decode of both heads, the NMS and the top-k alone on the candidates of a finished call, and the whole Detector call, for
  default      PostProcess(): the settings of model(x) (bit-identical result)
  multi        conf_thres = score_thres = 0.001, multi_label, max_det = 300, class-aware NMS
  multi_agn    the same with class-agnostic NMS
together with the candidates per image that the settings produce.

    python examples/time_post.py [--batch 64] [--size 352] [--windows 5] [--min-window 1.0] [--warmup 3] [--val-conf 0.1] [--max-candidates K]

Method of examples/time_eval.py: a figure is a host clock around `reps` calls that ends in a device synchronise, divided by `reps`;
`reps` is chosen after the warm-up so that a window lasts at least `--min-window` seconds; the median of `--windows` windows is
reported with their spread (max - min).  No accuracy is measured: the weights are procedural.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from mobilenet_yolo_pytorch_amd import Detector, PostProcess, postprocess, yolo  # noqa: E402
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
    ap.add_argument("--max-candidates", type=int, default=None, help="per-image bound of the candidate buffer (default: the worst case)")
    ap.add_argument("--only", default="", help="comma-separated subset of model,default,multi,multi_agn")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_post.py needs the MI355X"
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = a.val_conf
    x = procedural.images(a.batch, a.size, a.size, seed=3).cuda()
    N, C = a.batch, m.num_classes
    only = set(a.only.split(",")) if a.only else {"model", "default", "multi", "multi_agn"}
    res = {"batch": N, "size": a.size, "val_conf": a.val_conf, "windows": a.windows, "min_window_s": a.min_window, "warmup": a.warmup}
    win = (a.windows, a.min_window, a.warmup)
    if "model" in only:
        res["model_call"] = measure(lambda: m(x), *win)
    low = dict(conf_thres=0.001, score_thres=0.001, multi_label=True, max_det=300, max_candidates=a.max_candidates)
    for name, post in (("default", PostProcess()), ("multi", PostProcess(**low)), ("multi_agn", PostProcess(agnostic=True, **low))):
        if name not in only:
            continue
        det = Detector(m, post)
        out = det(x)
        b = next(iter(det._bufs.values()))
        plan = m._plan(N, a.size, a.size, False)
        r = {"row_stride": b["stride"], "candidates_per_image": round(float(b["cnt1"].float().mean()), 1),
             "candidates_max": int(b["cnt1"].max()), "kept_per_image": round(sum(len(d) for d in out) / N, 1)}
        o = b["out"]
        r["decode"] = measure(lambda: postprocess.decode_plan(plan, post, m, b["rows"], b["cnt0"], b["cnt1"], o[N + 1:2 * N + 1], o[2 * N + 1:],
                                                              b["cmask"]), *win)
        r["nms"] = measure(lambda: postprocess.run_nms(post, C, b["rows"], b["seg_begin"], b["cnt1"], b["out_idx"], o, b["out_rows"], b["ws"]), *win)
        if post.max_det is not None:
            r["nms_kept_per_image"] = round(float(o[:N].float().mean()), 1)      # (the last NMS above ran without the top-k behind it)
            r["topk"] = measure(lambda: postprocess.run_topk(post, b["rows"], b), *win)
        r["detector_call"] = measure(lambda: det(x), *win)
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
