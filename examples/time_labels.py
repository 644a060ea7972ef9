#!/usr/bin/env python3
"""Times class-name labels on annotated images (mny_viz_labels, mny_viz_compose_labels) beside the annotation kernel without them.

    python examples/time_labels.py [--rounds 7] [--warmup 2] [--reps 50] [--other-lib /path/to/another/libmnyolo.so]

The case of examples/time_encode.py: 64 images of 352x352 from a normalised fp32 batch, 300 detection rows each, thickness 2; the VOC
names in Pillow's built-in bitmap font (11 rows, 6 columns a character), so a label is "name 0.81".
  compose_us/no_names     mny_viz_compose, what Annotator() runs
  compose_us/null_labels  mny_viz_compose_labels with labels = NULL: the same kernel
  compose_us/other_lib    mny_viz_compose of the library given with --other-lib (a build of another commit), taking turns with the
                          variants above inside every round: the A/B that shows whether the kernel without labels moved
  labels_us               mny_viz_labels for the 19 200 rows
  compose_us/filled       mny_viz_compose_labels, labels on the box's colour
  compose_us/unfilled     mny_viz_compose_labels, labels straight on the image
Every figure is the HIP-event time of `--reps` back-to-back launches divided by `--reps`, the median of `rounds` windows after
`warmup` unrecorded ones; `spread_pct` is (max - min) / median over the windows.  MNY_LIB picks the library under test as
everywhere.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mobilenet_yolo_pytorch_amd import _lib, synthetic, viz  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_labels.py needs the MI355X"
    dev = torch.device("cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cn, cs, ck = 64, 352, 300
    g = torch.Generator().manual_seed(0)
    x = torch.randn(cn, 3, cs, cs, generator=g).to(dev)
    lo, hi = torch.rand(cn * ck, 2, generator=g) * 0.8, torch.rand(cn * ck, 2, generator=g) * 0.2 + 0.02
    rows = torch.cat([lo, lo + hi, torch.full((cn * ck, 2), 0.9), torch.randint(0, 20, (cn * ck, 1), generator=g).float()], 1).to(dev)
    sizes = [(cs, cs)] * cn
    begin = torch.arange(cn, dtype=torch.int32, device=dev) * ck
    count = torch.full((cn,), ck, dtype=torch.int32, device=dev)
    anns = {"filled": viz.Annotator(thickness=2, names=synthetic.VOC_NAMES), "unfilled": viz.Annotator(thickness=2, names=synthetic.VOC_NAMES, label_bg=False)}
    recs = {k: ann.records((rows, begin, count), 0, sizes, dev) for k, ann in anns.items()}
    rec, K = recs["filled"][0], recs["filled"][4]
    atlas, strips = anns["filled"]._atlas(dev)
    items = np.zeros(cn, viz.ITEM)
    for i in range(cn):
        items[i] = (i * 3 * cs * cs, 3 * cs, 0, cs, cs)
    i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    dst = torch.empty(cn * 3 * cs * cs, dtype=torch.uint8, device=dev)
    ws = torch.empty(_lib.query("mny_viz_ws_bytes", cn), dtype=torch.uint8, device=dev)
    m3, s3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    head = (p(x), cs, cs, m3, s3, None, None, p(i_dev), cn, p(rec), p(begin), p(count), K, None, 0, None, p(dst), p(ws))

    def with_labels(lab):
        return lambda: _lib.call("mny_viz_compose_labels", *head, p(lab) if lab is not None else None, p(atlas), p(strips), st)

    ann = anns["filled"]
    d_dev = torch.from_numpy(np.array([(0, cs, cs)] * cn, viz.DESC).view(np.uint8).copy()).to(dev)
    lab_out = torch.zeros(K * viz.LABEL.itemsize, dtype=torch.uint8, device=dev)
    rgb = (ctypes.c_uint8 * 3)(255, 255, 255)
    variants = {"compose_us/no_names": lambda: events(lambda: _lib.call("mny_viz_compose", *head, st), a.reps),
                "compose_us/null_labels": lambda: events(with_labels(None), a.reps),
                "labels_us": lambda: events(lambda: _lib.call("mny_viz_labels", p(rows), 0, p(begin), p(count), cn, K, p(d_dev), p(rec), p(strips), len(ann.names),
                                                              ann.text_h, 1, 1, 1, rgb, p(lab_out), st), a.reps),
                "compose_us/filled": lambda: events(with_labels(recs["filled"][1]), a.reps),
                "compose_us/unfilled": lambda: events(with_labels(recs["unfilled"][1]), a.reps)}
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        other.mny_viz_compose.restype, other.mny_viz_compose.argtypes = _lib._SIGS["mny_viz_compose"]

        def other_compose():
            assert other.mny_viz_compose(*head, st) == 0

        variants["compose_us/other_lib"] = lambda: events(other_compose, a.reps)
    times = {k: [] for k in variants}
    for r in range(a.warmup + a.rounds):
        for k, fn in variants.items():
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    res = {"images": cn, "size": cs, "boxes_per_image": ck, "text_h": ann.text_h, "atlas_bytes": int(len(ann.atlas)), "rounds": a.rounds, "warmup": a.warmup,
           "reps": a.reps, "library": _lib.LIB_PATH, "other_lib": a.other_lib}
    res.update({k: round(statistics.median(v), 1) for k, v in times.items()})
    res["windows"] = {k: [round(t, 1) for t in v] for k, v in times.items() if k in ("compose_us/no_names", "compose_us/other_lib")}
    res["spread_pct"] = {k: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
