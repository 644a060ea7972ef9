#!/usr/bin/env python3
"""Fits the six anchors of the VOC config to synthetic labels (synthetic.targets: w, h = 0.05 + 0.5 U of the image) on the device and
prints the anchors, the mask and the report.

    python examples/fit_anchors_synthetic.py [--images 2048] [--generations 1000] [--population 64] [--thr 0.25] [--seed 0]

The result drops into config["yolo"]; the anchors of a live model are not changed, a new yolo(config) is built with them.
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mobilenet_yolo_pytorch_amd import anchors, synthetic, yolo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--generations", type=int, default=1000)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--thr", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fit_anchors_synthetic.py needs the MI355X"
    config = copy.deepcopy(synthetic.VOC_CONFIG)
    labels = synthetic.targets(a.images, boxes_per_image=3, seed=a.seed + 1)
    fit = anchors.autoanchor(labels, config, generations=a.generations, population=a.population, thr=a.thr, seed=a.seed)
    rep = fit["report"]
    print("anchors", json.dumps(fit["anchors"]))
    print("mask   ", json.dumps(fit["mask"]))
    print("boxes %d (skipped %d), k-means %d steps (converged: %s), %d of %d generations improved" % (
        rep["boxes"], rep["skipped"], rep["kmeans_steps"], rep["kmeans_converged"], rep["evolve_improved"], a.generations))
    for stage in ("before", "kmeans", "evolved", "rounded"):
        if stage in rep:
            r = rep[stage]
            print("%-8s mean best IoU above %.2f: %.4f  recall %.4f  positives per head %s  orphans %d  best-anchor histogram %s" % (
                stage, rep["thr"], r["fitness"], r["recall"], [sum(p) for p in r["pos"]], r["orphans"], r["best"]))
    assert rep["evolved"]["fitness"] >= rep["kmeans"]["fitness"], "evolution lost fitness"
    config["yolo"]["anchors"], config["yolo"]["mask"] = fit["anchors"], fit["mask"]
    model = yolo(config)
    print("yolo(config) built with", model.yolo_losses[0].anchors)
    print(json.dumps({"anchors": fit["anchors"], "mask": fit["mask"], "report": rep}))


if __name__ == "__main__":
    main()
