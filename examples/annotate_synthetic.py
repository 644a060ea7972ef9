#!/usr/bin/env python3
"""Caller-side counterpart of inference.py:58-104: eval forward, boxes drawn on the images, the drivable-area overlay, one JPEG
file per image — and the val_batch*_pred.jpg contact sheet YOLO trainers write — with every pixel staying on the device until
it is a quantised coefficient.

    python examples/annotate_synthetic.py [--batch 8] [--size 352] [--seg 2] [--names voc|bdd|none] [--out annotated] [--quality 75]

The batch is synthetic photos through BatchPrep; the weights are random, so the boxes are many and meaningless.  With --seg C the
config gets a `seg:` section and the seg probabilities (segeval.upsample at the network size) dim channel G for class 0 and R
for class 1, as the reference does.  Every box carries "name score" (--names voc, the default; bdd: that dataset's ten names, classes
beyond them labelled by their index; none: colours alone, as before names could be drawn)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilenet_yolo_pytorch_amd import segeval, synthetic, yolo  # noqa: E402
from mobilenet_yolo_pytorch_amd.jpeg import JpegEncoder  # noqa: E402
from mobilenet_yolo_pytorch_amd.prep import BatchPrep  # noqa: E402
from mobilenet_yolo_pytorch_amd.viz import Annotator  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--seg", type=int, default=0, help="classes of a segmentation head (0: the VOC config, no head; at most 2)")
    ap.add_argument("--names", choices=("voc", "bdd", "none"), default="voc", help="the class names drawn on the boxes")
    ap.add_argument("--out", default="annotated")
    ap.add_argument("--quality", type=int, default=75)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = dict(synthetic.VOC_CONFIG, seg={"num_classes": a.seg}) if a.seg else synthetic.VOC_CONFIG
    model = yolo(cfg).to(dev).eval()
    for hs in model.yolo_losses:
        hs.val_conf = 0.3
    r = np.random.RandomState(0)
    photos = synthetic.photos([(int(r.randint(300, 500)), int(r.randint(300, 500))) for _ in range(a.batch)], seed=0)
    images = BatchPrep([(a.size, a.size)], MEAN, STD, device=dev)(photos)
    out = model(images)
    dets, probs = out, None
    if a.seg:
        dets = out[0]
        probs = segeval.upsample(model.seg_logits(), [(a.size, a.size)] * a.batch)     # [C,H,W] probabilities per image, on the device
    names = {"voc": synthetic.VOC_NAMES, "bdd": synthetic.BDD_NAMES, "none": None}[a.names]
    ann = Annotator(thickness=2, score_thres=0.15, names=names)
    enc = JpegEncoder(quality=a.quality, subsampling="4:2:0", device=dev)
    os.makedirs(a.out, exist_ok=True)
    buf, desc = ann.annotate(images, dets=dets, seg_probs=probs, mean=MEAN, std=STD)   # inference.py:70-103
    ann.check()
    files = enc(buf, desc)                                                              # inference.py:104
    for i, f in enumerate(files):
        with open(os.path.join(a.out, "image%03d_result.jpg" % i), "wb") as fh:
            fh.write(f)
    sheet, sdesc = ann.sheet(images, cols=4, dets=dets, seg_probs=probs, mean=MEAN, std=STD)
    with open(os.path.join(a.out, "val_batch0_pred.jpg"), "wb") as fh:
        fh.write(enc(sheet, sdesc)[0])
    assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in files)
    print("%d images, %s detections, %d + 1 files in %s/ (%d bytes; sheet %dx%d)" % (
        a.batch, [len(d) for d in dets], len(files), a.out, sum(len(f) for f in files), int(sdesc[0]["h"]), int(sdesc[0]["w"])))


if __name__ == "__main__":
    main()
