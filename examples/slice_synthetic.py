#!/usr/bin/env python3
"""Sliced inference on BDD100K-shaped frames: 1280x720 synthetic photos cut into 416-pixel tiles with 20 % overlap plus one whole-image
view (9 network inputs per frame), one NMS over the union, the boxes drawn on the ORIGINAL frames (the packed upload of the call, still
on the device) and one JPEG file per frame.

    python examples/slice_synthetic.py [--batch 4] [--size 416] [--tile 416] [--overlap 0.2] [--edge 0] [--no-full-view] [--out sliced]

The weights are random, so the boxes are many and meaningless; no accuracy gain is claimed or tested."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilenet_yolo_pytorch_amd import synthetic, yolo  # noqa: E402
from mobilenet_yolo_pytorch_amd.jpeg import JpegEncoder  # noqa: E402
from mobilenet_yolo_pytorch_amd.slicing import Sliced, tile_grid  # noqa: E402
from mobilenet_yolo_pytorch_amd.viz import Annotator  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--tile", type=int, default=416)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--edge", type=float, default=0.0, help="margin in network-input pixels inside which an interior tile edge cuts a box")
    ap.add_argument("--no-full-view", action="store_true")
    ap.add_argument("--out", default="sliced")
    ap.add_argument("--quality", type=int, default=75)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = yolo(synthetic.VOC_CONFIG).to(dev).eval()
    for hs in model.yolo_losses:
        hs.val_conf = 0.3
    frames = synthetic.photos([(720, 1280)] * a.batch, seed=0)
    sl = Sliced(model, size=a.size, tile=(a.tile, a.tile), overlap=a.overlap, full_view=not a.no_full_view, edge=a.edge, batch=64, mean=MEAN, std=STD)
    dets = sl(frames)                                                               # [k_i,7] per frame, normalised to the 1280x720 original
    ann = Annotator(thickness=2, score_thres=0.15, names=synthetic.VOC_NAMES)
    buf, desc = ann.annotate(sl.originals, dets=dets)                               # drawn on the packed originals, on the device
    ann.check()
    files = JpegEncoder(quality=a.quality, subsampling="4:2:0", device=dev)(buf, desc)
    os.makedirs(a.out, exist_ok=True)
    for i, f in enumerate(files):
        with open(os.path.join(a.out, "frame%03d_sliced.jpg" % i), "wb") as fh:
            fh.write(f)
    assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in files)
    tiles = len(tile_grid(720, 1280, a.tile, a.tile, a.overlap, a.overlap))
    print("%d frames, %d tiles%s each, %s detections, %d files in %s/ (%d bytes)" % (
        a.batch, tiles, "" if a.no_full_view else " + the full view", [len(d) for d in dets], len(files), a.out, sum(len(f) for f in files)))


if __name__ == "__main__":
    main()
