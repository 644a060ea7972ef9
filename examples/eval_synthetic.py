#!/usr/bin/env python3
"""Caller-side counterpart of the reference's validation pass (train.py:test(), :333-424) on synthetic data, everything
after JPEG decode on the GPU:  decoded uint8 photos -> BatchPrep (Resize/ToTensor/Normalize of collate_fn) ->
model.eval() forward (network + decode + per-class NMS) -> Evaluator (VOC07 11-point mAP, COCO-style AP / AR) -> adjust_confidence.
With --seg C the config gets a `seg:` section of C classes (the BDD100K config has 2: the drivable-area head) and the batched seg
logits are scored against full-resolution id maps by segeval.SegEvaluator: per-class IoU, mIoU, pixel accuracy — no seg map is
copied to the host except the reference's own seg_out of image 0.

With --report the same detections also give the validation report: per-class precision / recall / F1 at the confidence that maximises
the smoothed mean F1 (a threshold on obj * cls_conf, the score the metrics use), and the detection confusion matrix.

With --multi-label / --agnostic / --max-det K the detections come from postprocess.Detector instead of model(images): the Ultralytics
protocol (conf and score threshold 0.001, a candidate per (box, class) pair, class-agnostic NMS, at most K detections per image).

    python examples/eval_synthetic.py [--images 256] [--batch 64] [--size 352] [--seg 2] [--report] [--multi-label] [--agnostic] [--max-det 300]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilenet_yolo_pytorch_amd import Detector, PostProcess, synthetic, yolo  # noqa: E402
from mobilenet_yolo_pytorch_amd.evalmap import Evaluator, adjust_confidence  # noqa: E402
from mobilenet_yolo_pytorch_amd.prep import BatchPrep  # noqa: E402
from mobilenet_yolo_pytorch_amd.segeval import SegEvaluator  # noqa: E402


def id_maps(sizes, n_classes, seed):
    """Synthetic ground truth: uint8 id maps at the photos' sizes, one vertical band per class above a background sky, a strip of
    ignored pixels (255) at the bottom."""
    r = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        m = np.zeros((h, w), np.uint8)
        cuts = np.sort(r.randint(0, w, n_classes + 1))
        for c in range(n_classes):
            m[h // 2:, cuts[c]:cuts[c + 1]] = c + 1
        m[h - 8:] = 255
        out.append(m)
    return out


def print_report(rep, names):
    """the table current YOLO trainers print per epoch, at the confidence that maximises the smoothed mean F1"""
    print("REPORT best_conf %.3f (on obj * cls_conf)  P %.4f  R %.4f  F1 %.4f" % (rep["best_conf"], rep["P"], rep["R"], rep["F1"]))
    print("  %-10s %8s %8s %8s %8s" % ("class", "P", "R", "F1", "objects"))
    for n in names:
        P, R, F1, n_pos = rep["per_class"][n]
        print("  %-10s %8.4f %8.4f %8.4f %8d" % (n, P, R, F1, n_pos) if n_pos else "  %-10s %8s %8s %8s %8d" % (n, "-", "-", "-", 0))
    cm = rep["confusion"]
    K = cm.shape[0] - 1
    print("  confusion (rows predicted, columns true, last = background): %d matched on the diagonal, %d off it, %d missed, %d false positives" % (
        int(np.trace(cm[:K, :K])), int(cm[:K, :K].sum() - np.trace(cm[:K, :K])), int(cm[K, :K].sum()), int(cm[:K, K].sum())))
    with np.printoptions(linewidth=250):
        print(cm)
    assert cm[K, K] == 0 and 0.0 <= rep["best_conf"] <= 1.0 and len(rep["per_class"]) == K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--seg", type=int, default=0, help="classes of a segmentation head (0: the VOC config, no head)")
    ap.add_argument("--report", action="store_true", help="print the P / R / F1 table at the best confidence and the confusion matrix")
    ap.add_argument("--multi-label", action="store_true", help="a candidate per (box, class) pair with obj * cls > 0.001")
    ap.add_argument("--agnostic", action="store_true", help="class-agnostic NMS")
    ap.add_argument("--max-det", type=int, default=None, help="at most this many detections per image")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = dict(synthetic.VOC_CONFIG, seg={"num_classes": a.seg}) if a.seg else synthetic.VOC_CONFIG
    model = yolo(cfg).to(dev).eval()
    for hs in model.yolo_losses:
        hs.val_conf = 0.3
    detect = model
    if a.multi_label or a.agnostic or a.max_det is not None:
        low = 0.001 if a.multi_label else None                                      # the protocol's low thresholds go with multi_label
        detect = Detector(model, PostProcess(conf_thres=low, score_thres=low, multi_label=a.multi_label, agnostic=a.agnostic, max_det=a.max_det))
        print("post-processing:", detect.post)
    classes_name = ["background"] + ["class%d" % i for i in range(1, 21)]          # train.py:57-58
    prep = BatchPrep([(a.size, a.size)], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], device=dev)
    ev = Evaluator(classes_name)
    seg_ev = SegEvaluator(a.seg, device=dev) if a.seg else None
    r = np.random.RandomState(0)
    t0 = time.perf_counter()
    for b in range(0, a.images, a.batch):
        n = min(a.batch, a.images - b)
        sizes = [(int(r.randint(300, 500)), int(r.randint(300, 500))) for _ in range(n)]
        photos = synthetic.photos(sizes, seed=b)                                   # "decoded JPEGs"
        targets = synthetic.targets(n, seed=b + 1, empty_every=8)
        images = prep(photos)                                                      # folder2lmdb.py:223-256 on the device
        out = detect(images)
        if seg_ev is not None:
            out = out[0]                                                           # (dets, seg_out of image 0): the reference's return
            seg_ev.add(model.seg_logits(), id_maps(sizes, a.seg, seed=b + 2))      # all n seg outputs, at each label's own size
        ev.add(out, targets)                                                       # train.py:364-395
    aps, mAP, tp, fp = ev.compute()                                                # train.py:421
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    conf = adjust_confidence(ev.gt_box, ev.pred_box, model.yolo_losses[0].val_conf)   # train.py:417-418
    print("%d images in %.2f s; %d ground-truth boxes, %d detections; mAP %.4f (random weights); next val_conf %.2f" % (
        a.images, dt, ev.gt_box, ev.pred_box, mAP, conf))
    assert len(aps) == 20 and 0.0 <= mAP <= 1.0
    coco = ev.compute_coco(image_size=(a.size, a.size))                            # COCO protocol on the same detections, network input pixels
    print("COCO  " + "  ".join("%s %.4f" % (k, v) for k, v in coco.items() if k != "per_class_AP"))
    assert len(coco["per_class_AP"]) == 20 and all(v == -1 or 0.0 <= v <= 1.0 for k, v in coco.items() if k != "per_class_AP")
    if a.report:
        print_report(ev.compute_report(image_size=(a.size, a.size)), classes_name[1:])
    if seg_ev is not None:
        seg = seg_ev.compute()                                                     # the one host sync of the seg leg
        print("SEG   " + "  ".join("IoU[%s] %.4f" % kv for kv in seg["iou"].items())
              + "  mIoU %.4f  mIoU(fg) %.4f  pixel acc %.4f  (%d pixels, %d ignored)" % (
                  seg["miou"], seg["miou_fg"], seg["pixel_acc"], int(seg_ev.confusion.sum()), int(seg_ev.ignored.item())))
        assert int(seg_ev.confusion.sum()) > 0 and 0.0 <= seg["pixel_acc"] <= 1.0


if __name__ == "__main__":
    main()
