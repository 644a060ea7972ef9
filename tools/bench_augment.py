#!/usr/bin/env python3
"""Device training augmentation throughput (TrainAugment / mny_aug_batch): 256 VOC-shaped photos (500x375 / 375x500)
at 352x352 under the reference's mix (25 % 4-image mosaics on the 1000x1000 canvas, expand on singles), timed
  device : mny_aug_batch alone on already-uploaded images (CUDA events, median of --iters)
  full   : plan + pinned pack + H2D + device (wall clock, synchronised)
next to the Pillow CPU path (the reference's per-sample work: photometric ops, expand/crop/flip via tensors, Mosaic's
bicubic tiles, the BILINEAR resize + normalise) in images/s per core on this host.  Prints one JSON line; `step_share`
is the device time over a --step-ms training step.
usage: python tools/bench_augment.py [--iters 20] [--step-ms 36] [--cpu-samples 16]
       python tools/bench_augment.py --seq      # the blur / sharpen / noise stage (SeqAugment / mny_aug_seq_batch) on the same batch, at the
                                                # reference's draw probabilities, next to mny_aug_batch in the same process (device events, 5 warm-up
                                                # + 200 timed calls, three alternating repeats), plus the batch with every image given one op kind
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from mobilenet_yolo_pytorch_amd import augment, synthetic  # noqa: E402

SIZES = [[352, 352]]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
EXPAND = 2.1610954191879452                              # models/voc/config.yaml


def voc_groups(n, seed=0):
    r = random.Random(seed)
    kinds = [4 if r.random() < 0.25 else 1 for _ in range(n)]
    shapes = [(375, 500) if r.random() < 0.7 else (500, 375) for _ in range(sum(kinds))]
    photos = synthetic.photos(shapes, seed=seed)
    tg = [t.numpy() for t in synthetic.targets(len(photos), seed=seed + 1)]
    groups, k = [], 0
    for s in kinds:
        groups.append([(photos[k + j], tg[k + j]) for j in range(s)])
        k += s
    return groups


def pillow_per_core(groups, n):
    """Per-sample CPU work of the reference pipeline with Pillow + torch (one thread)."""
    from PIL import Image, ImageEnhance
    torch.set_num_threads(1)
    rng = random.Random(1)
    ops = [lambda im, f: ImageEnhance.Brightness(im).enhance(f), lambda im, f: ImageEnhance.Contrast(im).enhance(f),
           lambda im, f: ImageEnhance.Color(im).enhance(f), lambda im, f: im.convert("HSV").convert("RGB"),
           lambda im, f: im.point([int(255.999 * pow(v / 255., f)) for v in range(256)] * 3)]

    def single(photo, expand):
        im = Image.fromarray(photo)
        for op in rng.sample(range(5), 5):
            if rng.random() < 0.5:
                im = ops[op](im, rng.uniform(0.5, 1.5))
        t = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div(255)
        if expand and rng.random() < 0.5:
            s = rng.uniform(1, EXPAND)
            c = torch.full((3, int(s * t.shape[1]), int(s * t.shape[2])), 0.5)
            c[:, :t.shape[1], :t.shape[2]] = t
            t = c
        h, w = t.shape[1], t.shape[2]
        t = t[:, h // 8:h // 8 + 3 * h // 4, w // 8:w // 8 + 3 * w // 4]
        im = Image.fromarray(t.mul(255).byte().permute(1, 2, 0).numpy())
        return im.transpose(Image.FLIP_LEFT_RIGHT) if rng.random() < 0.5 else im

    t0 = time.perf_counter()
    imgs = 0
    for g in groups[:n]:
        if len(g) == 1:
            out = single(g[0][0], True)
        else:
            bg = np.zeros((1000, 1000, 3))
            for k, (p, _) in enumerate(g):
                tile = np.array(single(p, False).resize((500, 500)))
                y, x = (k // 2) * 500, (k % 2) * 500
                bg[y:y + 500, x:x + 500] = np.mean(tile, axis=(0, 1))
                bg[y:y + 500, x:x + 500] = tile
            out = Image.fromarray(bg.astype(np.uint8))
        r = out.resize((352, 352), Image.BILINEAR)
        x = torch.from_numpy(np.array(r)).permute(2, 0, 1).float().div(255)
        (x - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]
        imgs += 1
    return imgs / (time.perf_counter() - t0)


def timed(fn, warm=5, calls=200):
    """Mean ms per call between two device events."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def seq_leg(aug, plan, src):
    seq = augment.SeqAugment(seed=0)
    items = plan["items"]
    rec = seq.plan(len(items))
    px3 = 3 * items["h"].astype(np.int64) * items["w"]
    moved = lambda r: int((2 * px3 * np.maximum(r["n_ops"], 1)).sum())          # every pass reads and writes the image once
    out = aug.run_device(src, plan)
    seq.run_device(src, items, rec)
    seq.check()
    aug.check()
    t_seq, t_aug = [], []
    for _ in range(3):
        t_seq.append(timed(lambda: seq.run_device(src, items, rec)))
        t_aug.append(timed(lambda: aug.run_device(src, plan, out=out)))
    seq_ms, aug_ms = float(np.median(t_seq)), float(np.median(t_aug))
    res = {"images": len(items), "seq_ms": round(seq_ms, 4), "seq_ms_repeats": [round(t, 4) for t in t_seq], "aug_batch_ms": round(aug_ms, 4),
           "aug_batch_ms_repeats": [round(t, 4) for t in t_aug], "seq_over_aug": round(seq_ms / aug_ms, 4), "bytes_moved": moved(rec),
           "GB_s": round(moved(rec) / seq_ms / 1e6, 1), "ops": {str(k): int((rec["n_ops"] == k).sum()) for k in (0, 1, 2)}}
    kinds = {"copy": [], "gauss": [(augment.SEQ_GAUSS, 0.7)], "median3": [(augment.SEQ_MEDIAN, 3)], "median5": [(augment.SEQ_MEDIAN, 5)],
             "sharpen": [(augment.SEQ_SHARPEN, 0.05, 1.0)], "noise": [(augment.SEQ_NOISE, 4.0, True, 12345)]}
    for name, ops in kinds.items():                                             # which op costs what: the whole batch under one kind
        r = augment.seq_records([ops] * len(items))
        ms = timed(lambda: seq.run_device(src, items, r), calls=100)
        res["all_" + name + "_ms"] = round(ms, 4)
        res["all_" + name + "_GB_s"] = round(moved(r) / ms / 1e6, 1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=36.0)
    ap.add_argument("--cpu-samples", type=int, default=16)
    ap.add_argument("--seq", action="store_true", help="measure the blur / sharpen / noise stage next to mny_aug_batch and exit")
    a = ap.parse_args()
    groups = voc_groups(256)
    aug = augment.TrainAugment(SIZES, MEAN, STD, EXPAND, rng=random.Random(0))
    plan = aug.plan(groups)
    stage, offsets = aug.pack(groups)
    plan["items"]["offset"] = offsets
    src = stage.to("cuda:0")
    if a.seq:
        return seq_leg(aug, plan, src)
    out = aug.run_device(src, plan)
    aug.check()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        aug.run_device(src, plan, out=out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(times))
    walls = []
    for _ in range(max(3, a.iters // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug(groups, size=(352, 352))
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    full_ms = float(np.median(walls))
    cpu = pillow_per_core(groups, a.cpu_samples)
    print(json.dumps({"samples": len(groups), "images": plan["count"], "mosaics": plan["n_mosaic"], "device_ms": round(dev_ms, 3),
                      "device_img_s": round(len(groups) / dev_ms * 1e3, 1), "full_ms": round(full_ms, 2),
                      "full_img_s": round(len(groups) / full_ms * 1e3, 1), "step_share": round(dev_ms / a.step_ms, 4),
                      "pillow_img_s_per_core": round(cpu, 1)}))


if __name__ == "__main__":
    main()
