#!/usr/bin/env python3
"""Generate tests/golden/augseg_*.npz by running the REAL reference augmentation with a segmentation id map
(utils/image_augmentation.py transform_od(..., seg_id=...)) from the reference checkout that tools/gen_golden_augment.py names.

Import recipe: that of tools/gen_golden_augment.py (its stub modules, whose to_pil_image handles the one-channel map).
get_single_image's box conversions (folder2lmdb.py:113-151) are restated as there; the seg id map is a PIL 'L' image
of the photo's size, as folder2lmdb.py:99-108 builds it.  collate_fn's cv2.resize is NOT run (cv2 is not installed):
the fixtures pin the geometry half, the id map handed to collate_fn.

Every fixture: random.seed(s), then per sample transform_od with expand on (single-image groups, the only kind a seg
config has).  Recorded: inputs (photo, target, id map), the seed, the `new_seg_id` each sample hands to collate_fn, the
size of the augmented image, the targets, the batch's random.choice(train_img_size), and four random.random() draws
taken after the run (the RNG state the planner must leave).

usage: python tools/gen_golden_augment_seg.py   (from the repo root)
"""
import os
import random
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden_augment as base  # noqa: E402

import torch  # noqa: E402
from PIL import Image  # noqa: E402


def id_map(r, h, w, max_id):
    """Blobs of ids 1..max_id over background 0 (max_id may exceed the config's classes: such ids land in no map)."""
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(int(r.randint(3, 7))):
        cy, cx = r.randint(0, h), r.randint(0, w)
        ry, rx = r.randint(4, max(5, h // 2)), r.randint(4, max(5, w // 2))
        blob = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        m[blob] = r.randint(1, max_id + 1)
    return m


def get_single_image(aug, photo, target, seg, expand_scale):
    """folder2lmdb.py:113-151 (imgaug seq skipped), around the real transform_od with a seg id map."""
    target2 = torch.Tensor(target)
    boxes = target2[..., 1:5]
    if boxes.shape[0] == 0:
        boxes2, labels = torch.zeros(0, 4), torch.zeros(0)
    else:
        x1 = (boxes[..., 0] - boxes[..., 2] / 2).unsqueeze(1)
        y1 = (boxes[..., 1] - boxes[..., 3] / 2).unsqueeze(1)
        x2 = (boxes[..., 0] + boxes[..., 2] / 2).unsqueeze(1)
        y2 = (boxes[..., 1] + boxes[..., 3] / 2).unsqueeze(1)
        boxes2 = torch.cat((x1 * photo.shape[1], y1 * photo.shape[0], x2 * photo.shape[1], y2 * photo.shape[0]), 1)
        labels = target2[..., 0]
    difficulties = torch.zeros_like(labels)
    new_img, new_boxes, new_labels, _, new_seg_id = aug.transform_od(Image.fromarray(photo), boxes2, labels, difficulties,
                                                                     seg_id=Image.fromarray(seg), mean=[0.5, 0.5, 0.5], std=[1, 1, 1],
                                                                     phase="train", expand=True, expand_scale=expand_scale)
    array = np.array(new_seg_id)                                            # folder2lmdb.py:137
    assert array.dtype == np.uint8 and array.shape == (new_img.height, new_img.width)
    old_dims = torch.FloatTensor([new_img.width, new_img.height, new_img.width, new_img.height]).unsqueeze(0)
    nb = new_boxes / old_dims
    w = nb[..., 2] - nb[..., 0]
    h = nb[..., 3] - nb[..., 1]
    x = (nb[..., 0] + w / 2).unsqueeze(1)
    y = (nb[..., 1] + h / 2).unsqueeze(1)
    nb = torch.cat((x, y, w.unsqueeze(1), h.unsqueeze(1)), 1)
    return array, torch.cat((new_labels.unsqueeze(1), nb), 1)


# name, seed, samples, photo size range, expand_scale, train_img_size, seg classes, largest id drawn
CASES = [
    ("augseg_a.npz", 21, 6, (60, 130), 1.3, [[96, 96], [160, 160]], 2, 3),
    ("augseg_b.npz", 22, 5, (64, 120), 1.5, [[96, 96]], 3, 3),
]


if __name__ == "__main__":
    base._install_stubs()
    from utils.image_augmentation import Image_Augmentation
    aug = Image_Augmentation()
    for name, seed, n, lo_hi, expand_scale, tsizes, classes, max_id in CASES:
        photos, tg = base.make_inputs(seed, [1] * n, lo_hi)
        r = np.random.RandomState(seed + 1000)
        segs = [id_map(r, p.shape[0], p.shape[1], max_id) for p in photos]
        random.seed(seed)
        outs = [get_single_image(aug, p, t, s, expand_scale) for p, t, s in zip(photos, tg, segs)]
        size = random.choice(tsizes)
        after = np.array([random.random() for _ in range(4)])
        arrs = dict(expand_scale=np.float64(expand_scale), sizes=np.array(tsizes, np.int32), size=np.array(size, np.int32), count=np.int32(n),
                    seed=np.int32(seed), after=after, seg_classes=np.int32(classes))
        for i, (p, t, s, (new_seg, new_t)) in enumerate(zip(photos, tg, segs, outs)):
            arrs["img%d" % i], arrs["tgt%d" % i], arrs["seg%d" % i] = p, t.astype(np.float32).reshape(-1, 5), s
            arrs["new_seg%d" % i], arrs["out_tgt%d" % i] = new_seg, new_t.numpy().astype(np.float32).reshape(-1, 5)
        path = os.path.join(base.OUT, name)
        np.savez_compressed(path, **arrs)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
