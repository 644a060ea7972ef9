#!/usr/bin/env python3
"""Generate tests/golden/aug_*.npz by running the REAL reference augmentation (utils/image_augmentation.py:
transform_od, Mosaic) from /root/reference in the build container.

Import recipe (as tools/gen_golden.py): stub modules written to a temp dir.  `progress.bar` (utils/__init__.py) and
`cv2` are empty (the functions used here never call them).  torchvision is not installed anywhere, so `torchvision.transforms.functional` is a stub that
restates torchvision's PIL paths over the real Pillow: adjust_brightness / adjust_contrast / adjust_saturation ->
ImageEnhance, adjust_hue -> HSV with np.array(f * 255).astype(np.uint8) wrap, adjust_gamma -> point(), to_tensor,
to_pil_image (mul(255).byte()) and hflip.  get_single_image's box conversions (folder2lmdb.py:113-151) and
collate_fn's resize + normalise (folder2lmdb.py:223-256, Pillow BILINEAR + the torch ops of ToTensor / Normalize) are
restated here; imgaug's `seq` (:131) is out of scope.

Every fixture: random.seed(s), then per group get_single_image for each member (expand only for single-image
groups), Mosaic on a small square canvas for groups of 2-4, then the batch's random.choice(train_img_size).
Recorded: inputs, the uint8 image each sample hands to collate_fn, the normalised batch, the targets, the drawn
size, count, and four random.random() draws taken after the run (the RNG state the planner must leave).

usage: python tools/gen_golden_augment.py   (from the repo root)
"""
import os
import random
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

import torch  # noqa: E402
from PIL import Image  # noqa: E402

from mobilenet_yolo_pytorch_amd import synthetic  # noqa: E402

FUNCTIONAL = '''
import numpy as np
import torch
from PIL import Image, ImageEnhance


def adjust_brightness(img, f):
    return ImageEnhance.Brightness(img).enhance(f)


def adjust_contrast(img, f):
    return ImageEnhance.Contrast(img).enhance(f)


def adjust_saturation(img, f):
    return ImageEnhance.Color(img).enhance(f)


def adjust_hue(img, f):
    if not (-0.5 <= f <= 0.5):
        raise ValueError(f)
    mode = img.mode
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.array(f * 255).astype(np.uint8)
    h = Image.fromarray(np_h, "L")
    return Image.merge("HSV", (h, s, v)).convert(mode)


def adjust_gamma(img, gamma, gain=1):
    mode = img.mode
    img = img.convert("RGB")
    gamma_map = [int((255 + 1 - 1e-3) * gain * pow(ele / 255.0, gamma)) for ele in range(256)] * 3
    return img.point(gamma_map).convert(mode)


def to_tensor(pic):
    img = torch.from_numpy(np.array(pic, np.uint8, copy=True))
    img = img.view(pic.size[1], pic.size[0], len(pic.getbands())).permute((2, 0, 1)).contiguous()
    return img.to(dtype=torch.float32).div(255)


def to_pil_image(pic):
    pic = pic.mul(255).byte()
    npimg = np.transpose(pic.numpy(), (1, 2, 0))
    if npimg.shape[2] == 1:                     # expand_od's all-zero seg map (image_augmentation.py:36) comes through here
        return Image.fromarray(npimg[:, :, 0], "L")
    return Image.fromarray(npimg, "RGB")


def hflip(img):
    return img.transpose(Image.FLIP_LEFT_RIGHT)
'''


def _install_stubs():
    d = tempfile.mkdtemp(prefix="mny_aug_stubs_")
    open(os.path.join(d, "cv2.py"), "w").close()
    os.makedirs(os.path.join(d, "progress"))
    open(os.path.join(d, "progress", "__init__.py"), "w").close()
    with open(os.path.join(d, "progress", "bar.py"), "w") as f:
        f.write("class Bar:\n    def __init__(self,*a,**k): pass\nclass IncrementalBar(Bar): pass\n")
    os.makedirs(os.path.join(d, "torchvision", "transforms"))
    with open(os.path.join(d, "torchvision", "__init__.py"), "w") as f:
        f.write("from . import transforms\n")
    with open(os.path.join(d, "torchvision", "transforms", "__init__.py"), "w") as f:
        f.write("from . import functional\n")
    with open(os.path.join(d, "torchvision", "transforms", "functional.py"), "w") as f:
        f.write(FUNCTIONAL)
    sys.path.insert(0, REF)
    sys.path.insert(0, d)


def get_single_image(aug, photo, target, expand, expand_scale):
    """folder2lmdb.py:113-151 (imgaug seq skipped), around the real transform_od."""
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
    image = Image.fromarray(photo)
    new_img, new_boxes, new_labels, _, _ = aug.transform_od(image, boxes2, labels, difficulties, seg_id=None,
                                                            mean=[0.5, 0.5, 0.5], std=[1, 1, 1], phase="train",
                                                            expand=expand, expand_scale=expand_scale)
    old_dims = torch.FloatTensor([new_img.width, new_img.height, new_img.width, new_img.height]).unsqueeze(0)
    nb = new_boxes / old_dims
    w = nb[..., 2] - nb[..., 0]
    h = nb[..., 3] - nb[..., 1]
    x = (nb[..., 0] + w / 2).unsqueeze(1)
    y = (nb[..., 1] + h / 2).unsqueeze(1)
    nb = torch.cat((x, y, w.unsqueeze(1), h.unsqueeze(1)), 1)
    return new_img, torch.cat((new_labels.unsqueeze(1), nb), 1), []


def collate(pils, size, mean, std):
    out = []
    for im in pils:
        r = im.resize((size[1], size[0]), Image.BILINEAR)
        t = torch.from_numpy(np.asarray(r).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        m, s = torch.as_tensor(mean, dtype=t.dtype), torch.as_tensor(std, dtype=t.dtype)
        out.append(t.sub_(m[:, None, None]).div_(s[:, None, None]))
    return torch.stack(out).numpy()


# name, seed, group sizes, photo size range, expand_scale, canvas, train_img_size, mean, std
CASES = [
    ("aug_singles.npz", 11, [1, 1, 1, 1, 1, 1], (24, 72), 1.5, 160, [[32, 32], [40, 48]], [0.5, 0.5, 0.5], [1, 1, 1]),
    ("aug_mosaic.npz", 12, [2, 3, 4, 1], (24, 72), 1.5, 160, [[32, 32]], [0.5, 0.5, 0.5], [1, 1, 1]),
    ("aug_mix.npz", 13, [4, 1, 2, 1, 3, 1], (20, 64), 1.3, 128, [[32, 40], [48, 32]], [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]),
]


def make_inputs(seed, sizes, lo_hi):
    r = np.random.RandomState(seed)
    n = sum(sizes)
    shapes = [(int(r.randint(*lo_hi)), int(r.randint(*lo_hi))) for _ in range(n)]
    photos = synthetic.photos(shapes, seed=seed)
    tg = [t.numpy() for t in synthetic.targets(n, seed=seed, boxes_per_image=3, empty_every=5)]
    return photos, tg


if __name__ == "__main__":
    _install_stubs()
    from utils.image_augmentation import Image_Augmentation
    aug = Image_Augmentation()
    for name, seed, gsizes, lo_hi, expand_scale, canvas, tsizes, mean, std in CASES:
        photos, tg = make_inputs(seed, gsizes, lo_hi)
        random.seed(seed)
        pils, targets, k = [], [], 0
        for s in gsizes:
            group = []
            for _ in range(s):
                group.append(get_single_image(aug, photos[k], tg[k], s == 1, expand_scale))
                k += 1
            if s == 1:
                pils.append(group[0][0])
                targets.append(group[0][1])
            else:
                b = aug.Mosaic(group, [canvas, canvas])
                pils.append(b[0])
                targets.append(b[1])
        size = random.choice(tsizes)
        after = np.array([random.random() for _ in range(4)])
        arrs = dict(groups=np.array(gsizes), expand_scale=np.float64(expand_scale), canvas=np.int32(canvas),
                    sizes=np.array(tsizes, np.int32), size=np.array(size, np.int32), count=np.int32(sum(gsizes)),
                    mean=np.array(mean, np.float32), std=np.array(std, np.float32), seed=np.int32(seed), after=after,
                    batch=collate(pils, size, mean, std))
        for i, (p, t) in enumerate(zip(photos, tg)):
            arrs["img%d" % i], arrs["tgt%d" % i] = p, t.astype(np.float32).reshape(-1, 5)
        for i, (p, t) in enumerate(zip(pils, targets)):
            arrs["u8_%d" % i], arrs["out_tgt%d" % i] = np.asarray(p).copy(), t.numpy().astype(np.float32).reshape(-1, 5)
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **arrs)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
