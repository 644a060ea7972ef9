"""Oracle (test infrastructure, NOT product): deterministic, name-keyed tensor fill.

Both sides of a parity check (the real reference inside tools/gen_golden.py, the
oracle, and the HIP product in tests) regenerate identical weights from tensor
NAMES, so the 19.7 MB parameter set never has to be committed.
"""
import zlib

import numpy as np
import torch


def _rng(name, salt):
    return np.random.RandomState((zlib.crc32(name.encode()) ^ salt) & 0x7FFFFFFF)


def fill_state_dict_(module, salt=0):
    """Overwrite every parameter/buffer of `module` in place.

    conv weight  : N(0, sqrt(2/fan_in)) — keeps activations O(1) through 50+ layers
    conv bias    : U(-0.1, 0.1)
    BN weight    : U(0.8, 1.2)      BN bias       : U(-0.2, 0.2)
    running_mean : U(-0.1, 0.1)     running_var   : U(0.8, 1.2)
    num_batches_tracked untouched.
    """
    sd = module.state_dict()
    with torch.no_grad():
        for name, t in sd.items():
            r = _rng(name, salt)
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() == 4:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                v = r.standard_normal(t.shape) * np.sqrt(2.0 / fan_in)
            elif name.endswith("running_var"):
                v = r.uniform(0.8, 1.2, t.shape)
            elif name.endswith("running_mean"):
                v = r.uniform(-0.1, 0.1, t.shape)
            elif name.endswith(".bias") and t.dim() == 1 and (name.replace(".bias", ".weight") in sd
                                                             and sd[name.replace(".bias", ".weight")].dim() == 4):
                v = r.uniform(-0.1, 0.1, t.shape)
            elif name.endswith(".weight"):
                v = r.uniform(0.8, 1.2, t.shape)
            else:
                v = r.uniform(-0.2, 0.2, t.shape)
            t.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    return module


def images(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g)


def targets(n, num_classes=20, boxes_per_image=3, seed=1, empty_every=16):
    """SURVEY §8d synthetic targets: label~U{1..C}, cx,cy=0.1+0.8U, w,h=0.05+0.5U;
    every `empty_every`-th image has no boxes."""
    r = np.random.RandomState(seed)
    out = []
    for i in range(n):
        if empty_every and i % empty_every == empty_every - 1:
            out.append(torch.zeros(0, 5))
            continue
        lab = r.randint(1, num_classes + 1, size=(boxes_per_image, 1)).astype(np.float32)
        cxy = (0.1 + 0.8 * r.rand(boxes_per_image, 2)).astype(np.float32)
        wh = (0.05 + 0.5 * r.rand(boxes_per_image, 2)).astype(np.float32)
        out.append(torch.from_numpy(np.concatenate((lab, cxy, wh), 1)))
    return out


def crowded_scene(N, g, spec, seed, num_classes=None, img=352, max_targets=40, counts=None):
    """Seeded crowded batch for one head: -> (head_nchw [N, A*(5+C), g, g], targets list of [n_i,5]).  CPU only.

    Built to enter the branches of the loss that three uniformly placed boxes per image never reach (the counts are
    reported by yolo_ref.loss_branches and asserted in tests/test_oracle_detect.py):
      * images cycle through many targets (min(8,max_targets)..max_targets), many, one, none; `counts` (one int per
        image) overrides the cycle;
      * target shapes: near one anchor / arithmetic mean of two anchors / 0.4 % off their geometric mean (for two nested
        anchors the geometric mean has the same IoU with both, the one shape that can clear iou_thresh against both;
        the 0.4 % keeps the argmax between them decided) / random;
      * with probability 0.35 a second box lands in the same grid cell, half of them with the same label;
      * image 0 also gets one hand-made target per pair of this head's anchors at the pair's geometric mean, so the
        several-anchors-per-target branch is entered on every head;
      * for half of the targets the head's tx,ty,tw,th at the target's cell are overwritten, for every anchor of the head, by
        the logits that decode to the target plus noise 0.1 / 0.15: ignored cells, ignored-then-positive cells, recall hits;
      * the head is otherwise randn * 0.7.
    """
    C = spec.num_classes if num_classes is None else int(num_classes)
    r = np.random.RandomState(seed)
    anch = np.array(spec.anchors, np.float32) / np.float32(img)
    T, A = 5 + C, len(spec.mask)
    head = torch.randn(N, A * T, g, g, generator=torch.Generator().manual_seed(seed)) * 0.7
    hv = head.view(N, A, T, g, g)
    lo = min(8, max_targets)
    out = []
    for n in range(N):
        kind = n % 4
        nt = 0 if kind == 3 else (1 if kind == 2 else r.randint(lo, max_targets + 1))
        if counts is not None:
            nt = int(counts[n])
        rows = []
        while len(rows) < nt:
            cx, cy = 0.02 + 0.96 * r.rand(2)
            a = anch[r.randint(len(anch))]
            mode = r.randint(4)
            if mode == 0:                                             # near one anchor
                w, h = a * (0.8 + 0.4 * r.rand(2))
            elif mode == 1:                                           # between two anchors
                b = anch[r.randint(len(anch))]
                w, h = (a + b) / 2 if r.rand() < 0.5 else np.sqrt(a * b) * (0.996 if r.rand() < 0.5 else 1.004)
            else:
                w, h = 0.03 + 0.6 * r.rand(2)
            lab = r.randint(1, C + 1)
            rows.append([lab, cx, cy, w, h])
            if r.rand() < 0.35 and len(rows) < nt:                    # a second box in the same cell
                fx = (np.floor(cx * g) + 0.1 + 0.8 * r.rand()) / g
                fy = (np.floor(cy * g) + 0.1 + 0.8 * r.rand()) / g
                lab2 = lab if r.rand() < 0.5 else r.randint(1, C + 1)
                rows.append([lab2, fx, fy, w * (0.9 + 0.2 * r.rand()), h * (0.9 + 0.2 * r.rand())])
        if n == 0 and counts is None:
            for i in range(A):
                for j in range(i + 1, A):
                    w, h = np.sqrt(anch[spec.mask[i]] * anch[spec.mask[j]]) * 1.004
                    cx, cy = 0.1 + 0.8 * r.rand(2)
                    rows.append([r.randint(1, C + 1), cx, cy, w, h])
        t = torch.tensor(rows, dtype=torch.float32).reshape(-1, 5)
        out.append(t)
        for q in t.tolist():                                          # make some predictions fit their target
            if r.rand() < 0.5:
                continue
            gi, gj = int(np.float32(q[1]) * np.float32(g)), int(np.float32(q[2]) * np.float32(g))
            for k in range(A):
                aw, ah = anch[spec.mask[k]]
                fx = min(max(q[1] * g - gi, 0.02), 0.98)
                fy = min(max(q[2] * g - gj, 0.02), 0.98)
                hv[n, k, 0, gj, gi] = float(np.log(fx / (1 - fx))) + 0.1 * r.randn()
                hv[n, k, 1, gj, gi] = float(np.log(fy / (1 - fy))) + 0.1 * r.randn()
                hv[n, k, 2, gj, gi] = float(np.log(q[3] / aw)) + 0.15 * r.randn()
                hv[n, k, 3, gj, gi] = float(np.log(q[4] / ah)) + 0.15 * r.randn()
    return head, out


VOC_CONFIG = {
    "img_h": 352, "img_w": 352,
    "iou_weighting": 0.021830872589525777,
    "yolo": {
        "num_classes": 20, "num_anchors": 3,
        "ignore_thresh": [0.6076333316652263, 0.5623606200028424],
        "iou_thresh": 0.5497280113447018,
        "anchors": [[143, 265], [153, 121], [280, 279], [20, 37], [49, 94], [73, 201]],
        "classes": 20,
        "mask": [[0, 1, 2], [3, 4, 5]],
    },
}
