"""Device-side training augmentation — the train-phase sample path of the reference's data pipeline after decoding:
per image `transform_od` (utils/image_augmentation.py:279-334: photometric_distort, expand_od, random_crop_od, flip_od),
for groups of 2-4 images `Mosaic` (:216-278), then `collate_fn`'s resize + normalise (folder2lmdb.py:223-265).

`TrainAugment.plan` makes every random draw on the host, consuming the RNG in exactly the reference's order (per
group, per member: photometric -> expand gate -> expand -> crop loop -> flip; then the mosaic draws; the batch's size
choice last), and does the box maths with the same torch CPU fp32 ops, so targets are bit-equal.  `__call__` packs the
decoded uint8 images into one pinned upload and runs `mny_aug_batch` (csrc/augment.hip): photometric chain, geometry,
mosaic canvas and the final BILINEAR resize + Normalize, bit for bit against Pillow.

Configs with a `seg:` section (`seg_classes`): every group member also carries its uint8 id map.  The map makes the
image's geometric trip (expand border 0, crop, flip; no draw of its own, so the plan, the targets and the RNG state are
those of a plain instance) and `mny_aug_seg_batch` builds collate_fn's per-class maps on the S/16 grid
(folder2lmdb.py:135-141,243-261).  The geometry is pinned to the reference; the cv2 INTER_AREA resize is restated from
OpenCV's source (cv2 is not available to pin it), see include/mnyolo.h.  The reference defines no Mosaic with seg maps.

`SeqAugment` is the stage in front of all that: imgaug's `seq` (folder2lmdb.py:28-42), which the reference runs on every
decoded image before `transform_od` (:131): with probability 0.5 one or two of {Gaussian or median blur, sharpen, additive
Gaussian noise} in random order.  `SeqAugment.plan` draws from a numpy Generator of its own (imgaug does too; Python's
`random` is never touched, so TrainAugment's draws are those of a seq-less instance) and `mny_aug_seq_batch`
(csrc/augseq.hip) applies the ops uint8 -> uint8 on the packed upload; `TrainAugment(..., seq=SeqAugment(seed))` runs it
between the upload and `mny_aug_batch`.  Neither imgaug nor cv2 is available to pin it: like the INTER_AREA resize this
stage is parity-unpinned against the third-party libraries, the arithmetic stated in include/mnyolo.h is the specification
(tests/seq_ref.py restates it with numpy and scipy).  The reference applies `seq` in the test phase as well (line 131 has
no phase check); `SeqAugment.run_device` in front of `BatchPrep.run_device` reproduces that quirk for whoever wants it, it
is not a default.

`RandomPerspective` is a stage the reference does not have: YOLOv5's random_perspective (rotation, scale jitter, shear,
translation, perspective).  `TrainAugment(..., warp=RandomPerspective(seed))` runs it after `seq` and before `mny_aug_batch`:
`mny_aug_warp_batch` (csrc/augwarp.hip) gathers every decoded image through its inverse map, uint8 -> uint8 at source
resolution, and the targets go through the forward matrix before `_member` sees them; the id maps of a seg config take the
same coefficients.  Its draws come from a numpy Generator of its own.  The pixels equal Pillow's Image.transform(PERSPECTIVE)
byte for byte (tests/warp_ref.py, pinned in tests/test_warp_ref_cpu.py).

With `decoder` (a jpeg.JpegDecoder) the members carry the encoded JPEG streams in place of the decoded arrays: the decoder
fills the packed buffer on the device (host entropy decode, HIP pixels) and the plan is made from the decoded sizes; draws,
targets and the state of `rng` are those of the array path.  Seg id maps are not JPEG and stay decoded by the caller.

Not covered (stays with the caller): the sampler, and the scale < 1 path of the area resize (a cropped
geometry smaller than the S/16 grid is refused).  No CPU fallback: without libmnyolo.so every call raises MnyError."""
import ctypes
import math
import random

import numpy as np
import torch

from ._lib import call, query
from .prep import DESC, BatchPrep, all_encoded

BRIGHTNESS, CONTRAST, SATURATION, HUE, GAMMA = range(5)      # MNY_AUG_*; image_augmentation.py:178-182 order

ITEM = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32), ("n_ops", np.int32), ("op", np.int32, 5),
                 ("factor", np.float32, 5), ("hue_shift", np.int32), ("gamma_map", np.uint8, 256),
                 ("exp", np.int32, 4), ("crop", np.int32, 4), ("flip", np.int32), ("sample", np.int32),
                 ("tile", np.int32, 4), ("mask", np.int32, 4)], align=True)                     # mny_aug_item
SAMPLE = np.dtype([("first_item", np.int32), ("n_items", np.int32), ("canvas_slot", np.int32), ("reserved", np.int32)])
assert ITEM.itemsize == 392 and SAMPLE.itemsize == 16
SEG_MAX_CLASSES = 8                                           # MNY_AUG_SEG_MAX_CLASSES
SEQ_GAUSS, SEQ_MEDIAN, SEQ_SHARPEN, SEQ_NOISE = range(4)      # MNY_SEQ_*
SEQ = np.dtype([("n_ops", np.int32), ("op", np.int32, 2), ("taps", np.float32, 5), ("median_k", np.int32), ("sharpen_c", np.float32),
                ("sharpen_s", np.float32), ("noise_scale", np.float32), ("noise_per_channel", np.int32), ("noise_key", np.uint32, 2),
                ("reserved", np.int32)])                                                          # mny_aug_seq_item
assert SEQ.itemsize == 64
WARP = np.dtype([("c", np.float64, 8), ("identity", np.int32), ("fill", np.uint8, 3), ("reserved", np.uint8)])   # mny_aug_warp_item
assert WARP.itemsize == 72
SEQ_SIGMA_MIN = 1e-3                                          # imgaug GaussianBlur: a sigma below this is the identity


def hue_shift_u8(f):
    """torchvision adjust_hue: np.array(f * 255).astype(np.uint8) — truncate toward zero, wrap mod 256."""
    return int(math.trunc(f * 255.0)) % 256


def gamma_map(g):
    """torchvision adjust_gamma (gain 1): the point() table."""
    return np.array([int((255 + 1 - 1e-3) * 1 * pow(v / 255.0, g)) for v in range(256)], np.uint8)


def _jaccard(set_1, set_2):
    """utils/iou.py find_jaccard_overlap, the same torch ops in the same order."""
    lower = torch.max(set_1[:, :2].unsqueeze(1), set_2[:, :2].unsqueeze(0))
    upper = torch.min(set_1[:, 2:].unsqueeze(1), set_2[:, 2:].unsqueeze(0))
    dims = torch.clamp(upper - lower, min=0)
    inter = dims[:, :, 0] * dims[:, :, 1]
    a1 = (set_1[:, 2] - set_1[:, 0]) * (set_1[:, 3] - set_1[:, 1])
    a2 = (set_2[:, 2] - set_2[:, 0]) * (set_2[:, 3] - set_2[:, 1])
    return inter / (a1.unsqueeze(1) + a2.unsqueeze(0) - inter)


def gauss_taps(sigma):
    """The five taps exp(-d^2 / 2 sigma^2), d = -2..2, normalised in fp64, as fp32."""
    d = np.arange(-2, 3, dtype=np.float64)
    t = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).astype(np.float32)


def sharpen_coeffs(alpha, lightness):
    """imgaug Sharpen: (1 - alpha) * identity + alpha * [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]] -> (centre, neighbour) as fp32."""
    a, l = float(alpha), float(lightness)
    return np.float32((1.0 - a) + a * (8.0 + l)), np.float32(-a)


def seq_records(op_lists):
    """Per image a list of at most two ops -> SEQ array.  An op is (SEQ_GAUSS, sigma), (SEQ_MEDIAN, k), (SEQ_SHARPEN, alpha,
    lightness) or (SEQ_NOISE, scale, per_channel, key); a Gaussian with sigma < 1e-3 is the identity and is dropped."""
    rec = np.zeros(len(op_lists), SEQ)
    rec["median_k"] = 3
    for r, ops in zip(rec, op_lists):
        ops = [o for o in ops if not (o[0] == SEQ_GAUSS and o[1] < SEQ_SIGMA_MIN)]
        if len(ops) > 2 or len({o[0] for o in ops}) != len(ops):
            raise ValueError("an image takes at most two ops of different kinds, got %r" % (ops,))
        r["n_ops"] = len(ops)
        for k, o in enumerate(ops):
            r["op"][k] = o[0]
            if o[0] == SEQ_GAUSS:
                r["taps"] = gauss_taps(o[1])
            elif o[0] == SEQ_MEDIAN:
                if o[1] not in (3, 5):
                    raise ValueError("median size must be 3 or 5, got %r" % (o[1],))
                r["median_k"] = o[1]
            elif o[0] == SEQ_SHARPEN:
                r["sharpen_c"], r["sharpen_s"] = sharpen_coeffs(o[1], o[2])
            elif o[0] == SEQ_NOISE:
                r["noise_scale"], r["noise_per_channel"] = o[1], int(bool(o[2]))
                r["noise_key"] = (int(o[3]) & 0xffffffff, (int(o[3]) >> 32) & 0xffffffff)
            else:
                raise ValueError("unknown op %r" % (o[0],))
    return rec


class SeqAugment:
    """seq = SeqAugment(seed)                       # the reference's imgaug `seq`, folder2lmdb.py:28-42
       dst = seq.run_device(src, desc, seq.plan(len(desc)))     # src: the packed uint8 upload; dst: the same layout
    or TrainAugment(..., seq=seq), which does exactly that between the upload and mny_aug_batch.  The draws come from a
    numpy Generator owned by the instance, never from Python's `random`.  Per image, each draw a vector over the batch, in
    this order: (1) gate < p; (2) count in {1, 2}; (3) a permutation of the children (blur, sharpen, noise), the first
    `count` run in that order; (4) blur kind, Gaussian or median at 1/2 each; (5) sigma ~ U(0, 1), then k from {3, 4, 5}
    with an even draw raised to the next odd (imgaug MedianBlur); (6) alpha ~ U(0, 0.1); (7) lightness ~ U(0.9, 1.1); (8) the
    per-channel flag at 0.3; (9) scale ~ U(0, 0.03 * 255); (10) a 64-bit noise key.  Every vector is drawn whether or not an
    image uses it, so plan() is a function of the seed and the batch sizes alone."""
    CHILDREN = ("blur", "sharpen", "noise")

    def __init__(self, seed=None, p=0.5, device="cuda:0"):
        self.gen = np.random.Generator(np.random.PCG64(seed))
        self.p = float(p)
        self.device = torch.device(device)
        self._fixed = None
        self._status = None

    @classmethod
    def fixed(cls, records, device="cuda:0"):
        """Explicit per-image ops in place of the draws: a SEQ array or the op lists seq_records() takes."""
        self = cls(0, device=device)
        self._fixed = records.copy() if isinstance(records, np.ndarray) and records.dtype == SEQ else seq_records(records)
        return self

    def draw(self, n_images):
        """The raw draws of one batch, in the documented order (host only)."""
        g, n = self.gen, int(n_images)
        d = dict(gate=g.random(n) < self.p)
        d["count"] = g.integers(1, 3, n)
        d["order"] = np.argsort(g.random((n, 3)), axis=1)
        d["gauss"] = g.random(n) < 0.5
        d["sigma"] = g.uniform(0.0, 1.0, n)
        k = g.integers(3, 6, n)
        d["k"] = k + (k % 2 == 0)
        d["alpha"] = g.uniform(0.0, 0.1, n)
        d["lightness"] = g.uniform(0.9, 1.1, n)
        d["per_channel"] = g.random(n) < 0.3
        d["scale"] = g.uniform(0.0, 0.03 * 255, n)
        d["key"] = g.integers(0, 2 ** 64, n, dtype=np.uint64)
        return d

    @staticmethod
    def records(d):
        """draw() -> SEQ array."""
        ops = []
        for i in range(len(d["gate"])):
            chain = []
            if d["gate"][i]:
                for child in d["order"][i][:d["count"][i]]:
                    if child == 0:
                        chain.append((SEQ_GAUSS, float(d["sigma"][i])) if d["gauss"][i] else (SEQ_MEDIAN, int(d["k"][i])))
                    elif child == 1:
                        chain.append((SEQ_SHARPEN, float(d["alpha"][i]), float(d["lightness"][i])))
                    else:
                        chain.append((SEQ_NOISE, float(d["scale"][i]), bool(d["per_channel"][i]), int(d["key"][i])))
            ops.append(chain)
        return seq_records(ops)

    def plan(self, n_images):
        """Host only: the SEQ record of each of the batch's n_images decoded images."""
        if self._fixed is not None:
            if len(self._fixed) != n_images:
                raise ValueError("fixed records describe %d images, the batch holds %d" % (len(self._fixed), n_images))
            return self._fixed
        return self.records(self.draw(n_images))

    def run_device(self, src, desc_or_items, plan):
        """src: the packed uint8 images on the device; desc_or_items: their DESC array (prep.py) or TrainAugment's ITEM array with
        the offsets set; plan: plan(len(desc)).  -> dst, laid out like src, every image in it."""
        n = len(desc_or_items)
        if len(plan) != n or plan.dtype != SEQ:
            raise ValueError("the plan must hold one SEQ record per image")
        desc = np.zeros(n, DESC)
        for f in ("offset", "h", "w"):
            desc[f] = desc_or_items[f]
        max_h, max_w = int(desc["h"].max()), int(desc["w"].max())
        nbytes = int(src.numel())
        size = query("mny_aug_seq_ws_bytes", n, nbytes, max_h, max_w)
        if size == 0:
            raise ValueError("mny_aug_seq_ws_bytes refused n=%d bytes=%d max %dx%d" % (n, nbytes, max_h, max_w))
        dev = src.device                                       # the stage runs where the upload is
        ws = torch.empty(size, device=dev, dtype=torch.uint8)
        dst = torch.empty_like(src)
        d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        s_dev = torch.from_numpy(np.ascontiguousarray(plan).view(np.uint8).copy()).to(dev, non_blocking=True)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_aug_seq_batch", p(src), p(d_dev), p(s_dev), n, max_h, max_w, p(dst), p(ws), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        self._status = ws[:4].view(torch.int32)
        self._keep = (src, d_dev, s_dev, ws)
        return dst

    def check(self):
        """Host sync: raise if the last batch held a malformed image descriptor or record."""
        if self._status is not None:
            v = int(self._status.item())
            if v > 0:
                raise RuntimeError("seq augment: image %d is misaligned, outside the declared maximum or carries a malformed record" % (v - 1))


def warp_matrix(h, w, degrees=0.0, scale=1.0, shear_x=0.0, shear_y=0.0, tx=0.5, ty=0.5, px=0.0, py=0.0):
    """YOLOv5's random_perspective composition M = T . S . R . P . C (fp64), forward: source -> output.  Angles in degrees, tx / ty
    the fractions of the width / height at which the centre lands (0.5 = stays)."""
    C, P, R, S, T = (np.eye(3) for _ in range(5))
    C[0, 2], C[1, 2] = -w / 2, -h / 2
    P[2, 0], P[2, 1] = px, py
    a = math.radians(degrees)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = scale * math.cos(a), scale * math.sin(a), -scale * math.sin(a), scale * math.cos(a)
    S[0, 1], S[1, 0] = math.tan(math.radians(shear_x)), math.tan(math.radians(shear_y))
    T[0, 2], T[1, 2] = tx * w, ty * h
    return T @ S @ R @ P @ C


def warp_coeffs(M):
    """Forward 3x3 -> the eight coefficients of the inverse map, output -> source, the ninth normalised to 1 (what Pillow's
    Image.transform(..., PERSPECTIVE, c) takes).  ValueError for a matrix that is not finite or not invertible."""
    M = np.asarray(M, np.float64)
    if M.shape != (3, 3) or not np.isfinite(M).all():
        raise ValueError("a warp matrix must be a finite 3x3, got %r" % (M,))
    if np.linalg.det(M) == 0:
        raise ValueError("the warp matrix is singular: %r" % (M,))
    inv = np.linalg.inv(M)
    with np.errstate(all="ignore"):
        c = (inv / inv[2, 2]).reshape(9)[:8]
    if M[2, 0] == 0 and M[2, 1] == 0:
        c[6] = c[7] = 0.0                                         # the inverse of an affine map is affine, whatever the solver's rounding
    if not np.isfinite(c).all():
        raise ValueError("the inverse of the warp matrix cannot be normalised (its last entry is %r): %r" % (inv[2, 2], M))
    return c


class RandomPerspective:
    """warp = RandomPerspective(seed)               # YOLOv5's random_perspective, defaults of hyp.scratch-low
       plan = warp.plan([(h, w), ...])              # host: WARP records, forward matrices, identity flags
       dst = warp.run_device(src, desc, plan, channels=3)       # src: the packed uint8 upload; dst: the same layout
       target = warp.boxes(target, plan["matrices"][i], h, w)   # host: the [n,5] cls,cx,cy,w,h rows of image i
    or TrainAugment(..., warp=warp), which runs it after `seq` and before mny_aug_batch, on the id maps of a seg config too.
    The reference has no such stage; the arithmetic in include/mnyolo.h is the specification and equals Pillow's
    Image.transform(PERSPECTIVE) byte for byte (BILINEAR, fill 127 for images; NEAREST, fill 0 for id maps).
    The draws come from a numpy Generator owned by the instance, never from Python's `random`.  Each draw is a vector over the
    batch, drawn whether used or not, in this order: (1) gate < p; (2) a ~ U(-degrees, degrees); (3) s ~ U(1 - scale, 1 + scale);
    (4) shx, (5) shy ~ U(-shear, shear), degrees; (6) tx, (7) ty ~ U(0.5 - translate, 0.5 + translate); (8) px, (9) py ~
    U(-perspective, perspective).  The draws are a function of the seed and the batch size alone.  A gated-off image, and one
    whose matrix equals the identity exactly, is an identity item: its bytes are copied and its targets left alone."""
    FILL = (127, 127, 127)                                        # expand_od's filler

    def __init__(self, seed=None, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, p=1.0, device="cuda:0"):
        self.gen = np.random.Generator(np.random.PCG64(seed))
        self.degrees, self.translate, self.scale = float(degrees), float(translate), float(scale)
        self.shear, self.perspective, self.p = float(shear), float(perspective), float(p)
        self.device = torch.device(device)
        self._fixed = None
        self._status = {}
        self._keep = {}

    @classmethod
    def fixed(cls, matrices, device="cuda:0"):
        """Explicit forward 3x3 matrices (source -> output), one per image, in place of the draws.  A matrix that is not finite or
        not invertible raises ValueError here; the denominator at the image's corners is checked by plan(), which knows the sizes."""
        self = cls(0, device=device)
        ms = np.array([np.asarray(m, np.float64) for m in matrices], np.float64).reshape(-1, 3, 3)
        for i, m in enumerate(ms):
            try:
                warp_coeffs(m)
            except ValueError as e:
                raise ValueError("image %d: %s" % (i, e)) from None
        self._fixed = ms
        return self

    def draw(self, n_images):
        """The raw draws of one batch, in the documented order (host only)."""
        g, n = self.gen, int(n_images)
        d = dict(gate=g.random(n) < self.p)
        d["a"] = g.uniform(-self.degrees, self.degrees, n)
        d["s"] = g.uniform(1 - self.scale, 1 + self.scale, n)
        d["shx"] = g.uniform(-self.shear, self.shear, n)
        d["shy"] = g.uniform(-self.shear, self.shear, n)
        d["tx"] = g.uniform(0.5 - self.translate, 0.5 + self.translate, n)
        d["ty"] = g.uniform(0.5 - self.translate, 0.5 + self.translate, n)
        d["px"] = g.uniform(-self.perspective, self.perspective, n)
        d["py"] = g.uniform(-self.perspective, self.perspective, n)
        return d

    @staticmethod
    def matrices(d, sizes):
        """draw() and the (h, w) of every image -> forward matrices [n,3,3]; a gated-off image gets the identity."""
        out = np.tile(np.eye(3), (len(sizes), 1, 1))
        for i, (h, w) in enumerate(sizes):
            if d["gate"][i]:
                out[i] = warp_matrix(h, w, d["a"][i], d["s"][i], d["shx"][i], d["shy"][i], d["tx"][i], d["ty"][i], d["px"][i], d["py"][i])
        return out

    def plan(self, sizes):
        """Host only.  sizes: the (h, w) of each of the batch's decoded images -> dict(records WARP array, matrices [n,3,3] forward,
        identity bool [n]).  ValueError naming the image whose forward denominator is not positive at its four corners."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        if self._fixed is not None:
            if len(self._fixed) != len(sizes):
                raise ValueError("fixed matrices describe %d images, the batch holds %d" % (len(self._fixed), len(sizes)))
            ms = self._fixed.copy()
        else:
            ms = self.matrices(self.draw(len(sizes)), sizes)
        rec = np.zeros(len(sizes), WARP)
        rec["fill"] = self.FILL
        ident = np.zeros(len(sizes), bool)
        for i, ((h, w), m) in enumerate(zip(sizes, ms)):
            ident[i] = bool(np.array_equal(m, np.eye(3)))
            if ident[i]:
                rec["c"][i] = (1, 0, 0, 0, 1, 0, 0, 0)
                continue
            den = [m[2, 0] * x + m[2, 1] * y + m[2, 2] for x, y in ((0, 0), (w, 0), (0, h), (w, h))]
            if not min(den) > 0:
                raise ValueError("image %d: the warp's denominator is not positive at every corner of the %dx%d image (%s); the "
                                 "perspective terms are too large for this size" % (i, h, w, ", ".join("%g" % v for v in den)))
            try:
                rec["c"][i] = warp_coeffs(m)
            except ValueError as e:
                raise ValueError("image %d: %s" % (i, e)) from None
        rec["identity"] = ident
        return dict(records=rec, matrices=ms, identity=ident)

    @staticmethod
    def boxes(target, M, h, w):
        """[n,5] cls,cx,cy,w,h (normalised) of an image of size (h, w) under the forward matrix M -> float32 [k,5]: the corners go
        through M, the new box is their min / max clipped to the image; kept iff wider and higher than 2 px, aspect under 100 and
        more than 0.1 of the area the map gives the whole box."""
        t = np.asarray(target, np.float64).reshape(-1, 5)
        M = np.asarray(M, np.float64)
        x1, y1 = (t[:, 1] - t[:, 3] / 2) * w, (t[:, 2] - t[:, 4] / 2) * h
        x2, y2 = (t[:, 1] + t[:, 3] / 2) * w, (t[:, 2] + t[:, 4] / 2) * h
        xs, ys = np.stack([x1, x2, x1, x2], 1), np.stack([y1, y2, y2, y1], 1)
        with np.errstate(all="ignore"):
            den = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
            X = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / den
            Y = (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / den
            nx1, nx2 = np.clip(X.min(1), 0, w), np.clip(X.max(1), 0, w)
            ny1, ny2 = np.clip(Y.min(1), 0, h), np.clip(Y.max(1), 0, h)
            nw, nh = nx2 - nx1, ny2 - ny1
            area = (x2 - x1) * (y2 - y1)
            det = abs(M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
            keep = (nw > 2) & (nh > 2) & (np.maximum(nw / nh, nh / nw) < 100) & (nw * nh / (area * det + 1e-16) > 0.1)
        out = np.stack([t[:, 0], (nx1 + nx2) / 2 / w, (ny1 + ny2) / 2 / h, nw / w, nh / h], 1)
        return out[keep].astype(np.float32)

    def run_device(self, src, desc_or_items, plan, channels=3):
        """src: the packed uint8 images (channels 3, BILINEAR, fill 127) or id maps (channels 1, NEAREST, fill 0) on the device;
        desc_or_items: their DESC array (prep.py) or TrainAugment's ITEM array with the offsets set; plan: plan(sizes) or its
        records.  -> dst, laid out like src, every image in it."""
        rec = plan["records"] if isinstance(plan, dict) else plan
        n = len(desc_or_items)
        if channels not in (1, 3):
            raise ValueError("channels must be 3 (RGB images) or 1 (id maps), got %r" % (channels,))
        if not isinstance(rec, np.ndarray) or rec.dtype != WARP or len(rec) != n:
            raise ValueError("the plan must hold one WARP record per image")
        if channels == 1:
            rec = rec.copy()
            rec["fill"] = 0                                     # background
        desc = np.zeros(n, DESC)
        for f in ("offset", "h", "w"):
            desc[f] = desc_or_items[f]
        max_h, max_w = int(desc["h"].max()), int(desc["w"].max())
        size = query("mny_aug_warp_ws_bytes", n, channels, max_h, max_w)
        if size == 0:
            raise ValueError("mny_aug_warp_ws_bytes refused n=%d channels=%d max %dx%d" % (n, channels, max_h, max_w))
        dev = src.device                                       # the stage runs where the upload is
        ws = torch.empty(size, device=dev, dtype=torch.uint8)
        dst = torch.empty_like(src)
        d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        w_dev = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).to(dev, non_blocking=True)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_aug_warp_batch", p(src), p(d_dev), p(w_dev), n, channels, max_h, max_w, p(dst), p(ws), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        self._status[channels] = ws[:4].view(torch.int32)
        self._keep[channels] = (src, d_dev, w_dev, ws)
        return dst

    def check(self):
        """Host sync: raise if the last batch (its images or its id maps) held a malformed descriptor or record."""
        for channels, st in sorted(self._status.items(), reverse=True):
            v = int(st.item())
            if v > 0:
                raise RuntimeError("warp augment: %s %d is misaligned, outside the declared maximum or carries a non-finite coefficient"
                                   % ("image" if channels == 3 else "seg map", v - 1))


class TrainAugment:
    """aug = TrainAugment.from_config(config)
       images, targets, count = aug(groups)     # groups: [[(uint8 HWC RGB array, target [n,5] cls,cx,cy,w,h)] * 1..4]
    -> images [N,3,H,W] fp32 on `device`, targets a list of CPU [n,5] float32, count = number of decoded images.
    With `seg_classes` (a config with a `seg:` section) a member is (image, target, seg_id), seg_id the uint8 [h,w] id
    map of the image, groups hold one image, and the call returns collate_fn's train-phase tuple
       images, targets, count, seg_maps = aug(groups)     # seg_maps [N,H/16,W/16,seg_classes] fp32 on `device`
    ready for model(images, targets, seg_maps).
    With `seq` (a SeqAugment) the decoded images pass through the blur / sharpen / noise stage on the device first; the id
    maps of a seg config do not (folder2lmdb.py:131).  Targets, count and the state of `rng` are those of seq=None.
    With `decoder` (a jpeg.JpegDecoder) a member's first entry may be its encoded JPEG stream (bytes-like or a 1-D uint8
    array); a batch holds streams or arrays, not both.
    With `warp` (a RandomPerspective) every decoded image is rotated / scaled / sheared / translated / projected at source
    resolution after `seq`, its target goes through the same matrix before the reference's chain sees it, and the id map of a
    seg config takes the image's coefficients (NEAREST, border 0).  `rng` is not touched: its draws are those of warp=None on
    the transformed targets, and an all-identity warp changes nothing."""

    def __init__(self, train_img_size, mean, std, expand_scale, canvas=1000, device="cuda:0", rng=random, seg_classes=None, seq=None, decoder=None,
                 warp=None):
        self.sizes = [tuple(int(v) for v in s) for s in train_img_size]
        self.mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self.std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self.expand_scale = float(expand_scale)
        self.canvas = int(canvas)                   # folder2lmdb.py:172 Mosaic(group, [1000, 1000]); square only
        self.device = torch.device(device)
        self.rng = rng                              # the reference draws from the global `random`
        self._packer = BatchPrep(self.sizes, [0, 0, 0], [1, 1, 1], device=device)
        self._status = None
        self.seg_classes = None if seg_classes is None else int(seg_classes)
        if self.seg_classes is not None:
            if not 1 <= self.seg_classes <= SEG_MAX_CLASSES:
                raise ValueError("seg_classes must be 1..%d, got %d" % (SEG_MAX_CLASSES, self.seg_classes))
            if any(h != w for h, w in self.sizes):                         # folder2lmdb.py:244-247 holds for square sizes only
                raise ValueError("seg maps need square train_img_size entries, got %s" % (self.sizes,))
        self._seg_stage = None                      # pinned staging buffer of the id maps, grown on demand
        self._seg_status = None
        self.seq = seq
        self.decoder = decoder
        self.warp = warp

    @classmethod
    def from_config(cls, cfg, **kw):
        if "seg" in cfg:
            # train.py:114 hands config["mosaic_num"] to the sampler as the group sizes; Mosaic drops the seg maps and
            # collate_fn then indexes b[3], so a seg config has to switch Mosaic off itself (models/bdd100k: mosaic_num [1])
            sizes = cfg.get("mosaic_num")
            sizes = [sizes] if isinstance(sizes, int) else sizes
            if not sizes or any(int(v) != 1 for v in sizes):
                raise ValueError("TrainAugment: a config with a `seg:` section must set mosaic_num: [1] (the reference defines no Mosaic "
                                 "with seg maps), got mosaic_num=%r" % (cfg.get("mosaic_num"),))
            kw.setdefault("seg_classes", cfg["seg"]["num_classes"])
        return cls(cfg["train_img_size"], cfg["normalize"]["mean"], cfg["normalize"]["std"], cfg["expand_scale"], **kw)

    # ---- host planning (no GPU) -------------------------------------------------------------------------------------
    def _member(self, h, w, target, expand):
        """folder2lmdb.py get_single_image around transform_od for one decoded image of size (h, w)."""
        rng = self.rng
        t2 = torch.Tensor(np.asarray(target, np.float32).reshape(-1, 5))
        boxes = t2[..., 1:5]
        if boxes.shape[0] == 0:
            boxes2, labels = torch.zeros(0, 4), torch.zeros(0)
        else:
            x1 = (boxes[..., 0] - boxes[..., 2] / 2).unsqueeze(1)
            y1 = (boxes[..., 1] - boxes[..., 3] / 2).unsqueeze(1)
            x2 = (boxes[..., 0] + boxes[..., 2] / 2).unsqueeze(1)
            y2 = (boxes[..., 1] + boxes[..., 3] / 2).unsqueeze(1)
            boxes2 = torch.cat((x1 * w, y1 * h, x2 * w, y2 * h), 1)
            labels = t2[..., 0]
        order = [BRIGHTNESS, CONTRAST, SATURATION, HUE, GAMMA]           # photometric_distort
        rng.shuffle(order)
        chain = []
        for op in order:
            if rng.random() < 0.5:
                chain.append((op, rng.uniform(-18 / 255., 18 / 255.) if op == HUE else rng.uniform(0.5, 1.5)))
        exp = (h, w, 0, 0)                                                  # expand_od: (new_h, new_w, top, left)
        if rng.random() < 0.5 and expand:
            scale = rng.uniform(1, self.expand_scale)
            nh, nw = int(scale * h), int(scale * w)
            left = rng.randint(0, nw - w)
            top = rng.randint(0, nh - h)
            boxes2 = boxes2 + torch.FloatTensor([left, top, left, top]).unsqueeze(0)
            exp = (nh, nw, top, left)
        gh, gw = exp[0], exp[1]
        crop, boxes2, labels = self._crop(gh, gw, boxes2, labels)
        if crop is None:
            crop = (0, 0, gh, gw)                                           # (top, left, h, w) inside the expanded image
        gh, gw = crop[2], crop[3]
        flip = rng.random() < 0.5                                           # flip_od
        if flip:
            boxes2[:, 0] = gw - boxes2[:, 0] - 1
            boxes2[:, 2] = gw - boxes2[:, 2] - 1
            boxes2 = boxes2[:, [2, 1, 0, 3]]
        old = torch.FloatTensor([gw, gh, gw, gh]).unsqueeze(0)              # folder2lmdb.py:142-151
        b = boxes2 / old
        bw, bh = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
        b = torch.cat(((b[..., 0] + bw / 2).unsqueeze(1), (b[..., 1] + bh / 2).unsqueeze(1), bw.unsqueeze(1), bh.unsqueeze(1)), 1)
        return dict(chain=chain, exp=exp, crop=crop, flip=flip, geo=(gh, gw), target=torch.cat((labels.unsqueeze(1), b), 1))

    def _crop(self, gh, gw, boxes2, labels):
        """random_crop_od (image_augmentation.py:54-145): -> (None or (top, left, h, w), boxes, labels)."""
        rng = self.rng
        while True:
            min_overlap = rng.choice([0., .1, .2, .3, .4, .5, None])
            if min_overlap is None:
                return None, boxes2, labels
            for _ in range(50):
                new_h, new_w = int(rng.uniform(0.5, 1) * gh), int(rng.uniform(0.5, 1) * gw)
                if not 0.5 < new_h / new_w < 2:
                    continue
                left = rng.randint(0, gw - new_w)
                top = rng.randint(0, gh - new_h)
                right, bottom = left + new_w, top + new_h
                cr = torch.FloatTensor([left, top, right, bottom])
                if boxes2.shape[0] == 0:
                    return (top, left, new_h, new_w), boxes2, labels
                if _jaccard(cr.unsqueeze(0), boxes2).squeeze(0).max().item() < min_overlap:
                    continue
                c = (boxes2[:, :2] + boxes2[:, 2:]) / 2.
                inside = (c[:, 0] > left) * (c[:, 0] < right) * (c[:, 1] > top) * (c[:, 1] < bottom)
                if not inside.any():
                    continue
                nb = boxes2[inside, :]
                nb[:, :2] = torch.max(nb[:, :2], cr[:2])
                nb[:, :2] -= cr[:2]
                nb[:, 2:] = torch.min(nb[:, 2:], cr[2:])
                nb[:, 2:] -= cr[:2]
                return (top, left, new_h, new_w), nb, labels[inside]

    def _mosaic(self, mems):
        """generate_mosaic_mask + Mosaic (image_augmentation.py:199-278) on the square canvas."""
        rng, S, num = self.rng, self.canvas, len(mems)
        xc = int(rng.uniform(.25, .75) * S)
        yc = int(rng.uniform(.25, .75) * S)
        if num == 2:
            mask = rng.choice([[[0, 0, xc, S], [xc, 0, S, S]], [[0, 0, S, yc], [0, yc, S, S]]])
        elif num == 3:
            mask = rng.choice([[[0, 0, S, yc], [0, yc, xc, S], [xc, yc, S, S]], [[0, 0, xc, yc], [xc, 0, S, yc], [0, yc, S, S]],
                               [[0, 0, xc, S], [xc, 0, S, yc], [xc, yc, S, S]], [[0, 0, xc, yc], [xc, 0, S, S], [0, yc, xc, S]]])
        else:
            mask = [[0, 0, xc, yc], [xc, 0, S, yc], [0, yc, xc, S], [xc, yc, S, S]]
        out = torch.Tensor(0, 5)
        for m, mem in zip(mask, mems):
            gh, gw = mem["geo"]
            width, height = m[2] - m[0], m[3] - m[1]
            ar_src = gh / gw
            min_ratio, max_ratio = ar_src * 0.5, ar_src * 2
            ar_tar = height / width
            ox = oy = 0
            if ar_tar < min_ratio:
                ox = rng.randint(0, int(width - height * (1 / min_ratio)))
                width = int(height * (1 / min_ratio))
            if ar_tar > max_ratio:
                oy = rng.randint(0, int(height - width * max_ratio))
                height = int(width * max_ratio)
            mem["tile"] = (m[0] + ox, m[1] + oy, width, height)
            mem["mask"] = tuple(m)
            label = mem["target"]
            if label.size(0):
                nb = label[..., 1:5]
                w_scale, h_scale = S / width, S / height
                nb[..., 0], nb[..., 2] = nb[..., 0] / w_scale, nb[..., 2] / w_scale
                nb[..., 1], nb[..., 3] = nb[..., 1] / h_scale, nb[..., 3] / h_scale
                nb[..., 0] = nb[..., 0] + (m[0] + ox) / S
                nb[..., 1] = nb[..., 1] + (m[1] + oy) / S
                out = torch.cat((out, torch.cat((label[..., 0].unsqueeze(1), nb), 1)))
        return out

    def plan(self, groups, size=None):
        """Host only.  groups: [[(image or (h, w), target)]] (with seg_classes a member may carry a third entry, its
        seg_id, which is checked against the image's size).  -> dict(items ITEM array (offsets unset), samples SAMPLE
        array, targets, count, size, n_mosaic, max_h, max_w)."""
        if len(groups) == 0:
            raise ValueError("empty batch")
        if self.seg_classes is not None:
            for g in groups:
                if len(g) != 1:
                    raise ValueError("a seg config takes groups of one image (the reference defines no Mosaic with seg maps), got %d" % len(g))
                for m in g:
                    if len(m) > 2:
                        im, sg = m[0], np.asarray(m[2])
                        hw = (int(im[0]), int(im[1])) if isinstance(im, tuple) else (int(im.shape[0]), int(im.shape[1]))
                        if sg.dtype != np.uint8 or sg.shape != hw:
                            raise ValueError("seg_id must be uint8 [h,w] of the image's size %s, got %s %s" % (hw, sg.dtype, sg.shape))
            groups = [[m[:2] for m in g] for g in groups]
        members, samples, targets, n_mosaic = [], [], [], 0
        hw_of = lambda im: (int(im[0]), int(im[1])) if isinstance(im, tuple) else (int(im.shape[0]), int(im.shape[1]))
        wplan = None if self.warp is None else self.warp.plan([hw_of(m[0]) for g in groups for m in g])
        for gi, g in enumerate(groups):
            if not 1 <= len(g) <= 4:
                raise ValueError("a group holds 1 to 4 images, got %d" % len(g))
            mems = []
            for im, tgt in g:
                h, w = hw_of(im)
                k = len(members) + len(mems)
                if wplan is not None and not wplan["identity"][k]:
                    tgt = self.warp.boxes(tgt, wplan["matrices"][k], h, w)
                mems.append(self._member(h, w, tgt, len(g) == 1))
                mems[-1]["src"] = (h, w)
            if len(g) == 1:
                targets.append(mems[0]["target"])
                samples.append((len(members), 1, -1, 0))
            else:
                targets.append(self._mosaic(mems))
                samples.append((len(members), len(g), n_mosaic, 0))
                n_mosaic += 1
            for m in mems:
                m["sample"] = gi
            members.extend(mems)
        if size is None:
            size = self.rng.choice(self.sizes)                           # folder2lmdb.py:227, after every __getitem__
        items = np.zeros(len(members), ITEM)
        for it, m in zip(items, members):
            it["h"], it["w"] = m["src"]
            it["n_ops"] = len(m["chain"])
            for k, (op, f) in enumerate(m["chain"]):
                it["op"][k] = op
                if op == HUE:
                    it["hue_shift"] = hue_shift_u8(f)
                elif op == GAMMA:
                    it["gamma_map"] = gamma_map(f)
                else:
                    it["factor"][k] = f                                   # Image.blend takes a C float
            it["exp"] = m["exp"]
            it["crop"] = m["crop"]
            it["flip"] = int(m["flip"])
            it["sample"] = m["sample"]
            if "tile" in m:
                it["tile"] = m["tile"]
                it["mask"] = m["mask"]
        if self.seg_classes is not None:
            gh, gw = int(size[0] / 16), int(size[1] / 16)                # folder2lmdb.py:228
            for k, m in enumerate(members):
                if m["geo"][0] < gh or m["geo"][1] < gw:
                    raise ValueError("image %d: the cropped geometry %dx%d is smaller than the %dx%d seg grid (the scale < 1 path of the "
                                     "area resize is not implemented)" % (k, m["geo"][0], m["geo"][1], gh, gw))
        max_h = int(max(items["exp"][:, 0].max(), items["h"].max()))
        max_w = int(max(items["exp"][:, 1].max(), items["w"].max()))
        out = dict(items=items, samples=np.array(samples, SAMPLE), targets=targets, count=sum(len(g) for g in groups),
                   size=tuple(int(v) for v in size), n_mosaic=n_mosaic, max_h=max_h, max_w=max_w, members=members)
        if wplan is not None:
            out["warp"] = wplan
        return out

    # ---- device ---------------------------------------------------------------------------------------------------
    def run_device(self, src, plan, out=None):
        """src: the packed uint8 images on the device (plan["items"]["offset"] set)."""
        items, samples = plan["items"], plan["samples"]
        oh, ow = plan["size"]
        n_out = len(samples)
        if out is None:
            out = torch.empty(n_out, 3, oh, ow, device=self.device, dtype=torch.float32)
        args = (len(items), n_out, plan["n_mosaic"], plan["max_h"], plan["max_w"], self.canvas, oh, ow)
        ws = torch.empty(query("mny_aug_ws_bytes", *args), device=self.device, dtype=torch.uint8)
        it_dev = torch.from_numpy(items.view(np.uint8).copy()).to(self.device, non_blocking=True)
        sm_dev = torch.from_numpy(samples.view(np.uint8).copy()).to(self.device, non_blocking=True)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_aug_batch", p(src), p(it_dev), len(items), p(sm_dev), n_out, plan["max_h"], plan["max_w"], self.canvas,
             plan["n_mosaic"], oh, ow, self.mean, self.std, p(out), p(ws), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._status = ws[:4].view(torch.int32)
        self._keep = (src, it_dev, sm_dev, ws)
        return out

    def run_device_seg(self, seg_src, seg_offsets, plan, out=None, items_dev=None, samples_dev=None):
        """seg_src: the packed uint8 id maps on the device; seg_offsets: their byte offsets (int64 array, multiples of 4).
        -> seg_maps [n_out, out_h/16, out_w/16, seg_classes] fp32 on the device."""
        if self.seg_classes is None:
            raise ValueError("this TrainAugment was built without seg_classes")
        items, samples = plan["items"], plan["samples"]
        gh, gw = int(plan["size"][0] / 16), int(plan["size"][1] / 16)
        n_out, C = len(samples), self.seg_classes
        if out is None:
            out = torch.empty(n_out, gh, gw, C, device=self.device, dtype=torch.float32)
        ws = torch.empty(query("mny_aug_seg_ws_bytes", len(items), n_out, C, plan["max_h"], plan["max_w"], gh, gw), device=self.device, dtype=torch.uint8)
        if items_dev is None:
            items_dev = torch.from_numpy(items.view(np.uint8).copy()).to(self.device, non_blocking=True)
        if samples_dev is None:
            samples_dev = torch.from_numpy(samples.view(np.uint8).copy()).to(self.device, non_blocking=True)
        off_dev = torch.from_numpy(np.ascontiguousarray(seg_offsets, np.int64)).to(self.device, non_blocking=True)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_aug_seg_batch", p(seg_src), p(off_dev), p(items_dev), len(items), p(samples_dev), n_out, C, plan["max_h"], plan["max_w"], gh, gw,
             p(out), p(ws), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._seg_status = ws[:4].view(torch.int32)
        self._seg_keep = (seg_src, off_dev, items_dev, samples_dev, ws)
        return out

    def pack(self, groups):
        """-> (pinned uint8 staging view, byte offsets of every image in group order)."""
        stage, desc, _, _ = self._packer.pack([m[0] for g in groups for m in g])
        return stage, desc["offset"]

    def pack_seg(self, groups):
        """-> (pinned uint8 staging view of the id maps, their byte offsets in group order)."""
        arrs = []
        for g in groups:
            for m in g:
                if len(m) < 3:
                    raise ValueError("a seg config takes (image, target, seg_id) members")
                a = m[2].numpy() if isinstance(m[2], torch.Tensor) else np.asarray(m[2])
                hw = tuple(int(v) for v in (m[0] if isinstance(m[0], tuple) else m[0].shape[:2]))
                if a.dtype != np.uint8 or a.shape != hw:
                    raise ValueError("seg_id must be uint8 [h,w] of the image's size %s, got %s %s" % (hw, a.dtype, a.shape))
                arrs.append(a)
        offsets, off = np.zeros(len(arrs), np.int64), 0
        for i, a in enumerate(arrs):
            offsets[i] = off
            off += (a.size + 15) // 16 * 16
        if self._seg_stage is None or self._seg_stage.numel() < off:
            self._seg_stage = torch.empty(max(off, 1 << 20), dtype=torch.uint8)
            if torch.cuda.is_available():
                self._seg_stage = self._seg_stage.pin_memory()
        buf = self._seg_stage.numpy()
        for o, a in zip(offsets, arrs):
            buf[o:o + a.size] = a.reshape(-1)
        return self._seg_stage[:off], offsets

    def __call__(self, groups, size=None):
        if self.decoder is not None and all_encoded([m[0] for g in groups for m in g]):
            src, desc, _, _ = self.decoder([m[0] for g in groups for m in g])
            hw = iter((int(d["h"]), int(d["w"])) for d in desc)
            groups = [[(next(hw),) + tuple(m[1:]) for m in g] for g in groups]   # plan() and pack_seg() need the sizes only
            plan = self.plan(groups, size)
            plan["items"]["offset"] = desc["offset"]
        else:
            plan = self.plan(groups, size)
            stage, offsets = self.pack(groups)
            plan["items"]["offset"] = offsets
            src = stage.to(self.device, non_blocking=True)
        if self.seq is not None:
            src = self.seq.run_device(src, plan["items"], self.seq.plan(len(plan["items"])))
        if self.warp is not None:
            src = self.warp.run_device(src, plan["items"], plan["warp"], channels=3)
        if self.seg_classes is None:
            images = self.run_device(src, plan)
            return images, plan["targets"], plan["count"]
        seg_stage, seg_offsets = self.pack_seg(groups)
        images = self.run_device(src, plan)
        seg_src = seg_stage.to(self.device, non_blocking=True)
        if self.warp is not None:                                        # the id maps take the image's coefficients
            seg_desc = np.zeros(len(plan["items"]), DESC)
            seg_desc["offset"], seg_desc["h"], seg_desc["w"] = seg_offsets, plan["items"]["h"], plan["items"]["w"]
            seg_src = self.warp.run_device(seg_src, seg_desc, plan["warp"], channels=1)
        seg_maps = self.run_device_seg(seg_src, seg_offsets, plan, items_dev=self._keep[1], samples_dev=self._keep[2])
        return images, plan["targets"], plan["count"], seg_maps

    def check(self):
        """Host sync: raise if the last batch held an image or record outside the declared bounds."""
        if self.seq is not None:
            self.seq.check()
        if self.warp is not None:
            self.warp.check()
        if self._status is not None:
            v = int(self._status.item())
            if v > 0:
                raise RuntimeError("augment: image %d is empty, misaligned or larger than the declared maximum" % (v - 1))
            if v < 0:
                raise RuntimeError("augment: sample record %d is malformed" % (-v - 1))
        if self._seg_status is not None:
            v = int(self._seg_status.item())
            if v > 0:
                raise RuntimeError("augment: seg map %d is misaligned, outside the declared maximum or smaller than the seg grid" % (v - 1))
            if v < 0:
                raise RuntimeError("augment: sample record %d is malformed for the seg maps (one image per sample)" % (-v - 1))
