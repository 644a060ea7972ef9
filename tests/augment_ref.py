"""TEST INFRASTRUCTURE — numpy restatement of the reference's training augmentation (utils/image_augmentation.py
transform_od / Mosaic, folder2lmdb.py get_single_image / collate_fn), the contract that
mobilenet-yolo-pytorch_amd/augment.py + csrc/augment.hip reproduce.  Only tests/ may import this.

Pieces, each cited:
  * photometric_distort (image_augmentation.py:169-197): torchvision's PIL paths (not vendored, restated the way
    torchvision writes them) over Pillow's C ops (restated below and PINNED live against the installed Pillow by
    tests/test_oracle_augment.py over the whole 2**24-colour RGB cube):
      adjust_brightness / adjust_saturation / adjust_contrast -> ImageEnhance.{Brightness,Color,Contrast}.enhance(f)
        = Image.blend(degenerate, img, f) (Blend.c: float alpha; 0 <= f <= 1 truncates, otherwise clip then
        truncate).  Brightness: degenerate 0.  Color: degenerate = convert("L") per pixel.  Contrast: degenerate =
        int(mean(convert("L")) + 0.5) of the image AS IT IS at that point of the chain.
      convert("L") (Convert.c rgb2l): (r*19595 + g*38470 + b*7471 + 0x8000) >> 16.
      adjust_hue: convert("HSV") (Convert.c rgb2hsv_row, float/double mix restated with numpy dtypes), H += shift
        (uint8 wrap), convert("RGB") (hsv2rgb).  shift = np.array(f * 255).astype(np.uint8): the double is
        truncated toward zero, then wrapped mod 256 (-5.3 -> 251, -17.99 -> 239, -0.2 -> 0) — the rule this
        restatement pins (np.uint8(-5.3) itself raises OverflowError on NumPy 2).
      adjust_gamma (gain 1): point() with int((255 + 1 - 1e-3) * pow(v / 255, g)).
  * to_tensor -> expand_od -> random_crop_od -> to_pil_image (image_augmentation.py:14-145, 311-325): uint8 -> /255 ->
    *255 -> .byte() is the identity for all 256 values; the 0.5 filler becomes 127.  flip_od (:147-166): column swap.
  * Image.resize (Pillow Resample.c): bilinear (prep_ref) and bicubic (a = -0.5, support 2, taps rounded with +-0.5).
  * Mosaic (:199-278) on a square canvas, then collate_fn's bilinear resize + normalise (folder2lmdb.py:223-256).
  * The draw-order planner: get_single_image (folder2lmdb.py:78-154) per member, Mosaic's draws, the batch size last.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import prep_ref  # noqa: E402

PRECISION_BITS = prep_ref.PRECISION_BITS
F32, F64 = np.float32, np.float64

BRIGHTNESS, CONTRAST, SATURATION, HUE, GAMMA = range(5)      # image_augmentation.py:178-182, pre-shuffle order
OP_NAMES = ("brightness", "contrast", "saturation", "hue", "gamma")


# ---- Pillow pixel ops -------------------------------------------------------------------------------------------
def to_l(img):
    """Convert.c rgb2l: ITU-R 601-2 luma in 16-bit fixed point, rounded."""
    i = img.astype(np.int64)
    return ((i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, alpha):
    """Blend.c ImagingBlend(deg, img, (float)alpha): in1 + alpha * (in2 - in1) in fp32, truncated (clipped first when
    alpha is outside [0, 1])."""
    a = F32(alpha)
    d = np.asarray(deg).astype(np.int32)
    t = d.astype(F32) + a * (img.astype(np.int32) - d).astype(F32)
    if 0.0 <= a <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, F32(0), np.where(t >= 255, F32(255), t)).astype(np.uint8)


def l_mean(img):
    """ImageStat.Stat(img.convert("L")).mean[0] rounded as ImageEnhance.Contrast does: int(sum / count + 0.5)."""
    s = int(to_l(img).astype(np.int64).sum())
    return int(float(s) / float(img.shape[0] * img.shape[1]) + 0.5)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    return blend(np.full_like(img, l_mean(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(to_l(img)[..., None], 3, axis=2), img, f)


def rgb_to_hsv(img):
    """Convert.c rgb2hsv_row (float locals, double literals)."""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    same = mx == mn
    cr = (mx - mn).astype(F32)
    cr1 = np.where(same, F32(1), cr)
    s = cr / np.where(mx == 0, F32(1), mx.astype(F32))
    rc = (mx - r).astype(F32) / cr1
    gc = (mx - g).astype(F32) / cr1
    bc = (mx - b).astype(F32) / cr1
    h = np.where(r == mx, bc - gc,
                 np.where(g == mx, ((2.0 + rc.astype(F64)) - bc.astype(F64)).astype(F32),
                          ((4.0 + gc.astype(F64)) - rc.astype(F64)).astype(F32)))
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    uh = np.clip((h.astype(F64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(F64) * 255.0).astype(np.int64), 0, 255)
    uh = np.where(same, 0, uh)
    us = np.where(same, 0, us)
    return np.stack([uh, us, mx], -1).astype(np.uint8)


def _c_round(x):
    """C round(): half away from zero."""
    return np.where(x < 0, -np.floor(-x + 0.5), np.floor(x + 0.5))


def hsv_to_rgb(hsv):
    """Convert.c hsv2rgb."""
    h, s, v = (hsv[..., c].astype(np.int32) for c in range(3))
    hf = h.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int64)
    f = (hf - i.astype(F32).astype(F64)).astype(F32)
    fs = (s.astype(F32).astype(F64) / 255.0).astype(F32)
    vf = v.astype(F32).astype(F64)
    p = np.clip(_c_round(vf * (1.0 - fs.astype(F64))), 0, 255).astype(np.int64)
    q = np.clip(_c_round(vf * (1.0 - (fs * f).astype(F64))), 0, 255).astype(np.int64)
    t = np.clip(_c_round(vf * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64)))), 0, 255).astype(np.int64)
    v = v.astype(np.int64)
    sel = i % 6
    r = np.choose(sel, [v, q, p, p, t, v])
    g = np.choose(sel, [t, v, v, q, p, p])
    b = np.choose(sel, [p, p, t, v, v, q])
    out = np.stack([r, g, b], -1)
    grey = (s == 0)[..., None]
    return np.where(grey, np.repeat(v[..., None], 3, -1), out).astype(np.uint8)


def hue_shift_u8(f):
    """np.array(f * 255).astype(np.uint8) for |f*255| < 256: truncate toward zero, wrap mod 256."""
    return int(math.trunc(f * 255.0)) % 256


def hue(img, f):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift_u8(f)) % 256
    return hsv_to_rgb(hsv)


def gamma_map(g):
    """torchvision adjust_gamma (gain 1): the 256-entry point() table."""
    return np.array([int((255 + 1 - 1e-3) * 1 * pow(v / 255.0, g)) for v in range(256)], np.uint8)


def gamma(img, g):
    return gamma_map(g)[img]


OPS = (brightness, contrast, saturation, hue, gamma)


def photometric(img, chain):
    """chain: [(op, factor)] in application order."""
    for op, f in chain:
        img = OPS[op](img, f)
    return img


# ---- Pillow resample (Resample.c) -------------------------------------------------------------------------------
def bicubic_filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients_bicubic(in_size, out_size):
    """precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter (support 2): taps may be negative and are
    rounded with -0.5 / +0.5 before the int cast."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resize_bicubic_u8(img_hwc, out_h, out_w):
    """Image.resize((out_w, out_h)) of an RGB uint8 image (BICUBIC, Pillow's default): horizontal pass first, an
    unchanged axis skipped."""
    h, w = img_hwc.shape[:2]
    out = img_hwc
    if w != out_w:
        out = prep_ref._pass(out, *coefficients_bicubic(w, out_w), axis=1)
    if h != out_h:
        out = prep_ref._pass(out, *coefficients_bicubic(h, out_h), axis=0)
    return np.ascontiguousarray(out)


resize_bilinear_u8 = prep_ref.resize_bilinear_u8


# ---- geometry: expand / crop / flip on the uint8 image ----------------------------------------------------------
FILLER_U8 = 127          # torch.ones * 0.5 -> to_pil_image's mul(255).byte() = int(127.5)


def geometry(img, expand, crop, flip):
    """expand: None or (new_h, new_w, top, left); crop: None or (top, left, h, w); flip: bool."""
    if expand is not None:
        nh, nw, top, left = expand
        canvas = np.full((nh, nw, 3), FILLER_U8, np.uint8)
        canvas[top:top + img.shape[0], left:left + img.shape[1]] = img
        img = canvas
    if crop is not None:
        t, l, h, w = crop
        img = img[t:t + h, l:l + w]
    if flip:
        img = img[:, ::-1]
    return np.ascontiguousarray(img)


# ---- Mosaic (image_augmentation.py:216-278) on the uint8 tiles ----------------------------------------------------
def mosaic(tiles, size):
    """tiles: [(geometric uint8 image, (x1, y1, width, height), mask (x0, y0, x1, y1))] -> uint8 [size, size, 3].
    The mask rectangle takes np.mean of the resized tile (float64, then astype(uint8) = trunc), the tile is pasted."""
    bg = np.zeros((size, size, 3), np.float64)
    for img, (x1, y1, w, h), m in tiles:
        t = resize_bicubic_u8(img, h, w)
        bg[m[1]:m[3], m[0]:m[2]] = np.mean(t, axis=(0, 1))
        bg[y1:y1 + h, x1:x1 + w] = t
    return bg.astype(np.uint8)


# ---- the planner: the reference's draw order (folder2lmdb.py:78-154, 223-227; image_augmentation.py) --------------
def find_jaccard_overlap(set_1, set_2):
    """utils/iou.py:4-49, restated with the same torch ops."""
    lower = torch.max(set_1[:, :2].unsqueeze(1), set_2[:, :2].unsqueeze(0))
    upper = torch.min(set_1[:, 2:].unsqueeze(1), set_2[:, 2:].unsqueeze(0))
    dims = torch.clamp(upper - lower, min=0)
    inter = dims[:, :, 0] * dims[:, :, 1]
    a1 = (set_1[:, 2] - set_1[:, 0]) * (set_1[:, 3] - set_1[:, 1])
    a2 = (set_2[:, 2] - set_2[:, 0]) * (set_2[:, 3] - set_2[:, 1])
    union = a1.unsqueeze(1) + a2.unsqueeze(0) - inter
    return inter / union


def plan_member(rng, h, w, target, expand, expand_scale):
    """get_single_image for one decoded image: -> dict(chain, expand, crop, flip, geo (h, w), target [n,5] float32)."""
    t2 = torch.Tensor(np.asarray(target, np.float32).reshape(-1, 5))
    boxes = t2[..., 1:5]
    if boxes.shape[0] == 0:                                               # folder2lmdb.py:115-127
        boxes2, labels = torch.zeros(0, 4), torch.zeros(0)
    else:
        x1 = (boxes[..., 0] - boxes[..., 2] / 2).unsqueeze(1)
        y1 = (boxes[..., 1] - boxes[..., 3] / 2).unsqueeze(1)
        x2 = (boxes[..., 0] + boxes[..., 2] / 2).unsqueeze(1)
        y2 = (boxes[..., 1] + boxes[..., 3] / 2).unsqueeze(1)
        boxes2 = torch.cat((x1 * w, y1 * h, x2 * w, y2 * h), 1)
        labels = t2[..., 0]
    # photometric_distort (:169-197)
    order = [BRIGHTNESS, CONTRAST, SATURATION, HUE, GAMMA]
    rng.shuffle(order)
    chain = []
    for op in order:
        if rng.random() < 0.5:
            f = rng.uniform(-18 / 255., 18 / 255.) if op == HUE else rng.uniform(0.5, 1.5)
            chain.append((op, f))
    # expand_od (:14-52, gate :317)
    exp = None
    gh, gw = h, w
    if rng.random() < 0.5 and expand:
        scale = rng.uniform(1, expand_scale)
        nh, nw = int(scale * h), int(scale * w)
        left = rng.randint(0, nw - w)
        top = rng.randint(0, nh - h)
        boxes2 = boxes2 + torch.FloatTensor([left, top, left, top]).unsqueeze(0)
        exp = (nh, nw, top, left)
        gh, gw = nh, nw
    # random_crop_od (:54-145)
    crop = None
    while True:
        min_overlap = rng.choice([0., .1, .2, .3, .4, .5, None])
        if min_overlap is None:
            break
        done = False
        for _ in range(50):
            scale_h = rng.uniform(0.5, 1)
            scale_w = rng.uniform(0.5, 1)
            new_h, new_w = int(scale_h * gh), int(scale_w * gw)
            if not 0.5 < new_h / new_w < 2:
                continue
            left = rng.randint(0, gw - new_w)
            top = rng.randint(0, gh - new_h)
            right, bottom = left + new_w, top + new_h
            cr = torch.FloatTensor([left, top, right, bottom])
            if boxes2.shape[0] > 0:
                overlap = find_jaccard_overlap(cr.unsqueeze(0), boxes2).squeeze(0)
                if overlap.max().item() < min_overlap:
                    continue
                c = (boxes2[:, :2] + boxes2[:, 2:]) / 2.
                inside = (c[:, 0] > left) * (c[:, 0] < right) * (c[:, 1] > top) * (c[:, 1] < bottom)
                if not inside.any():
                    continue
                nb = boxes2[inside, :]
                labels = labels[inside]
                nb[:, :2] = torch.max(nb[:, :2], cr[:2])
                nb[:, :2] -= cr[:2]
                nb[:, 2:] = torch.min(nb[:, 2:], cr[2:])
                nb[:, 2:] -= cr[:2]
                boxes2 = nb
            crop = (top, left, new_h, new_w)
            done = True
            break
        if done:
            break
    if crop is not None:
        gh, gw = crop[2], crop[3]
    # flip_od (:147-166, gate :329)
    flip = rng.random() < 0.5
    if flip:
        nb = boxes2
        nb[:, 0] = gw - boxes2[:, 0] - 1
        nb[:, 2] = gw - boxes2[:, 2] - 1
        boxes2 = nb[:, [2, 1, 0, 3]]
    # back to normalised cx, cy, w, h of the augmented image (folder2lmdb.py:142-151)
    old = torch.FloatTensor([gw, gh, gw, gh]).unsqueeze(0)
    b = boxes2 / old
    bw = b[..., 2] - b[..., 0]
    bh = b[..., 3] - b[..., 1]
    x = (b[..., 0] + bw / 2).unsqueeze(1)
    y = (b[..., 1] + bh / 2).unsqueeze(1)
    b = torch.cat((x, y, bw.unsqueeze(1), bh.unsqueeze(1)), 1)
    tgt = torch.cat((labels.unsqueeze(1), b), 1)
    return dict(chain=chain, expand=exp, crop=crop, flip=flip, geo=(gh, gw), target=tgt)


def plan_mosaic(rng, members, size):
    """generate_mosaic_mask + Mosaic's per-tile aspect clamp and box maps (:199-278).  size: square canvas side.
    -> (tiles [(x1, y1, width, height)], masks, target [n,5])."""
    num = len(members)
    S = [size, size]
    mask = [[0, 0, S[0], S[1]]]
    xc = int(rng.uniform(.25, .75) * S[0])
    yc = int(rng.uniform(.25, .75) * S[1])
    if num == 2:
        m1 = [[0, 0, xc, S[1]], [xc, 0, S[0], S[1]]]
        m2 = [[0, 0, S[0], yc], [0, yc, S[0], S[1]]]
        mask = rng.choice([m1, m2])
    elif num == 3:
        m1 = [[0, 0, S[0], yc], [0, yc, xc, S[1]], [xc, yc, S[0], S[1]]]
        m2 = [[0, 0, xc, yc], [xc, 0, S[0], yc], [0, yc, S[0], S[1]]]
        m3 = [[0, 0, xc, S[1]], [xc, 0, S[0], yc], [xc, yc, S[0], S[1]]]
        m4 = [[0, 0, xc, yc], [xc, 0, S[0], S[1]], [0, yc, xc, S[1]]]
        mask = rng.choice([m1, m2, m3, m4])
    elif num == 4:
        mask = [[0, 0, xc, yc], [xc, 0, S[0], yc], [0, yc, xc, S[1]], [xc, yc, S[0], S[1]]]
    labels_out = torch.Tensor(0, 5)
    tiles = []
    for k, mem in enumerate(members):
        gh, gw = mem["geo"]
        label = mem["target"]
        m = mask[k]
        width, height = m[2] - m[0], m[3] - m[1]
        ar_src = gh / gw
        min_ratio, max_ratio = ar_src * 0.5, ar_src * 2
        ar_tar = height / width
        ox = oy = 0
        if ar_tar < min_ratio:
            scale = 1 / min_ratio
            ox = rng.randint(0, int(width - height * scale))
            width = int(height * scale)
        if ar_tar > max_ratio:
            oy = rng.randint(0, int(height - width * max_ratio))
            height = int(width * max_ratio)
        x1, y1 = m[0] + ox, m[1] + oy
        tiles.append((x1, y1, width, height))
        if label.size(0):
            nb = label[..., 1:5]
            w_scale = S[0] / width
            h_scale = S[1] / height
            nb[..., 0], nb[..., 2] = nb[..., 0] / w_scale, nb[..., 2] / w_scale
            nb[..., 1], nb[..., 3] = nb[..., 1] / h_scale, nb[..., 3] / h_scale
            nb[..., 0] = nb[..., 0] + (m[0] + ox) / S[0]
            nb[..., 1] = nb[..., 1] + (m[1] + oy) / S[1]
            labels_out = torch.cat((labels_out, torch.cat((label[..., 0].unsqueeze(1), nb), 1)))
    return tiles, [tuple(m) for m in mask[:num]], labels_out


def plan(rng, groups, expand_scale, canvas, sizes):
    """The whole batch in the reference's draw order; groups: [[(h, w, target)]].  -> (samples, size, count), a
    sample being dict(members=[member plans], tiles, masks, target)."""
    samples = []
    for g in groups:
        mems = [plan_member(rng, h, w, t, len(g) == 1, expand_scale) for h, w, t in g]
        if len(g) == 1:
            samples.append(dict(members=mems, tiles=None, masks=None, target=mems[0]["target"]))
        else:
            tiles, masks, tgt = plan_mosaic(rng, mems, canvas)
            samples.append(dict(members=mems, tiles=tiles, masks=masks, target=tgt))
    size = rng.choice(sizes)
    return samples, tuple(size), sum(len(g) for g in groups)


def render_u8(images, sample, canvas):
    """The uint8 image one sample hands to collate_fn. images: that sample's decoded members."""
    geos = [geometry(photometric(im, m["chain"]), m["expand"], m["crop"], m["flip"])
            for im, m in zip(images, sample["members"])]
    if sample["tiles"] is None:
        return geos[0]
    return mosaic(list(zip(geos, sample["tiles"], sample["masks"])), canvas)


def collate(u8_images, size, mean, std):
    """folder2lmdb.py:223-256: bilinear resize to size (h, w), ToTensor, Normalize, stack."""
    return prep_ref.collate(u8_images, size, mean, std)
