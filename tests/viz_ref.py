"""The annotation stage of include/mnyolo.h (mny_viz_boxes, mny_viz_compose) restated in numpy, operation by operation in
fp32: draw records from detection or target rows, then source pixels, box outlines, seg overlay.  tests/test_viz_ref_cpu.py
holds the box rule to Pillow's ImageDraw.rectangle; tests/test_gpu_viz.py holds the kernels to this file, exactly."""
import numpy as np

BOX = np.dtype([("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("rgb", np.uint8, 3), ("t", np.uint8)])
f32 = np.float32


def _corner(v, size):
    """floor(v * size + 0.5) in fp32, clamped to +-2^30; None for a NaN."""
    with np.errstate(all="ignore"):
        f = np.floor(f32(v) * f32(size) + f32(0.5))
    if np.isnan(f):
        return None
    return int(min(max(f, -2.0 ** 30), 2.0 ** 30))


def records(rows, mode, H, W, thr, palette, t):
    """rows [k,7] (mode 0: x1, y1, x2, y2, conf, cls_score, cls) or [k,5] (mode 1: cls, cx, cy, w, h) -> BOX [k]; a row that is not
    drawn leaves the empty record (t = 0)."""
    rows = np.asarray(rows, f32).reshape(-1, 7 if mode == 0 else 5)
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    out = np.zeros(len(rows), BOX)
    for i, p in enumerate(rows):
        with np.errstate(all="ignore"):
            if mode == 0:
                x1, y1, x2, y2, cls = p[0], p[1], p[2], p[3], p[6]
                if not f32(p[4] * p[5]) > f32(thr):
                    continue
            else:
                cls = p[0]
                hw, hh = f32(0.5) * p[3], f32(0.5) * p[4]
                x1, x2, y1, y2 = p[1] - hw, p[1] + hw, p[2] - hh, p[2] + hh
        if not (cls >= 0 and cls < 16777216.0):
            continue
        c = [_corner(x1, W), _corner(y1, H), _corner(x2, W), _corner(y2, H)]
        if None in c:
            continue
        out[i] = (min(c[0], c[2]), min(c[1], c[3]), max(c[0], c[2]), max(c[1], c[3]), palette[int(cls) % len(palette)], t)
    return out


def denorm(x, mean, std):
    """x fp32 [3,H,W], normalised -> uint8 [H,W,3]: clamp(floor((x * std + mean) * 255 + 0.5), 0, 255), each operation in fp32."""
    x = np.asarray(x, f32)
    m, s = np.asarray(mean, f32).reshape(3, 1, 1), np.asarray(std, f32).reshape(3, 1, 1)
    with np.errstate(all="ignore"):
        v = np.floor((x * s + m) * f32(255) + f32(0.5))
    v = np.where(v > 0, np.minimum(v, 255), 0)                      # a NaN gives 0
    return v.astype(np.uint8).transpose(1, 2, 0).copy()


def draw(img, recs):
    """The box rule, in record order, later over earlier; in place on uint8 [H,W,3]."""
    H, W = img.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    for b in recs:
        t = int(b["t"])
        if t == 0:
            continue
        x0, y0, x1, y1 = int(b["x0"]), int(b["y0"]), int(b["x1"]), int(b["y1"])
        hit = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & ((x < x0 + t) | (x > x1 - t) | (y < y0 + t) | (y > y1 - t))
        img[hit] = b["rgb"]
    return img


def overlay(img, probs, seg_channel=(1, 0)):
    """probs fp32 [C,H,W]: for class c in order, pixels with p > 0.5 get trunc(float(v) * (1 - p)) in channel seg_channel[c]."""
    probs = np.asarray(probs, f32)
    for c in range(probs.shape[0]):
        p = probs[c]
        with np.errstate(all="ignore"):
            mask = p > f32(0.5)
            v = img[..., seg_channel[c]].astype(f32) * (f32(1.0) - p)
        v = np.where(v > 0, v, 0).astype(np.int64)                   # truncation; a negative product gives 0
        img[..., seg_channel[c]][mask] = v[mask].astype(np.uint8)
    return img


def compose(source, recs=None, probs=None, seg_channel=(1, 0), mean=None, std=None):
    """source: uint8 [H,W,3], or fp32 [3,H,W] with mean / std -> the annotated uint8 [H,W,3]."""
    source = np.asarray(source)
    img = source.copy() if source.dtype == np.uint8 else denorm(source, mean, std)
    if recs is not None:
        draw(img, recs)
    if probs is not None and len(probs):
        overlay(img, probs, seg_channel)
    return img
