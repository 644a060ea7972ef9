"""The text part of the annotation stage of include/mnyolo.h (mny_viz_labels, mny_viz_compose_labels) restated in numpy on top of
tests/viz_ref.py: label records beside the box records, then per record its outline and its label, blended by Pillow's rule.
tests/test_vizlabel_ref_cpu.py holds this file to Pillow's ImageDraw.text and to hand-worked answers; tests/test_gpu_vizlabel.py holds
the kernels to this file, exactly."""
import numpy as np

import viz_ref as V

LABEL = np.dtype([("lx", np.int32), ("ly", np.int32), ("lw", np.int32), ("seq", np.uint16, 13), ("n", np.uint8), ("lh", np.uint8), ("filled", np.uint8),
                  ("bg", np.uint8, 3), ("fg", np.uint8, 3), ("reserved", np.uint8)])
CHARS = "0123456789. "
DOT, SPACE = 10, 11
PAD = 2
f32 = np.float32


def score_digits(prod):
    """fp32 product -> k = rint((double)prod * 100.0), ties to even, clamped to 0..999; its label digits are k // 100, '.', k // 10 % 10, k % 10."""
    with np.errstate(all="ignore"):
        v = np.rint(np.float64(f32(prod)) * np.float64(100.0))
    return int(v) if 0.0 < v < 999.0 else (999 if v >= 999.0 else 0)


def sequence(cls, n_names, prod=None):
    """The strip indices of a label: the name's strip, or the decimal digits of the class index; with a score five more."""
    c = int(cls)
    seq = [c] if c < n_names else [n_names + int(d) for d in str(c)]
    if prod is not None:
        k = score_digits(prod)
        seq += [n_names + SPACE, n_names + k // 100, n_names + DOT, n_names + k // 10 % 10, n_names + k % 10]
    return seq


def labels(rows, mode, recs, W, strips, n_names, h, with_score=True, filled=True, label_targets=True, text_rgb=(255, 255, 255)):
    """rows as viz_ref.records takes them, recs = what it returned for them, W the image's width -> LABEL [k]; all zero = empty."""
    rows = np.asarray(rows, f32).reshape(-1, 7 if mode == 0 else 5)
    strips = np.asarray(strips, np.int32).reshape(-1, 2)
    out = np.zeros(len(rows), LABEL)
    for i, (p, b) in enumerate(zip(rows, recs)):
        if int(b["t"]) == 0 or (mode == 1 and not label_targets):
            continue
        cls = p[6] if mode == 0 else p[0]
        if not (cls >= 0 and cls < 16777216.0):
            continue
        with np.errstate(all="ignore"):
            prod = f32(p[4] * p[5]) if mode == 0 and with_score else None
        seq = sequence(cls, n_names, prod)
        lw = int(sum(int(strips[s, 1]) for s in seq)) + 2 * PAD
        x0, y0 = int(b["x0"]), int(b["y0"])
        o = out[i]
        o["lx"], o["ly"], o["lw"] = max(min(x0, W - lw), 0), (y0 - h if y0 - h >= 0 else y0), lw
        o["seq"][:len(seq)] = seq
        o["n"], o["lh"], o["filled"], o["bg"], o["fg"] = len(seq), h, 1 if filled else 0, b["rgb"], text_rgb
    return out


def text_row(lab, atlas, strips):
    """The label's coverage, uint8 [lh, tw]: its strips side by side."""
    h = int(lab["lh"])
    parts = [np.zeros((h, 0), np.uint8)]
    for s in lab["seq"][:int(lab["n"])]:
        off, w = int(strips[s, 0]), int(strips[s, 1])
        parts.append(np.asarray(atlas[off:off + h * w], np.uint8).reshape(h, w))
    return np.concatenate(parts, 1)


def blend(m, under, ink):
    """Pillow's blend through an 8-bit mask, per channel, in integers."""
    tmp = m.astype(np.int64) * int(ink) + (255 - m.astype(np.int64)) * under.astype(np.int64) + 128
    return (((tmp >> 8) + tmp) >> 8).astype(np.uint8)


def draw_label(img, lab, atlas, strips):
    """One label onto uint8 [H,W,3], in place; clipped to the image."""
    if int(lab["n"]) == 0:
        return img
    H, W = img.shape[:2]
    lx, ly, lw, lh = int(lab["lx"]), int(lab["ly"]), int(lab["lw"]), int(lab["lh"])
    cov = np.zeros((lh, lw), np.uint8)
    text = text_row(lab, atlas, strips)
    cov[:, PAD:PAD + text.shape[1]] = text
    xa, xb, ya, yb = max(lx, 0), min(lx + lw, W), max(ly, 0), min(ly + lh, H)
    if xa >= xb or ya >= yb:
        return img
    m = cov[ya - ly:yb - ly, xa - lx:xb - lx]
    for c in range(3):
        under = np.full(m.shape, lab["bg"][c], np.uint8) if int(lab["filled"]) else img[ya:yb, xa:xb, c]
        img[ya:yb, xa:xb, c] = blend(m, under, lab["fg"][c])
    return img


def draw(img, recs, labs, atlas, strips):
    """Step 2 with labels: per record in order its outline (viz_ref.draw), then its label."""
    strips = np.asarray(strips, np.int32).reshape(-1, 2)
    for i in range(len(recs)):
        V.draw(img, recs[i:i + 1])
        draw_label(img, labs[i], atlas, strips)
    return img


def compose(source, recs, labs, atlas, strips, probs=None, seg_channel=(1, 0), mean=None, std=None):
    """viz_ref.compose with labels: source, then outlines and labels record by record, then the seg overlay."""
    source = np.asarray(source)
    img = source.copy() if source.dtype == np.uint8 else V.denorm(source, mean, std)
    draw(img, recs, labs, atlas, strips)
    if probs is not None and len(probs):
        V.overlay(img, probs, seg_channel)
    return img


def random_atlas(rng, n_names, h, max_w=40, empty=()):
    """n_names + 12 random uint8 strips of widths 1..max_w (0 for the indices in `empty`): every blend level, no font."""
    strips = np.zeros((n_names + len(CHARS), 2), np.int32)
    parts, off = [], 0
    for k in range(len(strips)):
        w = 0 if k in empty else int(rng.integers(1, max_w + 1))
        strips[k] = (off, w)
        cov = rng.integers(0, 256, h * w, dtype=np.uint8)
        cov[rng.random(h * w) < 0.3] = 0
        cov[rng.random(h * w) < 0.2] = 255
        parts.append(cov)
        off += h * w
    return np.concatenate(parts), strips
