"""Annotated images on the device — the reference's inference product (inference.py:58-104: draw the kept boxes on the decoded
image, dim the drivable-area pixels, write a file) and the train_batch*.jpg / val_batch*_pred.jpg sheets every YOLO trainer
writes.  `Annotator` turns what the other stages left on the device (a normalised batch or packed uint8 originals, the [k,7]
detection rows, [k,5] targets, seg probability planes) into packed uint8 RGB images, separately or as the tiles of one contact
sheet (csrc/viz.hip: mny_viz_boxes, mny_viz_compose); `jpeg.JpegEncoder` turns those into files.  No pixel visits the host.
With `names=` every drawn box carries "name score" as the reference's do (inference.py:90-95): the constructor renders one
coverage strip per class name and per character of "0123456789. " with Pillow (the reference's built-in bitmap font unless
`font=` says otherwise), the strips live on the device, and mny_viz_labels / mny_viz_compose_labels place and blend them.  No
font data is part of this package.  No CPU fallback: without libmnyolo.so every call raises MnyError."""
import colorsys
import ctypes
import math

import numpy as np
import torch

from ._lib import MnyError, call, query
from .prep import DESC

BOX = np.dtype([("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("rgb", np.uint8, 3), ("t", np.uint8)])   # mny_viz_box
ITEM = np.dtype([("dst_offset", np.int64), ("dst_stride", np.int64), ("seg_offset", np.int64), ("h", np.int32), ("w", np.int32)])   # mny_viz_item
LABEL = np.dtype([("lx", np.int32), ("ly", np.int32), ("lw", np.int32), ("seq", np.uint16, 13), ("n", np.uint8), ("lh", np.uint8), ("filled", np.uint8),
                  ("bg", np.uint8, 3), ("fg", np.uint8, 3), ("reserved", np.uint8)])   # mny_viz_label
assert BOX.itemsize == 20 and ITEM.itemsize == 32 and LABEL.itemsize == 48
CHARS = "0123456789. "                                                          # the strips after the names
MAX_TEXT_H, MAX_STRIP_W, MAX_NAMES = 64, 1024, 4096                             # the limits of include/mnyolo.h


def default_palette(n=20):
    """n well-separated saturated colours (golden-angle hues), uint8 [n,3]."""
    return np.array([[int(round(255 * c)) for c in colorsys.hsv_to_rgb((0.11 + 0.618033988749895 * i) % 1.0, 0.85, 1.0)] for i in range(n)], np.uint8)


def build_atlas(names, font=None):
    """The strip atlas of include/mnyolo.h: one coverage strip per class name, rendered whole, then one per character of CHARS.
    A strip is what ImageDraw.Draw(Image.new("L", (w, h), 0)).text((0, 0), s, fill=255, font=font) leaves, w = ceil(font.getlength(s)),
    h the font's line height (11 for the bitmap font, ascent + descent for a FreeType font); ink outside the strip, such as the faint
    column by which some FreeType glyphs overhang their advance, is cut.  font=None: Pillow's built-in bitmap font, ImageFont.load_default_imagefont() (1-bit, 6 x 11 cells, the
    reference's); pass ImageFont.load_default(size) or any other PIL font for larger antialiased text.
    -> (atlas uint8 [bytes], strips int32 [len(names) + 12, 2] of (offset, w), h)."""
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError as e:
        raise MnyError("names= renders its strips with Pillow, which is not installed") from e
    names = list(names)
    if len(names) > MAX_NAMES or not all(isinstance(s, str) for s in names):
        raise ValueError("names: at most %d strings" % MAX_NAMES)
    if font is None:
        font = ImageFont.load_default_imagefont()
    h = int(font.getbbox("0")[3]) if isinstance(font, ImageFont.ImageFont) else int(sum(font.getmetrics()))
    if not 1 <= h <= MAX_TEXT_H:
        raise ValueError("a line height of %d pixels (1..%d)" % (h, MAX_TEXT_H))
    strips = np.zeros((len(names) + len(CHARS), 2), np.int32)
    parts, off = [], 0
    for k, s in enumerate(names + list(CHARS)):
        try:
            w = int(math.ceil(font.getlength(s)))
            cov = np.zeros((h, 0), np.uint8)
            if w > 0:
                im = Image.new("L", (w, h), 0)
                ImageDraw.Draw(im).text((0, 0), s, fill=255, font=font)
                cov = np.asarray(im, np.uint8)
        except (UnicodeError, OSError, KeyError) as e:
            raise ValueError("class %d: the font cannot render the name %r (%s)" % (k, s, e)) from e
        if w > MAX_STRIP_W:
            raise ValueError("class %d: the name %r is %d pixels wide (at most %d)" % (k, s, w, MAX_STRIP_W))
        strips[k] = (off, w)
        parts.append(cov.reshape(-1))
        off += h * w
    return np.concatenate(parts), strips, h


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Annotator:
    """ann = Annotator(palette=None, thickness=2, score_thres=0.15, seg_channel=(1, 0), names=None, font=None, label="name_score",
                       label_bg=True, text_rgb=(255, 255, 255), label_targets=True)
       buf, desc = ann.annotate(images, dets=model.eval()(images), mean=cfg_mean, std=cfg_std)     # N separate images
       buf, desc = ann.sheet(images, cols=4, targets=targets, mean=cfg_mean, std=cfg_std)          # one image of N tiles
    images: a normalised fp32 [N,3,H,W] batch on the device (what BatchPrep / TrainAugment produce and the model takes), or a
    (buf, desc) pair of packed uint8 HWC originals (what JpegDecoder returns).  dets: the list of [k_i,7] tensors the model
    returns, or (rows [K,7], seg_begin int32 [N], seg_count int32 [N]) on the device.  targets: a list of [t_i,5] tensors
    (cls, cx, cy, w, h).  seg_probs: a list of fp32 [C,h_i,w_i] tensors on the device (segeval.upsample).  Targets are drawn
    first, detections over them.  -> (packed uint8 HWC buffer on the device, offsets multiples of 16; its DESC array).
    names: a list of str, index = class: every drawn box gets a label, "name 0.87" on a detection (label="name_score") or the
    name alone (label="name", and always on a target; label_targets=False leaves targets bare), above the box's top-left corner,
    or inside it where there is no room above, in text_rgb on the box's colour (label_bg=True) or straight on the image.  A
    class beyond the list is labelled with its index.  font: see build_atlas.  thickness=1, label="name", label_bg=False is the
    reference's style.  names=None (the default): no labels, and nothing of the above is built or run."""

    def __init__(self, palette=None, thickness=2, score_thres=0.15, seg_channel=(1, 0), names=None, font=None, label="name_score", label_bg=True,
                 text_rgb=(255, 255, 255), label_targets=True):
        pal = default_palette() if palette is None else np.ascontiguousarray(palette, np.uint8).reshape(-1, 3)
        if len(pal) < 1 or not 1 <= int(thickness) <= 8:
            raise ValueError("a palette of at least one colour and a thickness of 1..8")
        if any(c not in (0, 1, 2) for c in seg_channel):
            raise ValueError("seg_channel names RGB channels 0..2")
        self.palette, self.thickness, self.score_thres = pal, int(thickness), float(score_thres)
        self.seg_channel = tuple(int(c) for c in seg_channel)
        self.background = 114
        self.gutter = 2
        self._pal_dev = {}
        self._status = None
        self.names = None
        if names is not None:
            if label not in ("name_score", "name"):
                raise ValueError('label is "name_score" or "name"')
            if len(text_rgb) != 3 or any(not 0 <= int(c) <= 255 for c in text_rgb):
                raise ValueError("text_rgb is three bytes")
            self.names = list(names)
            self.atlas, self.strips, self.text_h = build_atlas(self.names, font)
            self.with_score, self.label_bg, self.label_targets = label == "name_score", bool(label_bg), bool(label_targets)
            self.text_rgb = tuple(int(c) for c in text_rgb)
            self._atlas_dev = {}

    # ---- pieces -------------------------------------------------------------------------------------------------------
    def _source(self, images):
        if isinstance(images, torch.Tensor):
            if images.ndim != 4 or images.shape[1] != 3 or images.dtype != torch.float32 or not images.is_cuda:
                raise ValueError("a batch is a fp32 [N,3,H,W] tensor on the device, got %s %s" % (images.dtype, tuple(images.shape)))
            x = images.contiguous()
            n, _, h, w = x.shape
            return x.device, n, [(h, w)] * n, x, None, None
        buf, desc = images
        desc = np.ascontiguousarray(desc, DESC)
        if buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
            raise ValueError("originals are a contiguous uint8 buffer on the device plus their DESC array")
        if len(desc) and (int(desc["offset"].min()) < 0 or int((desc["offset"] + 3 * desc["h"].astype(np.int64) * desc["w"]).max()) > buf.numel()):
            raise ValueError("an image lies outside buf")
        return buf.device, len(desc), [(int(d["h"]), int(d["w"])) for d in desc], None, buf, desc

    def _rows(self, rows, width, n, dev):
        """list of [k_i,width] tensors, or (rows, seg_begin, seg_count) -> (rows fp32 [K,width], begin int32 [n], count int32 [n], K) on dev."""
        if isinstance(rows, (tuple, list)) and len(rows) == 3 and isinstance(rows[1], torch.Tensor) and rows[1].dtype == torch.int32:
            r, b, c = rows
            if r.ndim != 2 or r.shape[1] != width or len(b) != n or len(c) != n:
                raise ValueError("(rows [K,%d], seg_begin [N], seg_count [N]) expected" % width)
            return r.to(dev, torch.float32).contiguous(), b.to(dev).contiguous(), c.to(dev).contiguous(), r.shape[0]
        if len(rows) != n or any(t.ndim != 2 or t.shape[1] != width for t in rows):
            raise ValueError("one [k,%d] tensor per image expected" % width)
        counts = np.array([t.shape[0] for t in rows], np.int32)                 # shapes are host knowledge: no sync
        begin = np.zeros(n, np.int32)
        begin[1:] = np.cumsum(counts)[:-1]
        r = torch.cat([t.to(dev, torch.float32) for t in rows]) if n else torch.zeros(0, width, device=dev)
        return r.contiguous(), torch.from_numpy(begin).to(dev), torch.from_numpy(counts).to(dev), int(counts.sum())

    def _atlas(self, dev):
        key = str(dev)
        if key not in self._atlas_dev:
            self._atlas_dev[key] = (torch.from_numpy(self.atlas.copy()).to(dev), torch.from_numpy(self.strips.copy()).to(dev))
        return self._atlas_dev[key]

    def boxes(self, rows, mode, sizes, dev):
        """`mny_viz_boxes` -> (records uint8 [K*20] on the device, seg_begin, seg_count, K); mode 0 detections, 1 targets."""
        out, _, begin, count, K = self.records(rows, mode, sizes, dev)
        return out, begin, count, K

    def records(self, rows, mode, sizes, dev):
        """`mny_viz_boxes`, and with names `mny_viz_labels` beside it -> (box records uint8 [K*20], label records uint8 [K*48] or None,
        seg_begin, seg_count, K), all on the device."""
        n = len(sizes)
        r, begin, count, K = self._rows(rows, 7 if mode == 0 else 5, n, dev)
        out = torch.zeros(max(K, 1) * BOX.itemsize, dtype=torch.uint8, device=dev)   # rows outside every segment: empty records
        lab = torch.zeros(max(K, 1) * LABEL.itemsize, dtype=torch.uint8, device=dev) if self.names is not None else None
        if K:
            dims = np.zeros(n, DESC)
            dims["h"], dims["w"] = [s[0] for s in sizes], [s[1] for s in sizes]
            key = str(dev)
            if key not in self._pal_dev:
                self._pal_dev[key] = torch.from_numpy(self.palette.copy()).to(dev)
            d_dev = torch.from_numpy(dims.view(np.uint8).copy()).to(dev)
            call("mny_viz_boxes", _p(r), mode, _p(begin), _p(count), n, K, _p(d_dev), self.score_thres, _p(self._pal_dev[key]), len(self.palette),
                 self.thickness, _p(out), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if lab is not None:
                _, strips = self._atlas(dev)
                call("mny_viz_labels", _p(r), mode, _p(begin), _p(count), n, K, _p(d_dev), _p(out), _p(strips), len(self.names), self.text_h,
                     int(self.with_score), int(self.label_bg), int(self.label_targets), (ctypes.c_uint8 * 3)(*self.text_rgb), _p(lab),
                     ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        return out, lab, begin, count, K

    def _compose(self, images, dets, targets, seg_probs, mean, std, dst, items):
        dev, n, sizes, batch, buf, desc = self._source(images)
        if n == 0:
            raise ValueError("empty batch")
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        C, seg, chan = 0, None, None
        keep = []
        if seg_probs is not None and len(seg_probs) and seg_probs[0].shape[0] > 0:
            C = int(seg_probs[0].shape[0])
            if C > len(self.seg_channel) or len(seg_probs) != n:
                raise ValueError("%d seg classes for seg_channel %s, %d planes for %d images" % (C, self.seg_channel, len(seg_probs), n))
            planes = [t.to(dev, torch.float32).contiguous() for t in seg_probs]
            for t, (h, w) in zip(planes, sizes):
                if tuple(t.shape) != (C, h, w):
                    raise ValueError("seg planes %s for an image of %dx%d" % (tuple(t.shape), h, w))
            base = min(t.data_ptr() for t in planes)                           # views of one buffer (segeval.upsample) or separate tensors
            items["seg_offset"] = [(t.data_ptr() - base) // 4 for t in planes]
            seg, chan = ctypes.c_void_p(base), (ctypes.c_int32 * C)(*self.seg_channel[:C])
            keep.append(planes)
        i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
        ws = torch.empty(query("mny_viz_ws_bytes", n), dtype=torch.uint8, device=dev)
        rec, lab, begin, count, K = None, None, None, None, 0
        if dets is not None and targets is not None:                            # one record list per image: its targets, then its detections
            if not all(isinstance(t, torch.Tensor) for t in dets):
                raise ValueError("targets together with detections need the detections as a list of [k,7] tensors")
            tr, tl, _, _, tk = self.records(targets, 1, sizes, dev)
            dr, dl, _, _, dk = self.records(dets, 0, sizes, dev)
            tcount, dcount = np.array([t.shape[0] for t in targets]), np.array([t.shape[0] for t in dets])
            t0, d0 = np.cumsum(tcount) - tcount, np.cumsum(dcount) - dcount
            order = np.concatenate([np.r_[np.arange(t0[i], t0[i] + tcount[i]), tk + np.arange(d0[i], d0[i] + dcount[i])] for i in range(n)]).astype(np.int64)
            both = torch.cat([tr.view(-1, BOX.itemsize)[:tk], dr.view(-1, BOX.itemsize)[:dk]])
            K = tk + dk
            o_dev = torch.from_numpy(order).to(dev)
            rec = both[o_dev].reshape(-1) if K else tr
            if tl is not None:                                                   # the same order for the labels
                lab = torch.cat([tl.view(-1, LABEL.itemsize)[:tk], dl.view(-1, LABEL.itemsize)[:dk]])[o_dev].reshape(-1) if K else tl
            cn = (tcount + dcount).astype(np.int32)
            begin, count = torch.from_numpy((np.cumsum(cn) - cn).astype(np.int32)).to(dev), torch.from_numpy(cn).to(dev)
        elif dets is not None:
            rec, lab, begin, count, K = self.records(dets, 0, sizes, dev)
        elif targets is not None:
            rec, lab, begin, count, K = self.records(targets, 1, sizes, dev)
        entry, more = "mny_viz_compose", ()
        if lab is not None and K:
            atlas, strips = self._atlas(dev)
            entry, more = "mny_viz_compose_labels", (_p(lab), _p(atlas), _p(strips))
        if batch is not None:
            m, s = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
            h, w = sizes[0]
            call(entry, _p(batch), h, w, m, s, None, None, _p(i_dev), n, _p(rec) if K else None, _p(begin), _p(count), K, seg, C, chan,
                 _p(dst), _p(ws), *more, st)
        else:
            d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
            call(entry, None, 0, 0, None, None, _p(buf), _p(d_dev), _p(i_dev), n, _p(rec) if K else None, _p(begin), _p(count), K, seg, C,
                 chan, _p(dst), _p(ws), *more, st)
            keep.append(d_dev)
        self._status = ws[:4].view(torch.int32)
        self._keep = (keep, i_dev, rec, lab, begin, count)

    # ---- the two layouts ----------------------------------------------------------------------------------------------
    def annotate(self, images, dets=None, targets=None, seg_probs=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        dev, n, sizes, _, _, _ = self._source(images)
        desc = np.zeros(n, DESC)
        items = np.zeros(n, ITEM)
        off = 0
        for i, (h, w) in enumerate(sizes):
            desc[i] = (off, h, w)
            items[i] = (off, 3 * w, 0, h, w)
            off += (3 * h * w + 15) // 16 * 16
        dst = torch.empty(max(off, 16), dtype=torch.uint8, device=dev)
        self._compose(images, dets, targets, seg_probs, mean, std, dst, items)
        return dst[:off], desc

    def sheet(self, images, cols=4, dets=None, targets=None, seg_probs=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
        """All images as tiles of one image, `cols` per row, cells of the largest image's size `gutter` pixels apart on `background`."""
        dev, n, sizes, _, _, _ = self._source(images)
        cols = max(1, min(int(cols), n))
        rows = -(-n // cols)
        ch, cw, g = max(s[0] for s in sizes), max(s[1] for s in sizes), self.gutter
        H, W = rows * ch + (rows + 1) * g, cols * cw + (cols + 1) * g
        items = np.zeros(n, ITEM)
        for i, (h, w) in enumerate(sizes):
            y, x = g + (i // cols) * (ch + g), g + (i % cols) * (cw + g)
            items[i] = ((y * W + x) * 3, 3 * W, 0, h, w)
        dst = torch.full((3 * H * W,), self.background, dtype=torch.uint8, device=dev)
        self._compose(images, dets, targets, seg_probs, mean, std, dst, items)
        desc = np.zeros(1, DESC)
        desc[0] = (0, H, W)
        return dst, desc

    def check(self):
        """Host sync: raise if the device left an item alone (its record contradicts its source)."""
        if self._status is not None and int(self._status.item()) != 0:
            raise RuntimeError("annotate: the device refused item %d" % (int(self._status.item()) - 1))
