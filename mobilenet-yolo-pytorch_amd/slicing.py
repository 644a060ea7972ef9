"""Sliced (tiled) inference for small objects (SAHI's `get_sliced_prediction`), on the device.

    sl = Sliced(model, size=416, tile=(416, 416), overlap=0.2, full_view=True, mean=cfg["normalize"]["mean"], std=cfg["normalize"]["std"])
    dets = sl(images)               # list of decoded uint8 [h,w,3] arrays of ANY sizes -> list of [k_i,7] device tensors, normalised
                                    # to each ORIGINAL image: the contract of model.eval()(images)

Every other detection path looks at an image once, squeezed to the network's square input; an object of a few pixels does not survive the
resize.  Here the original image is cut into overlapping tiles at native resolution (`tile_grid`), every tile is a network input of its own
(`mny_prep_tiles` reads the crop windows from the one packed upload), its candidates are mapped back into the original image and appended
to that image's joint segment (`mny_det_append_tiles`, which also drops the boxes an interior tile edge cuts: `edge`), with `full_view` the
candidates of one whole-image view join them (the large objects), and ONE NMS runs over the union, the way `tta.TTA` runs it.  The records
run in chunks of `batch` slots through one cached eval plan; one host sync per call.  Opt-in: `model(images)` is untouched, and with one
tile that is the whole image, no full view and edge 0 the result equals `model(BatchPrep(...)(images))` bit for bit.

Record order per image: the full view first (when asked for), then the grid's tiles row-major; images in batch order.  It is the order of
the joint segment, so it is the NMS's tie-break: on equal scores the whole-image view wins.

`post=PostProcess(...)`: every chunk decodes through `mny_yolo_decode_ex`, the joint NMS is class-aware or class-agnostic at
`post.iou_thres` (then the merge threshold too), `mny_det_topk` caps every image at `post.max_det`.  No accuracy gain is claimed or
tested: there are no trained weights here."""
import ctypes

import numpy as np
import torch

from . import _lib, ops, postprocess, prep
from ._lib import MnyError

TILE_DESC = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32), ("pitch", np.int32), ("image", np.int32)])       # mny_tile_desc
TILE_MAP = np.dtype([("ax", np.float64), ("bx", np.float64), ("ay", np.float64), ("by", np.float64), ("ex", np.float32), ("ey", np.float32),
                     ("image", np.int32), ("interior", np.uint32)])                                                              # mny_tile_map
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8                                            # bits of mny_tile_map.interior


def _axis(size, tile, ov):
    """[(start, end)] of one axis: include/mnyolo.h "the tile grid" """
    out, k = [], 0
    while True:
        start = k * (tile - ov)
        end = start + tile
        out.append((start, end) if end <= size else (max(0, size - tile), size))
        if not end < size:
            return out
        k += 1


def tile_grid(h, w, tile_h, tile_w, overlap_h, overlap_w):
    """[(x0, y0, x1, y1), ...] in integer pixels, row-major: SAHI's slice windows (include/mnyolo.h states the rule)."""
    for name, v in (("h", h), ("w", w), ("tile_h", tile_h), ("tile_w", tile_w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (name, v))
    for name, v in (("overlap_h", overlap_h), ("overlap_w", overlap_w)):
        if not 0.0 <= float(v) < 1.0:                                           # (a NaN fails both compares)
            raise ValueError("%s must lie in [0, 1), got %r" % (name, v))
    oy, ox = int(float(overlap_h) * tile_h), int(float(overlap_w) * tile_w)
    if oy >= tile_h or ox >= tile_w:
        raise ValueError("the overlap (%d x %d pixels) must be below the tile's size (%d x %d)" % (oy, ox, tile_h, tile_w))
    h, w, tile_h, tile_w = int(h), int(w), int(tile_h), int(tile_w)
    return [(x0, y0, x1, y1) for y0, y1 in _axis(h, tile_h, oy) for x0, x1 in _axis(w, tile_w, ox)]


def tile_map(box, h, w, edge, size, image):
    """One mny_tile_map record (a TILE_MAP scalar) of the window `box` = (x0, y0, x1, y1) of an h x w image: the affine map formed in
    double, the edge margins in units of the network input, the interior bits."""
    x0, y0, x1, y1 = box
    m = np.zeros((), TILE_MAP)
    m["ax"], m["bx"] = np.float64(x0) / np.float64(w), np.float64(x1 - x0) / np.float64(w)
    m["ay"], m["by"] = np.float64(y0) / np.float64(h), np.float64(y1 - y0) / np.float64(h)
    m["ex"] = m["ey"] = np.float32(np.float64(edge) / np.float64(size))
    m["image"] = image
    m["interior"] = (LEFT if x0 > 0 else 0) | (TOP if y0 > 0 else 0) | (RIGHT if x1 < w else 0) | (BOTTOM if y1 < h else 0)
    return m


def _pair(v, what):
    try:
        a, b = v
    except TypeError:
        a = b = v
    except ValueError:
        raise ValueError("%s must be one value or a (vertical, horizontal) pair, got %r" % (what, v))
    return a, b


class Sliced:
    def __init__(self, model, size=416, tile=(416, 416), overlap=0.2, full_view=True, edge=0, batch=64, mean=None, std=None,
                 merge=False, nms_thr=0.45, post=None, decoder=None, max_candidates=None):
        if isinstance(size, bool) or not isinstance(size, int) or size <= 0 or size % 32:
            raise ValueError("size must be a positive multiple of 32, got %r" % (size,))
        self.tile = tuple(int(v) for v in _pair(tile, "tile"))
        self.overlap = tuple(float(v) for v in _pair(overlap, "overlap"))
        tile_grid(self.tile[0], self.tile[1], self.tile[0], self.tile[1], *self.overlap)       # the argument errors of the grid, now
        edge = float(edge)
        if not 0.0 <= edge < size / 2:
            raise ValueError("edge is in network-input pixels and must lie in 0 <= edge < size / 2 = %g, got %r" % (size / 2, edge))
        for name, v in (("batch", batch), ("max_candidates", max_candidates)):
            if (v is not None or name == "batch") and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
                raise ValueError("%s must be an integer >= 1%s, got %r" % (name, "" if name == "batch" else " or None", v))
        if mean is None or std is None:
            raise ValueError("mean and std are the config's normalize.mean / normalize.std: both must be given")
        nms_thr = float(nms_thr)
        if not 0.0 <= nms_thr <= 1.0:
            raise ValueError("nms_thr must lie in [0, 1], got %r" % (nms_thr,))
        if post is not None:
            if not isinstance(post, postprocess.PostProcess):
                raise ValueError("post must be a PostProcess or None, got %r" % (post,))
            post.check_classes(model.num_classes)
            nms_thr = post.iou_thres
        self.model, self.post = model, post
        self.size, self.edge, self.batch = size, edge, batch
        self.full_view, self.merge, self.nms_thr = bool(full_view), bool(merge), nms_thr
        self.max_candidates = max_candidates
        self.decoder = decoder
        self._mean, self._std = [float(v) for v in mean], [float(v) for v in std]
        self._prep = None          # prep.BatchPrep: the packed upload (or the decoder's buffer), made at the first call on the model's device
        self._bufs = {}            # one call shape resident at a time
        self._templates = {}       # (h, w) -> the records of an image of that shape
        self._seg = None           # (logits [N,h,w,C], seg_out [C,h,w]) of the last call's full views
        self._keep = None          # the source buffer and the tables the last call's launches read
        self.originals = None      # (uint8 device buffer, prep.DESC array) of the last call's images

    # ---- the records of a call ---------------------------------------------------------------------------------------------
    def _template(self, h, w):
        """the records of one h x w image at offset 0, image 0 (cached per shape: a video's frames share one)"""
        t = self._templates.get((h, w))
        if t is None:
            boxes = ([(0, 0, w, h)] if self.full_view else []) + tile_grid(h, w, self.tile[0], self.tile[1], *self.overlap)
            tiles, maps, full = np.zeros(len(boxes), TILE_DESC), np.zeros(len(boxes), TILE_MAP), np.zeros(len(boxes), bool)
            for k, (x0, y0, x1, y1) in enumerate(boxes):
                tiles[k] = ((y0 * w + x0) * 3, y1 - y0, x1 - x0, 3 * w, 0)
                maps[k] = tile_map((x0, y0, x1, y1), h, w, self.edge, self.size, 0)       # (a full view: interior = 0, no side is inside)
            full[0] = self.full_view
            if len(self._templates) >= 64:
                self._templates.clear()
            self._templates[(h, w)] = t = (tiles, maps, full)
        return t

    def records(self, desc):
        """(tiles: TILE_DESC [R], maps: TILE_MAP [R], full: bool [R], the record is a full view) for the images of `desc` (prep.DESC:
        offset, h, w of each in the packed buffer)"""
        tiles, maps, full = [], [], []
        for i, d in enumerate(desc):
            t, m, f = self._template(int(d["h"]), int(d["w"]))
            t, m = t.copy(), m.copy()
            t["offset"] += int(d["offset"])
            t["image"] = m["image"] = i
            tiles.append(t), maps.append(m), full.append(f)
        return np.concatenate(tiles), np.concatenate(maps), np.concatenate(full)

    def _buffers(self, N, cap, Bc, chunks, plan, dev, max_h, max_w):
        key = (N, cap, Bc, chunks, plan.cap, str(dev), max_h, max_w)
        b = self._bufs.get(key)
        if b is not None:
            return b
        self._bufs.clear()
        C, post, S = self.model.num_classes, self.post, self.size
        if post is not None:
            stride = post.stride(plan.cap, C)
            b = postprocess.nms_buffers(post, C, N, cap, dev, extra=N + 2 * Bc * chunks)
            b.update({"chunk_rows": torch.zeros(Bc, stride, 7, device=dev),    # one chunk's candidates, before they are appended
                      "cnt0": torch.zeros(Bc, device=dev, dtype=torch.int32),
                      "cnt1": torch.zeros(Bc, device=dev, dtype=torch.int32),
                      "cmask": ops.class_mask(post.classes, C, dev) if post.classes is not None else None})
        else:
            b = {"seg_begin": (torch.arange(N, dtype=torch.int32) * cap).to(dev),
                 "out_idx": torch.zeros(N * cap, device=dev, dtype=torch.int32),
                 "out": torch.zeros(2 * N + 1, device=dev, dtype=torch.int32),
                 "out_rows": torch.zeros(N * cap, 7, device=dev),
                 "ws": torch.empty(_lib.query("mny_nms_ws_bytes", N, N * cap, C), device=dev, dtype=torch.uint8)}
            so = _lib.query("mny_nms_status_offset", N, N * cap, C)
            po = _lib.query("mny_nms_prefix_offset", N, N * cap, C)
            b["status"] = b["ws"][so:so + 4].view(torch.int32)
            b["prefix"] = b["ws"][po:po + 4 * (N + 1)].view(torch.int32)
        # `out` = out_counts [N] | NMS status [1] | the append's dropped [N] | (post) the decode's dropped [chunks, 2, Bc]: one copy back
        b.update({"cap": cap,
                  "rows": torch.zeros(N, cap, 7, device=dev),
                  "counts": torch.zeros(N, device=dev, dtype=torch.int32),
                  "x": torch.empty(Bc, 3, S, S, device=dev),                    # resident: the plan reads it through a raw pointer
                  "prep_ws": torch.empty(_lib.query("mny_prep_tiles_ws_bytes", Bc, max_h, max_w, S, S), device=dev, dtype=torch.uint8)})
        self._bufs[key] = b
        return b

    def __call__(self, images):
        model, post, S = self.model, self.post, self.size
        if model.training:
            raise MnyError("Sliced needs model.eval(): a decode in training mode would update the BatchNorm statistics once per chunk")
        if len(images) == 0:
            raise ValueError("empty batch")
        dev = model.device
        if self._prep is None:
            self._prep = prep.BatchPrep([(S, S)], self._mean, self._std, device=dev, decoder=self.decoder)
        if self.decoder is not None and prep.all_encoded(images):
            src, desc, _, _ = self.decoder(images)
        else:
            stage, desc, _, _ = self._prep.pack(images)
            src = stage.to(dev, non_blocking=True)                              # the one packed upload of the call
        N, C = len(images), model.num_classes
        tiles, maps, full = self.records(desc)
        R = len(tiles)
        per_image = np.bincount(tiles["image"], minlength=N)
        Bc = min(self.batch, R)
        chunks = -(-R // Bc)
        pad = chunks * Bc - R
        if pad:                                                                 # the last chunk is padded with image = -1 slots
            tiles = np.concatenate([tiles, np.zeros(pad, TILE_DESC)])
            maps = np.concatenate([maps, np.zeros(pad, TILE_MAP)])
            full = np.concatenate([full, np.zeros(pad, bool)])
            tiles["image"][R:] = -1
            maps["image"][R:] = -1
        max_h, max_w = int(tiles["h"].max()), int(tiles["w"].max())
        val_conf = [float(h.val_conf) for h in model.yolo_losses]
        with torch.no_grad():
            plan = model._eval_plans(Bc, [S], [S, S])[0]
            stride = plan.cap if post is None else post.stride(plan.cap, C)
            cap = int(per_image.max()) * stride if self.max_candidates is None else self.max_candidates
            b = self._buffers(N, cap, Bc, chunks, plan, dev, max_h, max_w)
            tiles_dev = torch.from_numpy(tiles.view(np.uint8).reshape(chunks, -1).copy()).to(dev, non_blocking=True)
            maps_dev = torch.from_numpy(maps.view(np.uint8).reshape(chunks, -1).copy()).to(dev, non_blocking=True)
            self._keep = (src, tiles_dev, maps_dev)
            self.originals = (src, desc)                                        # the packed originals on the device: what viz.Annotator draws on
            out = b["out"]
            b["counts"].zero_()
            out[N + 1:2 * N + 1].zero_()
            dropped = out[N + 1:2 * N + 1]
            seg = plan.seg_head is not None and self.full_view
            seg_logits, seg_out = [], None
            for k in range(chunks):
                ops.prep_tiles(src, tiles_dev[k], Bc, max_h, max_w, S, S, self._prep.mean, self._prep.std, out=b["x"], ws=b["prep_ws"])
                if post is None:
                    plan.forward_eval(b["x"], val_conf, nms=False)
                    ops.det_append_tiles(plan.rows, plan.cnt1, maps_dev[k], b["rows"], b["counts"], dropped)
                else:
                    plan.forward_eval(b["x"], val_conf, decode=False)
                    d0 = 2 * N + 1 + 2 * Bc * k
                    postprocess.decode_plan(plan, post, model, b["chunk_rows"], b["cnt0"], b["cnt1"], out[d0:d0 + Bc], out[d0 + Bc:d0 + 2 * Bc],
                                            b["cmask"])
                    ops.det_append_tiles(b["chunk_rows"], b["cnt1"], maps_dev[k], b["rows"], b["counts"], dropped)
                if seg:
                    # the next chunk overwrites the plan's buffers: take the full views' seg outputs now (a full view is the first record of
                    # its image, so image 0's is slot 0 of chunk 0: the plan's own sigmoid of its image 0)
                    seg_logits += [plan.seg_head[int(s)].to(torch.float32).clone() for s in np.nonzero(full[k * Bc:(k + 1) * Bc])[0]]
                    if k == 0:
                        seg_out = plan.seg_eval.clone()
            if post is None:
                _lib.call("mny_nms_per_class", ops._p(b["rows"]), ops._p(b["seg_begin"]), ops._p(b["counts"]), N, N * cap, cap, C,
                          ctypes.c_double(self.nms_thr), ops._p(b["out_idx"]), ops._p(out), ops._p(b["out_rows"]),
                          ctypes.c_void_p(b["ws"].data_ptr()), ops._st())
                prefix = b["prefix"]
            else:
                postprocess.run_nms(post, C, b["rows"], b["seg_begin"], b["counts"], b["out_idx"], out, b["out_rows"], b["ws"])
                prefix = postprocess.run_topk(post, b["rows"], b)
            if self.merge:
                ops.nms_merge(b["rows"].view(-1, 7), b["seg_begin"], b["counts"], b["out_idx"], out[:N], prefix, b["out_rows"], thr=self.nms_thr)
            out[N:N + 1].copy_(b["status"])
            host = out.tolist()                                                 # the one host sync of the call
            counts, status = host[:N], host[N]
            for n, d in enumerate(host[N + 1:2 * N + 1]):
                if d:
                    raise MnyError("sliced inference: image %d has %d candidates more than its joint segment of %d rows holds: raise "
                                   "max_candidates or the thresholds" % (n, d, cap))
            for j, d in enumerate(host[2 * N + 1:]):
                slot = j // (2 * Bc) * Bc + j % Bc
                if d and tiles["image"][slot] >= 0:
                    raise MnyError("decode (a tile of image %d): %d candidates more than the candidate buffer holds (head %d): raise "
                                   "post.max_candidates or the thresholds" % (tiles["image"][slot], d, j // Bc % 2))
            if status != 0:
                raise MnyError("NMS: a bucket of %d boxes exceeded the joint per-image candidate bound" % status)
            dets = b["out_rows"][:sum(counts)].clone()
        dets = list(torch.split(dets, counts))
        if seg:
            self._seg = (torch.stack(seg_logits), seg_out)
            return dets, seg_out.cpu().numpy()                                  # (output, seg_out) of image 0's full view, as model(images)
        self._seg = None
        return dets

    def seg_logits(self):
        """The full views' raw seg logits of the last call, [N,h,w,C] fp32 on the device (what model.seg_logits() returns after
        model(images) at `size`; a Sliced call withdraws that one, because the chunks overwrite the plan's buffers)."""
        if not self.model.has_seg:
            raise MnyError("seg_logits: this config has no `seg:` section, the model has no segmentation head")
        if not self.full_view:
            raise MnyError("seg_logits: full_view is off, no view of a call sees a whole image (stitched seg maps are out of scope)")
        if self._seg is None:
            raise MnyError("seg_logits: no Sliced call has run yet")
        return self._seg[0].clone()
