"""Evaluation consumer of the segmentation head (BDD100K config): per-class IoU, mIoU and pixel accuracy on the device.

The reference trains the drivable-area head and never scores it: its test() loader returns no seg labels
(folder2lmdb.py:264-265) and the only consumer of the seg output is inference.py:64-67,100-103, which resizes each class map to
the image with bilinear interpolation and thresholds it at 0.5.  That rule, made single-label by the arg-max, is what
`mny_seg_confusion` (csrc/segeval.hip) applies to the batched seg logits `yolo.seg_logits()` returns, against full-resolution
uint8 id maps (0 = background, c = class c, an id above the class count such as 255 = ignored).  The arithmetic is specified in
include/mnyolo.h and restated in tests/segeval_ref.py; it is not pinned against cv2.
There is no CPU fallback: without libmnyolo.so every call raises MnyError.
"""
import ctypes

import numpy as np
import torch

from ._lib import call


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _logits(logits):
    if logits.dim() != 4:
        raise ValueError("seg logits must be [N,h,w,C] (channels last, what yolo.seg_logits() returns), got %s" % (tuple(logits.shape),))
    if logits.device.type != "cuda":
        raise RuntimeError("the seg evaluator needs CUDA tensors (the HIP path is the only path)")
    return logits.detach().to(torch.float32).contiguous()


def _sizes(sizes, n):
    s = np.ascontiguousarray([(int(a), int(b)) for a, b in sizes], np.int32).reshape(-1, 2)
    if len(s) != n:
        raise ValueError("%d sizes for %d images" % (len(s), n))
    return s


def _packed_offsets(sizes, per_pixel):
    """Offsets (in elements) of images laid back to back, each start rounded up to 16 bytes worth of elements."""
    step = 16 if per_pixel == 1 else 4
    off, o = np.zeros(len(sizes), np.int64), 0
    for i, (h, w) in enumerate(sizes):
        off[i] = o
        o += (int(h) * int(w) * per_pixel + step - 1) // step * step
    return off, o


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def upsample(logits, sizes):
    """Seg logits [N,h,w,C] -> list of N fp32 device tensors [C,H_i,W_i]: sigmoid, then half-pixel bilinear resizing to
    sizes[i] = (H_i, W_i) — a batch of inference.py:66-67.  No host sync."""
    x = _logits(logits)
    N, h, w, C = x.shape
    sz = _sizes(sizes, N)
    off, total = _packed_offsets(sz, 1)                     # floats per class plane; the image takes C planes
    off = off * C
    out = torch.empty(max(total * C, 4), device=x.device, dtype=torch.float32)
    call("mny_seg_upsample", _p(x), N, h, w, C, _hp(sz), _hp(off), _p(out), _st())
    return [out[o:o + C * H * W].view(C, H, W) for o, (H, W) in zip(off.tolist(), sz.tolist())]


def predict(logits, sizes):
    """Seg logits [N,h,w,C] -> list of N uint8 device id maps [H_i,W_i] (0 = background, c = class c).  No host sync."""
    x = _logits(logits)
    N, h, w, C = x.shape
    sz = _sizes(sizes, N)
    off, total = _packed_offsets(sz, 1)
    out = torch.empty(max(total, 16), device=x.device, dtype=torch.uint8)
    call("mny_seg_confusion", _p(x), N, h, w, C, None, _hp(off), _hp(sz), None, None, _p(out), _st())
    return [out[o:o + H * W].view(H, W) for o, (H, W) in zip(off.tolist(), sz.tolist())]


def pack_labels(labels, device, compact=False):
    """labels: list of uint8 [H_i,W_i] arrays / tensors, or one [N,H,W] uint8 tensor -> (keepalive, base pointer, offsets, sizes).
    Host members travel in ONE pinned upload; device members that are contiguous and 16-byte aligned are read where they are
    (an [N,H,W] device tensor whose H*W is no multiple of 16 is padded per image in one copy).  compact=True gathers device
    members into one buffer as well, so that the offsets also describe a buffer of the same size (pred_out)."""
    if isinstance(labels, torch.Tensor) and labels.dim() == 3:
        n, hh, ww = labels.shape
        if labels.device.type == "cuda" and labels.dtype == torch.uint8 and n and hh * ww:
            if labels.device != device:
                raise ValueError("the labels live on %s, the logits on %s" % (labels.device, device))
            rows = labels.reshape(n, -1)                     # one buffer, a fixed stride: no per-image work on the host
            if (hh * ww) % 16:
                rows = torch.nn.functional.pad(rows, (0, -(hh * ww) % 16))
            elif not rows.is_contiguous() or rows.data_ptr() % 16:
                rows = rows.clone(memory_format=torch.contiguous_format)
            sizes = np.ascontiguousarray(np.tile(np.array([[hh, ww]], np.int32), (n, 1)))
            return (rows,), rows.data_ptr(), np.arange(n, dtype=np.int64) * rows.shape[1], sizes
        labels = list(labels.unbind(0))
    if isinstance(labels, np.ndarray) and labels.ndim == 3:
        labels = list(labels)
    members, host = [], []
    for i, m in enumerate(labels):
        if not isinstance(m, torch.Tensor):
            m = torch.from_numpy(np.ascontiguousarray(m))
        if m.dtype != torch.uint8 or m.dim() != 2 or m.numel() == 0:
            raise ValueError("label %d must be a non-empty uint8 [H,W] id map, got %s %s" % (i, m.dtype, tuple(m.shape)))
        if m.device.type == "cuda":
            if m.device != device:
                raise ValueError("label %d lives on %s, the logits on %s" % (i, m.device, device))
            if not m.is_contiguous() or m.data_ptr() % 16:
                m = m.clone(memory_format=torch.contiguous_format)
        else:
            host.append(i)
        members.append(m)
    sizes = np.ascontiguousarray([tuple(m.shape) for m in members], np.int32).reshape(-1, 2)
    keep = []
    if host:
        off, total = _packed_offsets([sizes[i] for i in host], 1)
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        buf = stage.numpy()
        for o, i in zip(off.tolist(), host):
            buf[o:o + members[i].numel()] = members[i].contiguous().numpy().reshape(-1)
        up = stage.to(device, non_blocking=True)
        keep.append(up)
        for o, i in zip(off.tolist(), host):
            members[i] = up[o:o + members[i].numel()]
    ptrs = [m.data_ptr() for m in members]
    base = min(ptrs)
    if compact and len(host) != len(members):
        off, total = _packed_offsets(sizes, 1)
        buf = torch.zeros(max(total, 16), device=device, dtype=torch.uint8)
        for o, m in zip(off.tolist(), members):
            buf[o:o + m.numel()].copy_(m.reshape(-1))
        return (buf,), buf.data_ptr(), off, sizes
    return (members, keep), base, np.ascontiguousarray([p - base for p in ptrs], np.int64), sizes


class SegEvaluator:
    """Accumulates the confusion matrix of a validation set on the device and scores it once.

        ev = SegEvaluator(num_classes=2, class_names=["background", "direct", "alternative"])
        for images, id_maps in loader:                   # id_maps: uint8 [H_i,W_i] per image (or one [N,H,W] tensor)
            model(images)                                # eval forward; its (dets, seg_out) return is as before
            ev.add(model.seg_logits(), id_maps)          # no host sync
        scores = ev.compute()                            # {"iou": {name: v}, "miou", "miou_fg", "pixel_acc"}: the one sync

    `num_classes` is the head's channel count C; the matrix is [(C+1),(C+1)] with row = ground truth, column = prediction and
    entry 0 the background.  A class in neither map has IoU NaN and is left out of the means.  Under data parallelism every rank
    adds its own shard; before `compute()` the ranks sum `confusion` and `ignored` with one `all_reduce` (integer sums: the result
    does not depend on the order)."""

    def __init__(self, num_classes, class_names=None, device=None):
        self.C = int(num_classes)
        if not 1 <= self.C <= 16:
            raise ValueError("num_classes %d outside 1..16 (the seg head's channels, background not counted)" % self.C)
        names = list(class_names) if class_names is not None else ["background"] + ["class%d" % c for c in range(1, self.C + 1)]
        if len(names) != self.C + 1:
            raise ValueError("class_names must hold %d names, 'background' first" % (self.C + 1))
        self.class_names = names
        self._state = None
        if device is not None:
            self._alloc(torch.device(device))

    def _alloc(self, device):
        self._state = torch.zeros((self.C + 1) ** 2 + 1, device=device, dtype=torch.int64)

    @property
    def confusion(self):
        return self._need()[:-1].view(self.C + 1, self.C + 1)

    @property
    def ignored(self):
        return self._need()[-1:]

    def _need(self):
        if self._state is None:
            self._alloc(torch.device("cuda", torch.cuda.current_device()))
        return self._state

    def add(self, logits, labels, pred_out=False):
        """logits [N,h,w,C]; labels: N uint8 id maps of any sizes.  pred_out=True also returns the predicted id maps (device)."""
        x = _logits(logits)
        N, h, w, C = x.shape
        if C != self.C:
            raise ValueError("logits have %d channels, the evaluator %d classes" % (C, self.C))
        if self._state is None:
            self._alloc(x.device)
        if len(labels) != N:
            raise ValueError("%d label maps for %d images" % (len(labels), N))
        keep, base, off, sizes = pack_labels(labels, x.device, compact=pred_out)
        preds = out = None
        if pred_out:
            span = int(max(o + H * W for o, (H, W) in zip(off.tolist(), sizes.tolist())))
            out = torch.empty(max(span, 16), device=x.device, dtype=torch.uint8)
            preds = [out[o:o + H * W].view(H, W) for o, (H, W) in zip(off.tolist(), sizes.tolist())]
        st = self._state
        call("mny_seg_confusion", _p(x), N, h, w, C, ctypes.c_void_p(base), _hp(off), _hp(sizes), _p(st),
             ctypes.c_void_p(st.data_ptr() + 8 * (st.numel() - 1)), _p(out) if out is not None else None, _st())
        del keep
        return preds

    def merge(self, other):
        if other.C != self.C:
            raise ValueError("evaluators of %d and %d classes" % (self.C, other.C))
        if other._state is not None:
            self._need().add_(other._state.to(self._need().device))
        return self

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def compute_device(self):
        """-> {"iou": [C+1], "miou": [1], "miou_fg": [1], "pixel_acc": [1]} as float64 device tensors.  No host sync."""
        st = self._need()
        out = torch.empty(self.C + 4, device=st.device, dtype=torch.float64)
        call("mny_seg_metrics", _p(st), self.C, _p(out), _st())
        K = self.C + 1
        return {"iou": out[:K], "miou": out[K:K + 1], "miou_fg": out[K + 1:K + 2], "pixel_acc": out[K + 2:K + 3]}

    def compute(self):
        r = self.compute_device()
        v = torch.cat([r["iou"], r["miou"], r["miou_fg"], r["pixel_acc"]]).tolist()
        K = self.C + 1
        return {"iou": dict(zip(self.class_names, v[:K])), "miou": v[K], "miou_fg": v[K + 1], "pixel_acc": v[K + 2]}
