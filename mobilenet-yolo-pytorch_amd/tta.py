"""Test-time augmentation of the detection path (Ultralytics' `--augment`) and box merging ("merge-NMS").

    tta = TTA(model, views=default_views(352), merge=True, nms_thr=0.45)
    dets = tta(images)              # list of [k_i,7] device tensors: the contract of model.eval()(images)

The batch goes through the model's cached eval plans once per view (`mny_tta_view` builds the mirrored / resized input on the device),
every view's pre-NMS candidates are appended per image, un-mirrored, into one joint buffer (`mny_det_append`: the rows are normalised,
so a change of scale needs no box arithmetic), ONE `mny_nms_per_class` runs over the union and, with `merge`, `mny_nms_merge` replaces
every kept box by the score-weighted mean of the candidates of its class that overlap it.  One host sync per call (the final counts).
Opt-in: `model(images)` is untouched, and `TTA(model, views=[(S, False)], merge=False)(x)` equals it bit for bit.

`post=PostProcess(...)` (postprocess.py): every view decodes through `mny_yolo_decode_ex` with the post-processing options, the joint NMS
is class-aware or class-agnostic at `post.iou_thres` (which then is the merge threshold too, `nms_thr` is not read), and `mny_det_topk`
caps every image at `post.max_det` before the merge.  `post=None` is the path above.
"""
import ctypes

import torch

from . import _lib, ops, postprocess
from ._lib import MnyError


def _ceil32(num, den):
    """ceil(num / den / 32) * 32 in integers"""
    return -((-num) // (den * 32)) * 32


def _check_size(size, what):
    if isinstance(size, bool) or not isinstance(size, int) or size <= 0 or size % 32:
        raise ValueError("%s must be a positive multiple of 32, got %r" % (what, size))


def default_views(size):
    """[(S, False), (ceil32(0.83 * S), True), (ceil32(0.67 * S), False)]: Ultralytics' scales and mirrors.  At small sizes the rounding
    makes views coincide; a view that repeats an earlier (size, flip) pair is left out (it would only double every candidate)."""
    _check_size(size, "default_views: size")
    views = []
    for v in [(size, False), (_ceil32(83 * size, 100), True), (_ceil32(67 * size, 100), False)]:
        if v not in views:
            views.append(v)
    return views


class TTA:
    def __init__(self, model, views, merge=True, nms_thr=0.45, post=None):
        try:
            views = [tuple(v) for v in views]
        except TypeError:
            views = []
        if not views or any(len(v) != 2 for v in views):
            raise ValueError("views must be a non-empty list of (size, flip) pairs")
        for size, flip in views:
            _check_size(size, "a view's size")
            if not isinstance(flip, (bool, int)) or flip not in (0, 1):
                raise ValueError("a view's flip must be True or False, got %r" % (flip,))
        if views[0][1]:
            raise ValueError("views[0] must be the identity view (the input's own size, no mirror)")
        nms_thr = float(nms_thr)
        if not 0.0 <= nms_thr <= 1.0:
            raise ValueError("nms_thr must lie in [0, 1], got %r" % (nms_thr,))
        if post is not None:
            if not isinstance(post, postprocess.PostProcess):
                raise ValueError("post must be a PostProcess or None, got %r" % (post,))
            post.check_classes(model.num_classes)
            nms_thr = post.iou_thres
        self.post = post
        self.model = model
        self.views = [(int(s), bool(f)) for s, f in views]
        self.merge = bool(merge)
        self.nms_thr = nms_thr
        self._bufs = {}            # N -> joint buffers and the view inputs
        self._seg = None           # (logits [N,h,w,C], seg_out [C,h,w]) of the last call's identity view, copied before the next view ran

    def _buffers(self, N, caps, dev):
        key = (N, tuple(caps), str(dev))
        b = self._bufs.get(key)
        if b is None:
            self._bufs.clear()                                                  # one batch shape resident at a time
            cap = sum(caps)
            C = self.model.num_classes
            b = {"cap": cap,
                 "rows": torch.zeros(N, cap, 7, device=dev),
                 "counts": torch.zeros(N, device=dev, dtype=torch.int32),
                 "seg_begin": (torch.arange(N, dtype=torch.int32) * cap).to(dev),
                 "out_idx": torch.zeros(N * cap, device=dev, dtype=torch.int32),
                 "out": torch.zeros(N + 1, device=dev, dtype=torch.int32),     # out_counts [N] | NMS status [1]: read back in one copy
                 "out_rows": torch.zeros(N * cap, 7, device=dev),
                 "ws": torch.empty(_lib.query("mny_nms_ws_bytes", N, N * cap, C), device=dev, dtype=torch.uint8),
                 "x": {}}
            so = _lib.query("mny_nms_status_offset", N, N * cap, C)
            po = _lib.query("mny_nms_prefix_offset", N, N * cap, C)
            b["status"] = b["ws"][so:so + 4].view(torch.int32)
            b["prefix"] = b["ws"][po:po + 4 * (N + 1)].view(torch.int32)
            self._bufs[key] = b
        return b

    def view_input(self, x, index, out=None):
        """The input tensor of views[index] for the batch x [N,3,S,S] (an identity view: x itself, nothing is launched)."""
        size, flip = self.views[index]
        if size == x.shape[2] and size == x.shape[3] and not flip:
            return x
        return ops.tta_view(x, size, size, flip, out=out)

    def __call__(self, x):
        model = self.model
        if model.training:
            raise MnyError("TTA needs model.eval(): a decode in training mode would update the BatchNorm statistics once per view")
        x = model._check_input(x)
        N, _, H, W = x.shape
        if H != W or H != self.views[0][0]:
            raise ValueError("views[0] must be the identity view: the input is %dx%d, views[0] has size %d (square inputs only)"
                             % (H, W, self.views[0][0]))
        if self.post is not None:
            return self._call_post(x)
        val_conf = [float(h.val_conf) for h in model.yolo_losses]
        with torch.no_grad():
            plans = model._eval_plans(N, [s for s, _ in self.views], [H, W])
            b = self._buffers(N, [p.cap for p in plans], x.device)
            b["counts"].zero_()
            st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
            for k, ((size, flip), plan) in enumerate(zip(self.views, plans)):
                if k not in b["x"] and (size != H or flip):
                    b["x"][k] = torch.empty(N, 3, size, size, device=x.device)  # resident: the plan reads it through a raw pointer
                xv = self.view_input(x, k, out=b["x"].get(k))
                plan.forward_eval(xv, val_conf, nms=False)
                ops.det_append(plan.rows, plan.cnt1, b["rows"], b["counts"], flip=flip)
                if k == 0 and plan.seg_head is not None:
                    # views of the identity's size share its plan and overwrite these buffers: take the seg outputs now
                    self._seg = (plan.seg_head.to(torch.float32).clone(), plan.seg_eval.clone())
            C = model.num_classes
            cap = b["cap"]
            _lib.call("mny_nms_per_class", ops._p(b["rows"]), ops._p(b["seg_begin"]), ops._p(b["counts"]), N, N * cap, cap, C,
                      ctypes.c_double(self.nms_thr), ops._p(b["out_idx"]), ops._p(b["out"]), ops._p(b["out_rows"]),
                      ctypes.c_void_p(b["ws"].data_ptr()), st)
            if self.merge:
                ops.nms_merge(b["rows"].view(-1, 7), b["seg_begin"], b["counts"], b["out_idx"], b["out"][:N], b["prefix"], b["out_rows"],
                              thr=self.nms_thr)
            b["out"][N:].copy_(b["status"])
            host = b["out"].tolist()                                            # the one host sync of the call
            counts, status = host[:N], host[N]
            if status != 0:
                raise MnyError("NMS: a bucket of %d boxes exceeded the joint per-image candidate bound" % status)
            dets = b["out_rows"][:sum(counts)].clone()
        dets = list(torch.split(dets, counts))
        if plans[0].seg_head is not None:
            return dets, self._seg[1].cpu().numpy()                             # (output, seg_out) of the identity view, as model(images)
        return dets

    def _post_buffers(self, N, plans, dev):
        post, C = self.post, self.model.num_classes
        strides = [post.stride(p.cap, C) for p in plans]
        key = (N, tuple(strides), str(dev))
        b = self._bufs.get(key)
        if b is None:
            self._bufs.clear()                                                  # one batch shape resident at a time
            V = len(plans)
            b = postprocess.nms_buffers(post, C, N, sum(strides), dev, extra=2 * N * V)
            b.update({"cap": sum(strides),
                      "rows": torch.zeros(N, sum(strides), 7, device=dev),
                      "counts": torch.zeros(N, device=dev, dtype=torch.int32),
                      "view_rows": [torch.zeros(N, s, 7, device=dev) for s in strides],     # one view's candidates, before they are appended
                      "cnt0": torch.zeros(N, device=dev, dtype=torch.int32),
                      "cnt1": torch.zeros(N, device=dev, dtype=torch.int32),
                      "cmask": ops.class_mask(post.classes, C, dev) if post.classes is not None else None,
                      "x": {}})
            self._bufs[key] = b
        return b

    def _call_post(self, x):
        """The call with a PostProcess: the same views, appends and merge; decode, NMS and top-k by the options."""
        model, post = self.model, self.post
        N, _, H, W = x.shape
        C = model.num_classes
        val_conf = [float(h.val_conf) for h in model.yolo_losses]
        with torch.no_grad():
            plans = model._eval_plans(N, [s for s, _ in self.views], [H, W])
            b = self._post_buffers(N, plans, x.device)
            b["counts"].zero_()
            out = b["out"]
            for k, ((size, flip), plan) in enumerate(zip(self.views, plans)):
                if k not in b["x"] and (size != H or flip):
                    b["x"][k] = torch.empty(N, 3, size, size, device=x.device)  # resident: the plan reads it through a raw pointer
                xv = self.view_input(x, k, out=b["x"].get(k))
                plan.forward_eval(xv, val_conf, decode=False)
                d0 = N + 1 + 2 * N * k
                postprocess.decode_plan(plan, post, model, b["view_rows"][k], b["cnt0"], b["cnt1"], out[d0:d0 + N], out[d0 + N:d0 + 2 * N],
                                        b["cmask"])
                ops.det_append(b["view_rows"][k], b["cnt1"], b["rows"], b["counts"], flip=flip)
                if k == 0 and plan.seg_head is not None:
                    self._seg = (plan.seg_head.to(torch.float32).clone(), plan.seg_eval.clone())
            postprocess.run_nms(post, C, b["rows"], b["seg_begin"], b["counts"], b["out_idx"], out, b["out_rows"], b["ws"])
            prefix = postprocess.run_topk(post, b["rows"], b)
            if self.merge:
                ops.nms_merge(b["rows"].view(-1, 7), b["seg_begin"], b["counts"], b["out_idx"], out[:N], prefix, b["out_rows"], thr=self.nms_thr)
            out[N:N + 1].copy_(b["status"])
            host = out.tolist()                                                 # the one host sync of the call
            counts, status = host[:N], host[N]
            postprocess.check_dropped(host[N + 1:], N, " (a TTA view)")
            if status != 0:
                raise MnyError("NMS: a bucket of %d boxes exceeded the joint per-image candidate bound" % status)
            dets = b["out_rows"][:sum(counts)].clone()
        dets = list(torch.split(dets, counts))
        if plans[0].seg_head is not None:
            return dets, self._seg[1].cpu().numpy()
        return dets

    def seg_logits(self):
        """The identity view's raw seg logits of the last call, [N,h,w,C] fp32 on the device (what model.seg_logits() returns after
        model(images); a TTA call withdraws that one, because the views overwrite the plans' buffers)."""
        if not self.model.has_seg:
            raise MnyError("seg_logits: this config has no `seg:` section, the model has no segmentation head")
        if self._seg is None:
            raise MnyError("seg_logits: no TTA call has run yet")
        return self._seg[0].clone()
