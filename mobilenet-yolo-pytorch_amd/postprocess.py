"""Post-processing options of the detection path (Ultralytics' `non_max_suppression` protocol), on the device.

    post = PostProcess(conf_thres=0.001, score_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300)
    dets = Detector(model, post)(images)        # list of [k_i,7] device tensors: the contract of model.eval()(images)

`model(images)` keeps the reference's hard-wired post-processing (best class of every cell above `val_conf`, class-aware NMS, no cap).
A `Detector` runs the model's cached eval plan's forward and then its own decode (`mny_yolo_decode_ex`: a score threshold on
conf * cls, a candidate per (cell, class) pair with `multi_label`, a class filter), the class-aware or the class-agnostic NMS and, with
`max_det`, `mny_det_topk`.  One host sync per call (the final counts).  Opt-in: `Detector(model, PostProcess())(x)` equals `model(x)` bit
for bit, and `tta.TTA(..., post=...)` takes the same options.
"""
import ctypes

import torch

from . import _lib, ops
from ._lib import MnyError


def _unit(v, what):
    v = float(v)
    if not 0.0 <= v <= 1.0:                       # (a NaN fails both compares)
        raise ValueError("%s must lie in [0, 1], got %r" % (what, v))
    return v


class PostProcess:
    """A validated value object.
    conf_thres   objectness threshold (strict >); None: each head's `val_conf` at call time, as model(images)
    score_thres  threshold on conf * cls (strict >); None: no score test
    iou_thres    NMS threshold
    multi_label  a candidate per (cell, class) pair that passes, not only the cell's best class
    agnostic     class-agnostic NMS (one bucket per image); the rows keep their classes
    max_det      at most this many detections per image, by score; None: no cap
    classes      keep these class indices only; None: every class
    max_candidates  per-image bound of the candidate buffer; None: the worst case of the mode.  A call whose candidates do not fit
                 raises MnyError (nothing is dropped silently)."""

    def __init__(self, conf_thres=None, score_thres=None, iou_thres=0.45, multi_label=False, agnostic=False, max_det=None, classes=None,
                 max_candidates=None):
        self.conf_thres = None if conf_thres is None else _unit(conf_thres, "conf_thres")
        self.score_thres = None if score_thres is None else _unit(score_thres, "score_thres")
        self.iou_thres = _unit(iou_thres, "iou_thres")
        for name, v in (("multi_label", multi_label), ("agnostic", agnostic)):
            if not isinstance(v, (bool, int)) or v not in (0, 1):
                raise ValueError("%s must be True or False, got %r" % (name, v))
        self.multi_label = bool(multi_label)
        self.agnostic = bool(agnostic)
        for name, v in (("max_det", max_det), ("max_candidates", max_candidates)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
                raise ValueError("%s must be an integer >= 1 or None, got %r" % (name, v))
        self.max_det = max_det
        self.max_candidates = max_candidates
        if classes is not None:
            try:
                classes = list(classes)
            except TypeError:
                raise ValueError("classes must be a list of class indices or None, got %r" % (classes,))
            if not classes or any(isinstance(c, bool) or not isinstance(c, int) or c < 0 for c in classes):
                raise ValueError("classes must be a non-empty list of class indices >= 0, got %r" % (classes,))
            classes = sorted(set(classes))
        self.classes = classes

    def check_classes(self, num_classes):
        """`classes` must lie in 0..C-1 (C is the model's: checked where the model is known)."""
        if self.classes is not None and self.classes[-1] >= num_classes:
            raise ValueError("classes must lie in 0..%d, got %d" % (num_classes - 1, self.classes[-1]))

    def multi(self, num_classes):
        return self.multi_label and num_classes > 1

    def stride(self, cells, num_classes):
        """Per-image row stride for `cells` grid cells (all heads): the worst case of the mode, bounded by max_candidates."""
        per_cell = min(num_classes, len(self.classes) if self.classes is not None else num_classes) if self.multi(num_classes) else 1
        worst = cells * per_cell
        return worst if self.max_candidates is None else min(worst, self.max_candidates)

    def thresholds(self, model):
        """([obj_thr per head], score_thr) of a call"""
        obj = [float(h.val_conf) if self.conf_thres is None else self.conf_thres for h in model.yolo_losses]
        return obj, (-1.0 if self.score_thres is None else self.score_thres)

    def __repr__(self):
        return "PostProcess(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in (
            "conf_thres", "score_thres", "iou_thres", "multi_label", "agnostic", "max_det", "classes", "max_candidates"))


def decode_plan(plan, post, model, rows, cnt0, cnt1, drop0, drop1, cmask):
    """The plan's two heads through mny_yolo_decode_ex into rows [N,stride,7], the second head behind the first: cnt1 = the counts."""
    obj, score = post.thresholds(model)
    multi = int(post.multi(model.num_classes))
    st = ops._st()
    for hi, (base, cnt, drop) in enumerate(((None, cnt0, drop0), (cnt0, cnt1, drop1))):
        _lib.call("mny_yolo_decode_ex", ops._p(plan.heads[hi]), ops._p(plan.anchors[hi]), ops._p(plan.masks[hi]), ctypes.byref(plan.hp[hi]),
                  obj[hi], score, multi, ops._p(cmask), ops._p(rows), rows.shape[1], ops._p(base), ops._p(cnt), ops._p(drop), st)


def run_nms(post, num_classes, rows, seg_begin, counts, out_idx, out_counts, out_rows, ws):
    """The chosen NMS over rows [N,stride,7] (one segment per image) at post.iou_thres"""
    N, stride = rows.shape[0], rows.shape[1]
    thr, wsp = ctypes.c_double(post.iou_thres), ctypes.c_void_p(ws.data_ptr())
    if post.agnostic:
        _lib.call("mny_nms_agnostic", ops._p(rows), ops._p(seg_begin), ops._p(counts), N, N * stride, stride, thr, ops._p(out_idx),
                  ops._p(out_counts), ops._p(out_rows), wsp, ops._st())
    else:
        _lib.call("mny_nms_per_class", ops._p(rows), ops._p(seg_begin), ops._p(counts), N, N * stride, stride, num_classes, thr,
                  ops._p(out_idx), ops._p(out_counts), ops._p(out_rows), wsp, ops._st())


def nms_buffers(post, num_classes, N, stride, dev, extra=0):
    """Buffers of one NMS (+ top-k) over N segments of `stride` rows.  `out` = out_counts [N] | NMS status [1] | `extra` more int32 (the
    decode's dropped counts): read back in one copy."""
    cap = N * stride
    if post.agnostic:
        q = [_lib.query("mny_nms_agnostic_" + w, N, cap) for w in ("ws_bytes", "status_offset", "prefix_offset")]
    else:
        q = [_lib.query("mny_nms_" + w, N, cap, num_classes) for w in ("ws_bytes", "status_offset", "prefix_offset")]
    b = {"stride": stride,
         "seg_begin": (torch.arange(N, dtype=torch.int32) * stride).to(dev),
         "out_idx": torch.zeros(cap, device=dev, dtype=torch.int32),
         "out": torch.zeros(N + 1 + extra, device=dev, dtype=torch.int32),
         "out_rows": torch.zeros(cap, 7, device=dev),
         "ws": torch.empty(q[0], device=dev, dtype=torch.uint8)}
    b["status"] = b["ws"][q[1]:q[1] + 4].view(torch.int32)
    b["prefix"] = b["ws"][q[2]:q[2] + 4 * (N + 1)].view(torch.int32)
    if post.max_det is not None:
        b["topk_ws"] = torch.empty(_lib.query("mny_det_topk_ws_bytes", N, cap), device=dev, dtype=torch.uint8)
        b["topk_prefix"] = torch.zeros(N + 1, device=dev, dtype=torch.int32)
    return b


def run_topk(post, rows, b):
    """mny_det_topk on the NMS result in `b` (nms_buffers); -> the prefix that holds afterwards"""
    if post.max_det is None:
        return b["prefix"]
    N = rows.shape[0]
    _lib.call("mny_det_topk", ops._p(rows), ops._p(b["seg_begin"]), N, N * rows.shape[1], post.max_det, ops._p(b["out_idx"]), ops._p(b["out"]),
              ops._p(b["out_rows"]), ops._p(b["topk_prefix"]), ctypes.c_void_p(b["topk_ws"].data_ptr()), ops._st())
    return b["topk_prefix"]


def check_dropped(dropped, N, what=""):
    """dropped: host list, N entries per decode call"""
    for k, d in enumerate(dropped):
        if d:
            raise MnyError("decode%s: image %d has %d candidates more than the candidate buffer holds (head %d): raise max_candidates "
                           "or the thresholds" % (what, k % N, d, (k // N) % 2))


class Detector:
    def __init__(self, model, post=None):
        post = PostProcess() if post is None else post
        if not isinstance(post, PostProcess):
            raise ValueError("post must be a PostProcess, got %r" % (post,))
        post.check_classes(model.num_classes)
        self.model = model
        self.post = post
        self._bufs = {}

    def _buffers(self, plan, N, dev):
        key = (N, plan.cap, str(dev))
        b = self._bufs.get(key)
        if b is None:
            self._bufs.clear()                                                  # one batch shape resident at a time
            C = self.model.num_classes
            stride = self.post.stride(plan.cap, C)
            b = nms_buffers(self.post, C, N, stride, dev, extra=2 * N)
            b["rows"] = torch.zeros(N, stride, 7, device=dev)
            b["cnt0"] = torch.zeros(N, device=dev, dtype=torch.int32)
            b["cnt1"] = torch.zeros(N, device=dev, dtype=torch.int32)
            b["cmask"] = ops.class_mask(self.post.classes, C, dev) if self.post.classes is not None else None
            self._bufs[key] = b
        return b

    def __call__(self, x):
        model, post = self.model, self.post
        if model.training:
            raise MnyError("Detector needs model.eval(): a decode in training mode would update the BatchNorm statistics")
        x = model._check_input(x)
        N, _, H, W = x.shape
        C = model.num_classes
        with torch.no_grad():
            for hs in model.yolo_losses:
                hs.img_size = [H, W]                                            # mbv2_yolo.py:139-140, as model(images)
            plan = model._plan(N, H, W, False)
            b = self._buffers(plan, N, x.device)
            plan.forward_eval(x, [float(h.val_conf) for h in model.yolo_losses], decode=False)
            model._eval_plan = plan                                             # seg_logits() reads this call's seg head
            out = b["out"]
            decode_plan(plan, post, model, b["rows"], b["cnt0"], b["cnt1"], out[N + 1:2 * N + 1], out[2 * N + 1:], b["cmask"])
            run_nms(post, C, b["rows"], b["seg_begin"], b["cnt1"], b["out_idx"], out, b["out_rows"], b["ws"])
            run_topk(post, b["rows"], b)
            out[N:N + 1].copy_(b["status"])
            host = out.tolist()                                                 # the one host sync of the call
            counts, status = host[:N], host[N]
            check_dropped(host[N + 1:], N)
            if status != 0:
                raise MnyError("NMS: a bucket of %d boxes exceeded the per-image candidate bound" % status)
            dets = b["out_rows"][:sum(counts)].clone()
        dets = list(torch.split(dets, counts))
        if plan.seg_head is not None:
            return dets, plan.seg_eval.cpu().numpy()                            # (output, seg_out), as model(images)
        return dets
