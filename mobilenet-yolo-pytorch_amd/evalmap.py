"""Evaluation consumer of the detection path: VOC07 11-point mAP and COCO-style AP / AR on the device.

Host-side mirror of the reference's interface — `calculate_mAP` keeps the name, argument list and return
value of utils/eval_mAP.py:134-187, `adjust_confidence` is train.py:434-440 — over `mny_map_eval`
(csrc/evalmap.hip).  `Evaluator` is the loop body of train.py:test() (:359-395) without the per-image Python:
detections stay in the packed [k,7] rows the NMS stage wrote and are converted by `mny_eval_pack`.
`coco_eval` / `Evaluator.compute_coco` score the same packed detections by the COCO protocol (AP over IoU 0.50:0.05:0.95, by
object size, AR at 1 / 10 / 100 detections) over `mny_coco_eval` (csrc/cocoeval.hip); its arithmetic is specified in
include/mnyolo.h and is not pinned against pycocotools.
`det_curves` / `det_confusion` / `Evaluator.compute_report` turn the match flags `coco_eval` leaves on the device into per-class
precision / recall / F1 curves, the confidence that maximises F1, and a detection confusion matrix (`mny_det_curves`,
`mny_det_confusion`, csrc/detreport.hip).
There is no CPU fallback: without libmnyolo.so every call raises MnyError.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, query


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    return t.detach().to(dtype=torch.float32).contiguous()


def map_eval(det_boxes, det_labels, det_scores, det_off, true_boxes, true_labels, true_diff, true_off, n_classes):
    """Packed inputs on one CUDA device (float32; offsets int32 [n_images+1]); n_classes counts the background entry.
    -> dict of device tensors: ap [n-1], tp [n-1], fp [n-1], prec11 [n-1,11], mean_ap [1].  No host sync."""
    dev = det_off.device
    if dev.type != "cuda":
        raise RuntimeError("map_eval needs CUDA tensors (the HIP path is the only path)")
    D, T, n_img = int(det_labels.numel()), int(true_labels.numel()), int(det_off.numel()) - 1
    args = [_f32(det_boxes), _f32(det_labels), _f32(det_scores), det_off.to(torch.int32).contiguous(),
            _f32(true_boxes), _f32(true_labels), _f32(true_diff), true_off.to(torch.int32).contiguous()]
    if true_off.numel() != n_img + 1:
        raise ValueError("det_off and true_off describe different numbers of images")
    nb = query("mny_map_ws_bytes", D, T)
    ws = torch.empty(max(int(nb), 256), device=dev, dtype=torch.uint8)
    out = torch.empty(14 * (n_classes - 1) + 1, device=dev, dtype=torch.float32)
    n = n_classes - 1
    ap, tp, fp, p11, mean = out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:14 * n], out[14 * n:]
    call("mny_map_eval", *[_p(a) for a in args], n_img, D, T, int(n_classes), _p(ap), _p(tp), _p(fp), _p(p11), _p(mean),
         ctypes.c_void_p(ws.data_ptr()), _st())
    return {"ap": ap, "tp": tp, "fp": fp, "prec11": p11.view(n, 11), "mean_ap": mean, "_keepalive": (args, ws)}


COCO_STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
COCO_LIMITS = {"iou_thrs": 16, "rec_thrs": 128, "max_dets": 4, "area_rngs": 8, "stat_desc": 32}


def coco_defaults():
    """The package's Params for iouType='bbox'."""
    return {"iou_thrs": np.linspace(.5, .95, 10), "rec_thrs": np.linspace(0, 1, 101), "max_dets": (1, 10, 100),
            "area_rngs": np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)}


def _coco_default_stats(iou_thrs, n_area, n_maxdet):
    """(is_recall, IoU index or -1, area index, cap index) of COCO_STAT_NAMES; needs the default shape of the parameters."""
    i50, i75 = [int(np.argmin(np.abs(iou_thrs - v))) for v in (.5, .75)]
    if n_area != 4 or n_maxdet != 3 or abs(iou_thrs[i50] - .5) > 1e-9 or abs(iou_thrs[i75] - .75) > 1e-9:
        raise ValueError("the twelve default statistics need thresholds with 0.5 and 0.75, four area_rngs and three max_dets; pass stat_desc")
    return [[0, -1, 0, 2], [0, i50, 0, 2], [0, i75, 0, 2], [0, -1, 1, 2], [0, -1, 2, 2], [0, -1, 3, 2],
            [1, -1, 0, 0], [1, -1, 0, 1], [1, -1, 0, 2], [1, -1, 1, 2], [1, -1, 2, 2], [1, -1, 3, 2]]


def coco_eval(det_boxes, det_labels, det_scores, det_off, true_boxes, true_labels, true_crowd, true_off, n_classes, image_sizes=None,
              iou_thrs=None, rec_thrs=None, max_dets=None, area_rngs=None, stat_desc=None, matches=False):
    """COCO-style metrics of packed inputs on one CUDA device (float32; offsets int32 [n_images+1]; image_sizes [n_images,2] = (w, h)
    or None = (1, 1)); n_classes counts the background entry.  Parameters default to `coco_defaults()`, stat_desc to the twelve
    numbers of COCO_STAT_NAMES.  -> dict of device tensors (float64): precision [T,R,K,A,M], recall [T,K,A,M], stats [S],
    per_class_ap [K]; with matches=True also det_match [A,T,D] int32 and det_ignore [A,T,D] uint8 in stored order.  No host sync."""
    d = coco_defaults()
    iou_thrs = np.ascontiguousarray(d["iou_thrs"] if iou_thrs is None else iou_thrs, np.float64).reshape(-1)
    rec_thrs = np.ascontiguousarray(d["rec_thrs"] if rec_thrs is None else rec_thrs, np.float64).reshape(-1)
    max_dets = np.ascontiguousarray(d["max_dets"] if max_dets is None else max_dets, np.int32).reshape(-1)
    area_rngs = np.ascontiguousarray(d["area_rngs"] if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    if stat_desc is None:
        stat_desc = _coco_default_stats(iou_thrs, len(area_rngs), len(max_dets))
    stat_desc = np.ascontiguousarray(stat_desc, np.int32).reshape(-1, 4)
    for name, arr in (("iou_thrs", iou_thrs), ("rec_thrs", rec_thrs), ("max_dets", max_dets), ("area_rngs", area_rngs), ("stat_desc", stat_desc)):
        if not 1 <= len(arr) <= COCO_LIMITS[name]:
            raise ValueError("%s has %d entries; 1..%d are supported" % (name, len(arr), COCO_LIMITS[name]))
    if max_dets[0] < 1 or (np.diff(max_dets) < 0).any():
        raise ValueError("max_dets must be positive and ascending")
    if not 2 <= int(n_classes) <= 255:
        raise ValueError("n_classes %d outside 2..255 (it counts the background entry)" % n_classes)
    n_img = int(det_off.numel()) - 1
    if true_off.numel() != n_img + 1:
        raise ValueError("det_off and true_off describe different numbers of images")
    if image_sizes is not None and tuple(image_sizes.shape) != (n_img, 2):
        raise ValueError("image_sizes must be [n_images, 2] = (w, h)")
    dev = det_off.device
    if dev.type != "cuda":
        raise RuntimeError("coco_eval needs CUDA tensors (the HIP path is the only path)")
    D, T = int(det_labels.numel()), int(true_labels.numel())
    args = [_f32(det_boxes), _f32(det_labels), _f32(det_scores), det_off.to(torch.int32).contiguous(),
            _f32(true_boxes), _f32(true_labels), _f32(true_crowd), true_off.to(torch.int32).contiguous(),
            _f32(image_sizes) if image_sizes is not None else None]
    K, nt, nr, na, nm, S = int(n_classes) - 1, len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets), len(stat_desc)
    nb = query("mny_coco_ws_bytes", D, T, n_img, int(n_classes), nt, nr, na, nm)
    ws = torch.empty(max(int(nb), 256), device=dev, dtype=torch.uint8)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {"precision": f64(nt, nr, K, na, nm), "recall": f64(nt, K, na, nm), "stats": f64(S), "per_class_ap": f64(K)}
    if matches:
        out["det_match"] = torch.empty(na, nt, max(D, 1), device=dev, dtype=torch.int32)[:, :, :D]
        out["det_ignore"] = torch.empty(na, nt, max(D, 1), device=dev, dtype=torch.uint8)[:, :, :D]
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call("mny_coco_eval", *[_p(a) for a in args], n_img, D, T, int(n_classes), hp(iou_thrs), nt, hp(rec_thrs), nr, hp(max_dets), nm,
         hp(area_rngs), na, hp(stat_desc), S, _p(out["precision"]), _p(out["recall"]), _p(out["stats"]), _p(out["per_class_ap"]),
         _p(out.get("det_match")) if D else None, _p(out.get("det_ignore")) if D else None, ctypes.c_void_p(ws.data_ptr()), _st())
    out["_keepalive"] = (args, ws)
    return out


def det_curves(det_labels, det_scores, det_match, det_ignore, true_labels, true_crowd, n_classes, grid=1000, smooth=101):
    """Precision / recall / F1 of every class over `grid` confidences c_j = j / (grid-1), and the confidence that maximises the mean F1
    smoothed over an odd window of `smooth` points (`mny_det_curves`, csrc/detreport.hip; specified in include/mnyolo.h).  det_match [D]
    int32 / det_ignore [D] uint8 are one [area, iou] slice of `coco_eval(..., matches=True)`.  The curves are exact step functions of the
    set {score >= c}.  -> dict of device tensors: tp, fp [K,G] int64; npos [K] int64; precision, recall, f1 [K,G], mean_f1, smooth_f1 [G]
    float64 (-1: class without positives); best [1] int32, best_conf [1] float64, at_best [K+1,3] = (P, R, F1) per class at `best`, last
    row their means.  No host sync."""
    if not 2 <= int(n_classes) <= 255:
        raise ValueError("n_classes %d outside 2..255 (it counts the background entry)" % n_classes)
    G, W = int(grid), int(smooth)
    if not 2 <= G <= 4096:
        raise ValueError("grid %d outside 2..4096" % G)
    if not (1 <= W <= G and W % 2 == 1):
        raise ValueError("smooth %d is not an odd number in 1..grid" % W)
    D, T = int(det_labels.numel()), int(true_labels.numel())
    if not (det_scores.numel() == det_match.numel() == det_ignore.numel() == D) or true_crowd.numel() != T:
        raise ValueError("det_labels / det_scores / det_match / det_ignore, or true_labels / true_crowd, differ in length")
    dev = det_labels.device
    if dev.type != "cuda":
        raise RuntimeError("det_curves needs CUDA tensors (the HIP path is the only path)")
    args = [_f32(det_labels), _f32(det_scores), det_match.to(torch.int32).contiguous(), det_ignore.to(torch.uint8).contiguous(),
            _f32(true_labels), _f32(true_crowd)]
    K = int(n_classes) - 1
    nb = query("mny_det_curves_ws_bytes", D, T, int(n_classes), G, W)
    ws = torch.empty(max(int(nb), 256), device=dev, dtype=torch.uint8)
    i64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int64)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {"tp": i64(K, G), "fp": i64(K, G), "npos": i64(K), "precision": f64(K, G), "recall": f64(K, G), "f1": f64(K, G), "mean_f1": f64(G),
           "smooth_f1": f64(G), "best": torch.empty(1, device=dev, dtype=torch.int32), "best_conf": f64(1), "at_best": f64(K + 1, 3)}
    call("mny_det_curves", _p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), D, _p(args[4]), _p(args[5]), T, int(n_classes), G, W,
         *[_p(out[k]) for k in ("tp", "fp", "npos", "precision", "recall", "f1", "mean_f1", "smooth_f1", "best", "best_conf", "at_best")],
         ctypes.c_void_p(ws.data_ptr()), _st())
    out["_keepalive"] = (args, ws)
    return out


def det_confusion(det_boxes, det_labels, det_scores, det_off, true_boxes, true_labels, true_crowd, true_off, n_classes, image_sizes=None,
                  conf=0.25, iou_thr=0.45, out=None):
    """Detection confusion matrix of packed inputs (the layout of `coco_eval`) on one CUDA device (`mny_det_confusion`, csrc/detreport.hip):
    per image the detections with score > conf are matched one-to-one to the ground truths, classes not compared, largest IoU > iou_thr
    first.  -> dict of device tensors: matrix [K+1,K+1] int64 (row = predicted class, column = true class, index K = background), det_gt [D]
    int32 (packed index of the matched ground truth, -1 unmatched, -2 not considered).  out= a matrix of an earlier call: it is added to
    and returned, so a loop can call this once per batch.  No host sync."""
    if not 2 <= int(n_classes) <= 255:
        raise ValueError("n_classes %d outside 2..255 (it counts the background entry)" % n_classes)
    conf, iou_thr = float(conf), float(iou_thr)
    if not 0.0 <= conf <= 1.0:
        raise ValueError("conf %r outside 0..1" % conf)
    if not 0.0 <= iou_thr <= 1.0:
        raise ValueError("iou_thr %r outside 0..1" % iou_thr)
    n_img = int(det_off.numel()) - 1
    if true_off.numel() != n_img + 1:
        raise ValueError("det_off and true_off describe different numbers of images")
    if image_sizes is not None and tuple(image_sizes.shape) != (n_img, 2):
        raise ValueError("image_sizes must be [n_images, 2] = (w, h)")
    K = int(n_classes) - 1
    dev = det_off.device
    if dev.type != "cuda":
        raise RuntimeError("det_confusion needs CUDA tensors (the HIP path is the only path)")
    if out is not None and (tuple(out.shape) != (K + 1, K + 1) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous()):
        raise ValueError("out must be a contiguous int64 [%d,%d] matrix on %s" % (K + 1, K + 1, dev))
    D, T = int(det_labels.numel()), int(true_labels.numel())
    args = [_f32(det_boxes), _f32(det_labels), _f32(det_scores), det_off.to(torch.int32).contiguous(),
            _f32(true_boxes), _f32(true_labels), _f32(true_crowd), true_off.to(torch.int32).contiguous(),
            _f32(image_sizes) if image_sizes is not None else None]
    nb = query("mny_det_confusion_ws_bytes", D, T, n_img, int(n_classes))
    ws = torch.empty(max(int(nb), 256), device=dev, dtype=torch.uint8)
    matrix = out if out is not None else torch.empty(K + 1, K + 1, device=dev, dtype=torch.int64)
    det_gt = torch.empty(max(D, 1), device=dev, dtype=torch.int32)[:D]
    call("mny_det_confusion", *[_p(a) for a in args], n_img, D, T, int(n_classes), conf, iou_thr, 1 if out is not None else 0, _p(matrix),
         _p(det_gt), ctypes.c_void_p(ws.data_ptr()), _st())
    return {"matrix": matrix, "det_gt": det_gt, "_keepalive": (args, ws)}


def _pack_list(ts, width, dev):
    ts = [t.reshape(-1, width) if width else t.reshape(-1) for t in ts]
    off = torch.tensor([0] + [int(t.shape[0]) for t in ts], dtype=torch.int64).cumsum(0).to(torch.int32)
    if ts:
        flat = torch.cat([t.to(dev, torch.float32) for t in ts])
    else:
        flat = torch.zeros((0, width) if width else (0,), device=dev)
    return flat, off.to(dev)


def calculate_mAP(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_difficulties, classes_name, device=None):
    """Drop-in for utils/eval_mAP.py:134-187: lists with one tensor per image, `classes_name` with 'background' first.
    -> (average_precisions {name: AP}, mean_average_precision, class_true_positive {name: n}, class_false_positive {name: n})."""
    assert len(det_boxes) == len(det_labels) == len(det_scores) == len(true_boxes) == len(true_labels) == len(true_difficulties)
    dev = torch.device(device) if device is not None else next((t.device for t in list(det_boxes) + list(true_boxes) if t.is_cuda), torch.device("cuda:0"))
    db, do = _pack_list(det_boxes, 4, dev)
    dl, _ = _pack_list(det_labels, 0, dev)
    ds, _ = _pack_list(det_scores, 0, dev)
    tb, to = _pack_list(true_boxes, 4, dev)
    tl, _ = _pack_list(true_labels, 0, dev)
    td, _ = _pack_list(true_difficulties, 0, dev)
    r = map_eval(db, dl, ds, do, tb, tl, td, to, len(classes_name))
    ap, tp, fp, m = r["ap"].tolist(), r["tp"].tolist(), r["fp"].tolist(), float(r["mean_ap"])
    names = list(classes_name)[1:]
    return dict(zip(names, ap)), m, dict(zip(names, tp)), dict(zip(names, fp))


def adjust_confidence(gt_box_num, pred_box_num, conf):
    """train.py:434-440 (host logic)."""
    if pred_box_num > gt_box_num * 3:
        conf = conf + 0.01
    elif pred_box_num < gt_box_num * 2 and conf > 0.01:
        conf = conf - 0.01
    return conf


class Evaluator:
    """Accumulates an evaluation set on the device and scores it once (train.py:359-421).

        ev = Evaluator(classes_name)
        for images, targets in loader:
            ev.add(model(images), targets)           # list of [k_i,7] rows per image, list of [t_i,5] targets
        aps, mAP, tp, fp = ev.compute()
        coco = ev.compute_coco(image_size=(W, H))    # or per-image sizes given to add(..., sizes=[(w, h), ...])
    """

    def __init__(self, classes_name):
        self.classes_name = list(classes_name)
        self.rows, self.row_counts, self.tg, self.tg_counts = [], [], [], []
        self.sizes, self.crowd = [], []              # per image: (w, h) or None; per image: [t_i] flags (COCO metrics only)
        self.gt_box = self.pred_box = 0

    def _note(self, targets, sizes, crowd):
        n = len(targets)
        if sizes is not None and len(sizes) != n:
            raise ValueError("sizes must hold one (w, h) per image")
        if crowd is not None and len(crowd) != n:
            raise ValueError("crowd must hold one flag vector per image")
        for i, t in enumerate(targets):
            k = int(torch.as_tensor(t).reshape(-1, 5).shape[0])
            self.sizes.append(None if sizes is None else (float(sizes[i][0]), float(sizes[i][1])))
            c = torch.zeros(k) if crowd is None else torch.as_tensor(crowd[i], dtype=torch.float32).reshape(-1).cpu()
            if c.numel() != k:
                raise ValueError("crowd[%d] has %d flags for %d objects" % (i, c.numel(), k))
            self.crowd.append(c)

    def add(self, detections, targets, sizes=None, crowd=None):
        dets = [d if d is not None else None for d in detections]
        dev = next((d.device for d in dets if d is not None), torch.device("cuda:0"))
        self._note(list(targets)[:len(dets)], sizes, crowd)
        for d, t in zip(dets, targets):
            t = torch.as_tensor(t, dtype=torch.float32).reshape(-1, 5)
            k = 0 if d is None else int(d.shape[0])
            if k:
                self.rows.append(d.reshape(-1, 7).to(dev, torch.float32))
            self.row_counts.append(k)
            self.tg.append(t)
            self.tg_counts.append(int(t.shape[0]))
            self.gt_box += int(t.shape[0])
            self.pred_box += k

    def add_packed(self, rows, counts, targets, sizes=None, crowd=None):
        """rows [sum(counts),7] on the device (what the NMS stage wrote), counts: python ints per image."""
        self._note(list(targets), sizes, crowd)
        if rows.shape[0]:
            self.rows.append(rows.reshape(-1, 7).to(torch.float32))
        self.row_counts += [int(c) for c in counts]
        for t in targets:
            t = torch.as_tensor(t, dtype=torch.float32).reshape(-1, 5)
            self.tg.append(t)
            self.tg_counts.append(int(t.shape[0]))
            self.gt_box += int(t.shape[0])
        self.pred_box += int(rows.shape[0])

    def _packed(self, device=None):
        dev = torch.device(device) if device is not None else (self.rows[0].device if self.rows else torch.device("cuda:0"))
        rows = torch.cat(self.rows) if self.rows else torch.zeros(0, 7, device=dev)
        tg = (torch.cat(self.tg) if self.tg else torch.zeros(0, 5)).to(dev)
        D, T = int(rows.shape[0]), int(tg.shape[0])
        f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        db, dl, ds, tb, tl, td = f(max(D, 1), 4), f(max(D, 1)), f(max(D, 1)), f(max(T, 1), 4), f(max(T, 1)), f(max(T, 1))
        call("mny_eval_pack", _p(rows), D, _p(tg), T, _p(db), _p(dl), _p(ds), _p(tb), _p(tl), _p(td), _st())
        off = lambda c: torch.tensor([0] + c, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
        return db[:D], dl[:D], ds[:D], off(self.row_counts), tb[:T], tl[:T], td[:T], off(self.tg_counts)

    def compute_device(self, device=None):
        return map_eval(*self._packed(device), len(self.classes_name))

    def compute_coco_device(self, image_size=None, device=None, **params):
        """-> the dict of `coco_eval` (device tensors, no host sync); **params: iou_thrs, rec_thrs, max_dets, area_rngs, stat_desc."""
        if image_size is None and any(s is None for s in self.sizes):
            raise ValueError("compute_coco needs image_size=(W, H), or sizes= at every add(): area ranges are in pixels")
        sizes = [s if s is not None else (float(image_size[0]), float(image_size[1])) for s in self.sizes]
        db, dl, ds, do, tb, tl, _, to = self._packed(device)
        dev = do.device
        crowd = (torch.cat(self.crowd) if self.crowd else torch.zeros(0)).to(dev)
        return coco_eval(db, dl, ds, do, tb, tl, crowd, to, len(self.classes_name),
                         image_sizes=torch.tensor(sizes, dtype=torch.float32).reshape(-1, 2).to(dev), **params)

    def compute_coco(self, image_size=None, device=None):
        """COCO protocol with the package's default parameters -> {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100",
        "ARs", "ARm", "ARl"} as floats (-1: undefined) + "per_class_AP" {name: AP}.  Image sizes come from add(..., sizes=), else
        from image_size=(W, H)."""
        r = self.compute_coco_device(image_size, device)
        out = dict(zip(COCO_STAT_NAMES, r["stats"].tolist()))
        out["per_class_AP"] = dict(zip(self.classes_name[1:], r["per_class_ap"].tolist()))
        return out

    def compute_report_device(self, image_size=None, iou=0.5, max_det=100, device=None, **params):
        """Validation report on the device, no host sync: `coco_eval` at the one threshold `iou`, all areas and at most `max_det`
        detections per (image, class) gives the match flags; `det_curves` turns them into P / R / F1 curves and the best confidence;
        `det_confusion` builds the confusion matrix.  **params: grid, smooth (det_curves), conf, iou_thr (det_confusion).
        -> {"curves": dict of det_curves, "confusion": dict of det_confusion, "coco": dict of coco_eval}."""
        cp = {k: params.pop(k) for k in ("grid", "smooth") if k in params}
        fp = {k: params.pop(k) for k in ("conf", "iou_thr") if k in params}
        if params:
            raise TypeError("compute_report: unknown parameters %s" % sorted(params))
        if image_size is None and any(s is None for s in self.sizes):
            raise ValueError("compute_report needs image_size=(W, H), or sizes= at every add()")
        sizes = [s if s is not None else (float(image_size[0]), float(image_size[1])) for s in self.sizes]
        db, dl, ds, do, tb, tl, _, to = self._packed(device)
        dev = do.device
        crowd = (torch.cat(self.crowd) if self.crowd else torch.zeros(0)).to(dev)
        isz = torch.tensor(sizes, dtype=torch.float32).reshape(-1, 2).to(dev)
        nc = len(self.classes_name)
        coco = coco_eval(db, dl, ds, do, tb, tl, crowd, to, nc, image_sizes=isz, iou_thrs=[float(iou)], area_rngs=[[0, 1e10]],
                         max_dets=[int(max_det)], stat_desc=[[0, 0, 0, 0]], matches=True)
        curves = det_curves(dl, ds, coco["det_match"][0, 0], coco["det_ignore"][0, 0], tl, crowd, nc, **cp)
        confusion = det_confusion(db, dl, ds, do, tb, tl, crowd, to, nc, image_sizes=isz, **fp)
        return {"curves": curves, "confusion": confusion, "coco": coco}

    def compute_report(self, image_size=None, iou=0.5, max_det=100, device=None, **params):
        """-> {"best_conf", "P", "R", "F1" (means over the classes with positives at best_conf; -1 without any), "per_class": {name: (P, R,
        F1, n_pos)}, "confusion": int64 ndarray [K+1,K+1] (row = predicted, column = true, last = background), "curves": {"conf",
        "precision", "recall", "f1", "mean_f1", "smooth_f1", "tp", "fp"} as ndarrays}.  best_conf is a threshold on the score the metrics
        use, obj * cls_conf."""
        r = self.compute_report_device(image_size, iou, max_det, device, **params)
        c = {k: v.cpu().numpy() for k, v in r["curves"].items() if not k.startswith("_")}
        G = c["mean_f1"].shape[0]
        at, npos, names = c["at_best"], c["npos"], self.classes_name[1:]
        curves = {k: c[k] for k in ("precision", "recall", "f1", "mean_f1", "smooth_f1", "tp", "fp")}
        curves["conf"] = np.arange(G, dtype=np.float64) / (G - 1)
        return {"best_conf": float(c["best_conf"][0]), "P": float(at[-1, 0]), "R": float(at[-1, 1]), "F1": float(at[-1, 2]),
                "per_class": {n: (float(at[k, 0]), float(at[k, 1]), float(at[k, 2]), int(npos[k])) for k, n in enumerate(names)},
                "confusion": r["confusion"]["matrix"].cpu().numpy(), "curves": curves}

    def compute(self, device=None):
        r = self.compute_device(device)
        names = self.classes_name[1:]
        return dict(zip(names, r["ap"].tolist())), float(r["mean_ap"]), dict(zip(names, r["tp"].tolist())), dict(zip(names, r["fp"].tolist()))
