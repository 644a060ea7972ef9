"""Restatement of pycocotools.cocoeval.COCOeval for iouType='bbox' on the packed layout of `mny_coco_eval`
(include/mnyolo.h): numpy, every quantity in float64, written for reading and not for speed.

pycocotools is not installed where this project is developed, so nothing here is pinned against the package itself:
the arithmetic below IS the specification of the device kernels (csrc/cocoeval.hip), and the known answers of
tests/test_coco_ref_cpu.py are what holds it in place.  Function names follow the package (computeIoU / evaluateImg /
accumulate / summarize).

Inputs: det_boxes [D,4], det_labels [D], det_scores [D], det_off [n+1], true_boxes [T,4], true_labels [T],
true_crowd [T], true_off [n+1] (float32 / int32, boxes normalised xyxy), image_sizes [n,2] = (w, h) or None = (1, 1).
Classes 1..n_classes-1; a label that is not an integer in that range is never evaluated.
"""
import numpy as np

EPS = 2.220446049250313e-16          # np.spacing(1)


def default_params():
    return {"iou_thrs": np.linspace(.5, .95, 10), "rec_thrs": np.linspace(0, 1, 101), "max_dets": (1, 10, 100),
            "area_rngs": np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], np.float64)}


# (is_recall, iou index or -1 = all, area index, cap index) of the package's twelve numbers, for the default parameters
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
DEFAULT_STATS = np.array([[0, -1, 0, 2], [0, 0, 0, 2], [0, 5, 0, 2], [0, -1, 1, 2], [0, -1, 2, 2], [0, -1, 3, 2],
                          [1, -1, 0, 0], [1, -1, 0, 1], [1, -1, 0, 2], [1, -1, 1, 2], [1, -1, 2, 2], [1, -1, 3, 2]], np.int32)


def classes_of(labels, n_classes):
    """-> int array: the class of each label, 0 where the label is not an integer in 1..n_classes-1"""
    out = np.zeros(len(labels), np.int64)
    for i, v in enumerate(labels):
        v = float(v)
        if 1.0 <= v <= float(n_classes - 1) and v == int(v):
            out[i] = int(v)
    return out


def geometry(box, W, H):
    """-> (X1, Y1, w, h, area) in pixels, float64"""
    x1, y1, x2, y2 = (float(v) for v in box)
    X1, Y1, X2, Y2 = x1 * W, y1 * H, x2 * W, y2 * H
    w, h = X2 - X1, Y2 - Y1
    return X1, Y1, w, h, w * h


def iou(d, g, crowd):
    """maskApi.c bbIou on (x, y, w, h): the far corner is re-formed from x + w"""
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if iw <= 0:
        return 0.0
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if ih <= 0:
        return 0.0
    inter = iw * ih
    union = d[4] if crowd else (d[4] + g[4]) - inter
    return inter / union


def evaluate_img(dts, gts, crowd, iou_thrs, area_rng, table):
    """COCOeval.evaluateImg for one (image, class, area range).  dts / gts: geometries (detections already in score order and
    cut), table[d][g] the IoUs.  -> dtm [T_,nd] (index into gts or -1), dt_ig [T_,nd] bool, gt_ig [ng] bool"""
    lo, hi = float(area_rng[0]), float(area_rng[1])
    gt_ig = np.array([bool(crowd[j]) or g[4] < lo or g[4] > hi for j, g in enumerate(gts)], bool)
    order = [j for j in range(len(gts)) if not gt_ig[j]] + [j for j in range(len(gts)) if gt_ig[j]]
    n_t, nd = len(iou_thrs), len(dts)
    dtm = -np.ones((n_t, nd), np.int64)
    dt_ig = np.zeros((n_t, nd), bool)
    for ti, t in enumerate(iou_thrs):
        gtm = [False] * len(gts)
        for di in range(nd):
            best = min(float(t), 1 - 1e-10)
            m = -1
            row = table[di]
            for j in order:
                if gtm[j] and not crowd[j]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[j]:
                    break
                if row[j] < best:
                    continue
                best = row[j]
                m = j
            if m == -1:
                continue
            dt_ig[ti, di] = gt_ig[m]
            dtm[ti, di] = m
            gtm[m] = True
    out = np.array([d[4] < lo or d[4] > hi for d in dts], bool).reshape(1, nd)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == -1, np.repeat(out, n_t, 0)))
    return dtm, dt_ig, gt_ig


def evaluate(det_boxes, det_labels, det_scores, det_off, true_boxes, true_labels, true_crowd, true_off, n_classes,
             image_sizes=None, iou_thrs=None, rec_thrs=None, max_dets=None, area_rngs=None, stat_desc=None):
    """-> dict: precision [T_,R,K,A,M], recall [T_,K,A,M], stats [S], per_class_ap [K] (float64, -1 = undefined),
    det_match [A,T_,D] int32 (stored order: packed ground-truth index, -1 unmatched, -2 not evaluated), det_ignore [A,T_,D] uint8"""
    p = default_params()
    iou_thrs = np.asarray(p["iou_thrs"] if iou_thrs is None else iou_thrs, np.float64)
    rec_thrs = np.asarray(p["rec_thrs"] if rec_thrs is None else rec_thrs, np.float64)
    max_dets = [int(v) for v in (p["max_dets"] if max_dets is None else max_dets)]
    area_rngs = np.asarray(p["area_rngs"] if area_rngs is None else area_rngs, np.float64).reshape(-1, 2)
    stat_desc = np.asarray(DEFAULT_STATS if stat_desc is None else stat_desc, np.int64).reshape(-1, 4)
    n_img, D = len(det_off) - 1, len(det_labels)
    K, n_t, n_r, n_a, n_m = n_classes - 1, len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets)
    dcls, gcls = classes_of(det_labels, n_classes), classes_of(true_labels, n_classes)
    det_match = np.full((n_a, n_t, D), -2, np.int32)
    det_ignore = np.zeros((n_a, n_t, D), np.uint8)

    # ---- evaluate: per (image, class), per area range ------------------------------------------------------------------
    evals = {}                                           # (class, area, image) -> dict, only where the pair has a detection or an object
    for i in range(n_img):
        W, H = (1.0, 1.0) if image_sizes is None else (float(image_sizes[i][0]), float(image_sizes[i][1]))
        d0, d1, g0, g1 = int(det_off[i]), int(det_off[i + 1]), int(true_off[i]), int(true_off[i + 1])
        for c in range(1, n_classes):
            di = np.array([d for d in range(d0, d1) if dcls[d] == c], np.int64)
            gi = [g for g in range(g0, g1) if gcls[g] == c]
            if len(di) == 0 and len(gi) == 0:
                continue
            if len(di):
                di = di[np.argsort(-det_scores[di], kind="mergesort")][:max_dets[-1]]     # stable; -0.0 == 0.0; NaN last
            dts = [geometry(det_boxes[d], W, H) for d in di]
            gts = [geometry(true_boxes[g], W, H) for g in gi]
            crowd = [bool(true_crowd[g] != 0) for g in gi]
            table = [[iou(d, g, crowd[j]) for j, g in enumerate(gts)] for d in dts]
            for a in range(n_a):
                dtm, dt_ig, gt_ig = evaluate_img(dts, gts, crowd, iou_thrs, area_rngs[a], table)
                evals[(c, a, i)] = {"scores": np.asarray(det_scores[di], np.float64), "dtm": dtm, "dt_ig": dt_ig, "gt_ig": gt_ig}
                for ti in range(n_t):
                    for k, d in enumerate(di):
                        det_match[a, ti, d] = gi[dtm[ti, k]] if dtm[ti, k] >= 0 else -1
                        det_ignore[a, ti, d] = dt_ig[ti, k]

    # ---- accumulate ------------------------------------------------------------------------------------------------------
    precision = -np.ones((n_t, n_r, K, n_a, n_m))
    recall = -np.ones((n_t, K, n_a, n_m))
    for k in range(K):
        for a in range(n_a):
            E = [evals[(k + 1, a, i)] for i in range(n_img) if (k + 1, a, i) in evals]
            if not E:
                continue
            for m, cap in enumerate(max_dets):
                scores = np.concatenate([e["scores"][:cap] for e in E])
                order = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, :cap] for e in E], axis=1)[:, order]
                dt_ig = np.concatenate([e["dt_ig"][:, :cap] for e in E], axis=1)[:, order]
                npig = int(np.count_nonzero(~np.concatenate([e["gt_ig"] for e in E])))
                if npig == 0:
                    continue
                tps = np.logical_and(dtm >= 0, ~dt_ig)
                fps = np.logical_and(dtm < 0, ~dt_ig)
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
                for ti in range(n_t):
                    tp, fp = tp_sum[ti], fp_sum[ti]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + EPS)
                    recall[ti, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for j in range(nd - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(inds):
                        precision[ti, ri, k, a, m] = pr[pi] if pi < nd else 0.0

    # ---- summarize -----------------------------------------------------------------------------------------------------
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    stats = np.zeros(len(stat_desc))
    for si, (is_recall, ti, a, m) in enumerate(stat_desc):
        s = recall[:, :, a, m] if is_recall else precision[:, :, :, a, m]
        stats[si] = mean(s if ti < 0 else s[ti:ti + 1])
    per_class_ap = np.array([mean(precision[:, :, k, 0, n_m - 1]) for k in range(K)])
    return {"precision": precision, "recall": recall, "stats": stats, "per_class_ap": per_class_ap, "det_match": det_match,
            "det_ignore": det_ignore}
