"""Restatement of the validation report of include/mnyolo.h (`mny_det_curves`, `mny_det_confusion`; csrc/detreport.hip): numpy, every
quantity in float64, every sum in the stated order, written for reading and not for speed.

Nothing here is pinned against a third-party package (none that draws such curves or matrices is installed where this project is
developed): the arithmetic below IS the specification of the device kernels, and the known answers of tests/test_report_ref_cpu.py
are what holds it in place.  The curves are exact step functions of the detection set {score >= c}; the np.interp that other
trainers apply to theirs is not reproduced.

`curves` takes the match flags of the COCO restatement: det_match [D] / det_ignore [D] are one [area, iou] slice of what
tests/coco_ref.py `evaluate` returns.  `confusion` takes the packed layout of coco_ref.evaluate and uses its geometry and IoU.
"""
import numpy as np

import coco_ref


def curves(det_labels, det_scores, det_match, det_ignore, true_labels, true_crowd, n_classes, grid=1000, smooth=101):
    """-> dict: tp, fp [K,G] int64; npos [K] int64; precision, recall, f1 [K,G]; mean_f1, smooth_f1 [G]; best (int), best_conf (float),
    at_best [K+1,3] (float64; -1 = class without positives)"""
    K, G, W = n_classes - 1, int(grid), int(smooth)
    assert 2 <= G <= 4096 and 1 <= W <= G and W % 2 == 1
    dcls, gcls = coco_ref.classes_of(det_labels, n_classes), coco_ref.classes_of(true_labels, n_classes)
    scores = np.asarray(det_scores, np.float32).astype(np.float64)
    counted = (dcls > 0) & (np.asarray(det_match) != -2) & (np.asarray(det_ignore) == 0)
    is_tp = np.asarray(det_match) >= 0
    conf = np.array([float(j) / float(G - 1) for j in range(G)], np.float64)
    tp, fp, npos = np.zeros((K, G), np.int64), np.zeros((K, G), np.int64), np.zeros(K, np.int64)
    for k in range(K):
        npos[k] = int(np.count_nonzero((gcls == k + 1) & (np.asarray(true_crowd) == 0)))
        for flag, out in ((is_tp, tp), (~is_tp, fp)):
            s = scores[counted & (dcls == k + 1) & flag]
            s = np.sort(s[~np.isnan(s)])                                  # a NaN score is >= nothing
            out[k] = len(s) - np.searchsorted(s, conf, side="left")      # how many s >= c_j, exactly
    precision, recall, f1 = -np.ones((K, G)), -np.ones((K, G)), -np.ones((K, G))
    for k in range(K):
        if npos[k] == 0:
            continue
        t, n = tp[k].astype(np.float64), (tp[k] + fp[k]).astype(np.float64)
        P = np.ones(G)
        P[n > 0] = t[n > 0] / n[n > 0]
        R = t / float(npos[k])
        precision[k], recall[k], f1[k] = P, R, ((2.0 * P) * R) / ((P + R) + 1e-16)

    def class_mean(rows):
        """fixed-order mean over the classes with positives of rows [K, ...]; -1 without any"""
        acc, cnt = np.zeros(rows.shape[1:]), 0
        for k in range(K):
            if npos[k] != 0:
                acc, cnt = acc + rows[k], cnt + 1
        return acc / float(cnt) if cnt else -np.ones(rows.shape[1:])

    mean_f1 = class_mean(f1)
    half, j = W // 2, np.arange(G)
    acc = np.zeros(G)
    for o in range(-half, half + 1):                                     # per grid point: the window in ascending order, ends clamped
        acc = acc + mean_f1[np.clip(j + o, 0, G - 1)]
    smooth_f1 = acc / float(W)
    best = int(np.argmax(smooth_f1))                                     # the first maximum
    at_best = np.zeros((K + 1, 3))
    for q, rows in enumerate((precision, recall, f1)):
        at_best[:K, q] = rows[:, best]
        at_best[K, q] = class_mean(rows[:, best:best + 1])[0]
    return {"tp": tp, "fp": fp, "npos": npos, "precision": precision, "recall": recall, "f1": f1, "mean_f1": mean_f1, "smooth_f1": smooth_f1,
            "best": best, "best_conf": float(conf[best]), "at_best": at_best}


def confusion(det_boxes, det_labels, det_scores, det_off, true_boxes, true_labels, true_crowd, true_off, n_classes, image_sizes=None,
              conf=0.25, iou_thr=0.45):
    """-> dict: matrix [K+1,K+1] int64 (row = predicted class, column = true class, K = background), det_gt [D] int32 (packed index of the
    matched ground truth, -1 unmatched, -2 not considered)"""
    K, n_img, D = n_classes - 1, len(det_off) - 1, len(det_labels)
    conf, iou_thr = float(conf), float(iou_thr)
    dcls, gcls = coco_ref.classes_of(det_labels, n_classes), coco_ref.classes_of(true_labels, n_classes)
    matrix = np.zeros((K + 1, K + 1), np.int64)
    det_gt = np.full(D, -2, np.int32)
    for i in range(n_img):
        W, H = (1.0, 1.0) if image_sizes is None else (float(image_sizes[i][0]), float(image_sizes[i][1]))
        dets = [d for d in range(int(det_off[i]), int(det_off[i + 1])) if dcls[d] > 0 and float(det_scores[d]) > conf]
        gts = [g for g in range(int(true_off[i]), int(true_off[i + 1])) if gcls[g] > 0]
        dgeo = [coco_ref.geometry(det_boxes[d], W, H) for d in dets]
        ggeo = [coco_ref.geometry(true_boxes[g], W, H) for g in gts]
        cand = []
        for a, d in enumerate(dets):
            for b, g in enumerate(gts):
                v = coco_ref.iou(dgeo[a], ggeo[b], False)
                if v > iou_thr:                                          # false for NaN
                    cand.append((-v, d, g))
        cand.sort()                                                      # largest IoU, then smaller detection, then smaller ground truth
        d_of, g_of = {d: -1 for d in dets}, {g: -1 for g in gts}
        for _, d, g in cand:
            if d_of[d] < 0 and g_of[g] < 0:
                d_of[d], g_of[g] = g, d
        for d in dets:
            det_gt[d] = d_of[d]
            if d_of[d] < 0:
                matrix[dcls[d] - 1, K] += 1
        for g in gts:
            if true_crowd[g] != 0:
                continue
            matrix[dcls[g_of[g]] - 1 if g_of[g] >= 0 else K, gcls[g] - 1] += 1
    return {"matrix": matrix, "det_gt": det_gt}
