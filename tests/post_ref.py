"""numpy restatement of the post-processing stages of include/mnyolo.h (mny_yolo_decode_ex, mny_nms_agnostic, mny_det_topk): every fp32
operation one np.float32 operation in the header's order, the sigmoid as 1 / (1 + exp(-x)) in float32, the NMS and the top-k as the
sequential loops of the specification."""
import numpy as np

from tta_ref import iou32_many

f32, f64 = np.float32, np.float64


def sigmoid(x):
    x = np.asarray(x, dtype=f32)
    with np.errstate(over="ignore"):
        return f32(1.0) / (f32(1.0) + np.exp(-x))


def class_mask_words(classes, C):
    words = np.zeros((C + 31) // 32, dtype=np.uint32)
    for c in classes:
        words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return words


def _allowed(words, C):
    if words is None:
        return np.ones(C, dtype=bool)
    return np.array([(int(words[c >> 5]) >> (c & 31)) & 1 for c in range(C)], dtype=bool)


def decode_cells(head, anchors_all, mask):
    """head [N,g,g,A*(5+C)] float32 (channels last) -> box [N,A,g,g,4], conf [N,A,g,g], cls [N,A,g,g,C], all float32: cells in the
    (anchor, gy, gx) order of the specification"""
    head = np.asarray(head, dtype=f32)
    N, g = head.shape[0], head.shape[1]
    A = len(mask)
    T = head.shape[3] // A
    p = head.reshape(N, g, g, A, T).transpose(0, 3, 1, 2, 4)                       # [N,A,gy,gx,T]
    anchors = np.asarray(anchors_all, dtype=f32)[np.asarray(mask)]
    gx = np.arange(g, dtype=f32).reshape(1, 1, 1, g)
    gy = np.arange(g, dtype=f32).reshape(1, 1, g, 1)
    gf = f32(g)
    aw, ah = anchors[:, 0].reshape(1, A, 1, 1), anchors[:, 1].reshape(1, A, 1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        cx = (sigmoid(p[..., 0]) + gx) / gf
        cy = (sigmoid(p[..., 1]) + gy) / gf
        w = np.exp(p[..., 2]) * aw
        h = np.exp(p[..., 3]) * ah
        x1 = cx - w / f32(2)
        y1 = cy - h / f32(2)
        x2 = w + x1
        y2 = h + y1
    box = np.stack((x1, y1, x2, y2), -1)
    assert box.dtype == f32
    return box, sigmoid(p[..., 4]), sigmoid(p[..., 5:])


def decode_candidates(head, anchors_all, mask, obj_thr, score_thr=-1.0, multi_label=False, class_mask=None):
    """-> per image the candidate rows [t,7] float32 in emission order (no capacity applied)"""
    box, conf, cls = decode_cells(head, anchors_all, mask)
    N, C = box.shape[0], cls.shape[-1]
    allowed = _allowed(class_mask, C)
    obj_thr, score_thr = f32(obj_thr), f32(score_thr)
    out = []
    for n in range(N):
        b, cf, cl = box[n].reshape(-1, 4), conf[n].reshape(-1), cls[n].reshape(-1, C)
        with np.errstate(invalid="ignore"):
            score = cf[:, None] * cl                                               # one fp32 product
            ok = (cf > obj_thr)[:, None] & allowed[None, :]
            if not score_thr < 0:
                ok = ok & (score > score_thr)
        if not multi_label:
            best = np.zeros(len(cf), dtype=np.int64)                               # first maximum; a NaN never wins
            bv = np.full(len(cf), -np.inf, dtype=f32)
            for c in range(C):
                with np.errstate(invalid="ignore"):
                    win = cl[:, c] > bv
                best[win], bv[win] = c, cl[win, c]
            sel = np.zeros_like(ok)
            sel[np.arange(len(cf)), best] = True
            ok = ok & sel
            cl = cl.copy()
            cl[np.arange(len(cf)), best] = bv                                      # (-inf where every class score is NaN)
        cell, c = np.nonzero(ok)                                                   # row-major: cells, then classes ascending
        out.append(np.concatenate((b[cell], cf[cell, None], cl[cell, c][:, None], c.astype(f32)[:, None]), 1).astype(f32))
    return out


def margins(head, anchors_all, mask, obj_thr, score_thr=-1.0):
    """smallest |conf - obj_thr| and |score_c - score_thr| over every cell and class of the case (inf when the test is off)"""
    _, conf, cls = decode_cells(head, anchors_all, mask)
    m_obj = float(np.abs(conf.astype(f64) - f64(f32(obj_thr))).min())
    m_score = np.inf
    if not score_thr < 0:
        with np.errstate(invalid="ignore"):
            score = conf[..., None] * cls
        m_score = float(np.abs(score.astype(f64) - f64(f32(score_thr))).min())
    return m_obj, m_score


def decode_ex(cands, rows, row_stride, base_counts=None):
    """Apply the capacity rule: cands = decode_candidates(...), rows [N,row_stride,7] written in place -> (counts, dropped) int32 [N]"""
    N = len(cands)
    counts, dropped = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for n, r in enumerate(cands):
        base = int(base_counts[n]) if base_counts is not None else 0
        room = row_stride - base if 0 <= base <= row_stride else 0
        w = min(len(r), room)
        if w:
            rows[n, base:base + w] = r[:w]
        counts[n], dropped[n] = base + w, len(r) - w
    return counts, dropped


def desc_key(score):
    """the NMS's sort key of a float32 score: larger score -> smaller key"""
    u = np.asarray(score, dtype=f32).reshape(-1).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~u


def _scores(rows):
    with np.errstate(invalid="ignore", over="ignore"):
        return (rows[:, 5] * rows[:, 4]).astype(f32)


def nms_agnostic(rows, thr):
    """rows [n,7] float32 (one segment) -> kept row indices, descending score (ties by original order): greedy, the kept box first in
    the IoU, the float IoU promoted to double before the strict compare"""
    rows = np.asarray(rows, dtype=f32).reshape(-1, 7)
    n = len(rows)
    order = np.lexsort((np.arange(n), desc_key(_scores(rows))))
    dead = np.zeros(n, dtype=bool)
    kept = []
    for j in order:
        if dead[j]:
            continue
        kept.append(int(j))
        dead |= iou32_many(rows[j], rows).astype(f64) > f64(thr)                  # (also marks j itself or not: it is kept already)
    return np.array(kept, dtype=np.int64)


def det_topk(rows, kept_idx, max_det):
    """rows [.,7]; kept_idx: one segment's kept row indices in NMS output order -> the indices after the cap"""
    kept_idx = np.asarray(kept_idx, dtype=np.int64)
    assert max_det >= 1
    key = desc_key(_scores(np.asarray(rows, dtype=f32).reshape(-1, 7)[kept_idx]))
    order = np.lexsort((np.arange(len(kept_idx)), key))
    return kept_idx[order[:max_det]]
