"""numpy restatement of the three test-time-augmentation stages of include/mnyolo.h (mny_tta_view, mny_det_append, mny_nms_merge):
fp32 operations in np.float32, the fp64 parts in np.float64, the merge as the sequential loop of the specification."""
import numpy as np

f32, f64 = np.float32, np.float64


def _axis(Ss, Sd):
    """source coordinates of one axis: (i0, i1, l, 1 - l) per output index, fp64"""
    r = f64(Ss) / f64(Sd)
    s = np.maximum((np.arange(Sd, dtype=f64) + f64(0.5)) * r - f64(0.5), f64(0.0))
    i0 = np.minimum(s.astype(np.int64), Ss - 1)
    i1 = np.minimum(i0 + 1, Ss - 1)
    l = s - i0.astype(f64)
    return i0, i1, l, f64(1.0) - l


def _mix(w0, p, w1, q):
    """w0 * p + w1 * q without the term whose weight is exactly 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(w1 == 0.0, w0 * p, np.where(w0 == 0.0, w1 * q, w0 * p + w1 * q))


def tta_view(src, Hd, Wd, flip):
    """src [N,C,Hs,Ws] float32 -> [N,C,Hd,Wd] float32"""
    src = np.asarray(src, dtype=f32)
    N, C, Hs, Ws = src.shape
    if flip:
        src = src[:, :, :, ::-1]                                   # mirror first: column c is read from Ws - 1 - c
    s = src.astype(f64)
    y0, y1, ly, wy0 = _axis(Hs, Hd)
    x0, x1, lx, wx0 = _axis(Ws, Wd)
    ly, wy0 = ly[:, None], wy0[:, None]
    a, b = s[:, :, y0][:, :, :, x0], s[:, :, y0][:, :, :, x1]
    c, d = s[:, :, y1][:, :, :, x0], s[:, :, y1][:, :, :, x1]
    top = _mix(wx0, a, lx, b)
    bot = _mix(wx0, c, lx, d)
    with np.errstate(over="ignore"):
        return _mix(wy0, top, ly, bot).astype(f32)


def det_append(src_rows, src_counts, flip, dst_rows, counts):
    """src_rows [N,src_stride,7], dst_rows [N,dst_stride,7] (written in place), counts [N] (updated in place)"""
    N, src_stride, _ = src_rows.shape
    dst_stride = dst_rows.shape[1]
    for n in range(N):
        base = int(counts[n])
        if base < 0 or base > dst_stride:
            continue
        m = max(0, min(int(src_counts[n]), src_stride, dst_stride - base))
        r = np.array(src_rows[n, :m], dtype=f32)
        if flip:
            x1, x2 = r[:, 0].copy(), r[:, 2].copy()
            r[:, 0] = f32(1.0) - x2
            r[:, 2] = f32(1.0) - x1
        dst_rows[n, base:base + m] = r
        counts[n] = base + m
    return dst_rows, counts


def iou32(a, b):
    """the NMS kernel's fp32 IoU of boxes a (the kept one) and b"""
    return iou32_many(a, np.asarray(b, dtype=f32).reshape(1, -1))[0]


def iou32_many(a, B):
    """the NMS kernel's fp32 IoU of box a (the kept one) with every row of B [n,>=4]: float32 [n], every operation one fp32 op"""
    a, B = np.asarray(a, dtype=f32), np.asarray(B, dtype=f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ia = (a[2] - a[0]) * (a[3] - a[1])
        ib = (B[:, 2] - B[:, 0]) * (B[:, 3] - B[:, 1])
        xx1 = np.where(a[0] > B[:, 0], a[0], B[:, 0])
        yy1 = np.where(a[1] > B[:, 1], a[1], B[:, 1])
        xx2 = np.where(a[2] < B[:, 2], a[2], B[:, 2])
        yy2 = np.where(a[3] < B[:, 3], a[3], B[:, 3])
        w = xx2 - xx1
        h = yy2 - yy1
        w = np.where(w > 0, w, f32(0.0))
        h = np.where(h > 0, h, f32(0.0))
        inter = w * h
        out = inter / ((ia + ib) - inter)
    assert out.dtype == f32
    return out


def merge_members(rows, kept, thr):
    """indices (ascending) of the members of kept row `kept` among one segment's rows [n,7]"""
    rows = np.asarray(rows, dtype=f32)
    over = iou32_many(rows[kept], rows).astype(f64) > f64(thr)
    over[kept] = True                                              # j == i
    ok = (rows[:, 6] == rows[kept, 6]) & over                      # (a NaN class equals nothing, itself included: no members)
    return [int(j) for j in np.nonzero(ok)[0]]


def nms_merge(rows, kept_idx, thr):
    """rows [n,7] float32 (one segment), kept_idx: kept row indices in NMS output order -> merged kept rows [k,7] float32"""
    rows = np.asarray(rows, dtype=f32).reshape(-1, 7)
    out = rows[np.asarray(kept_idx, dtype=np.int64)].copy()
    for p, i in enumerate(kept_idx):
        i = int(i)
        sw = f64(0.0)
        sx = [f64(0.0)] * 4
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in merge_members(rows, i, thr):
                w = f64(f32(rows[j, 5] * rows[j, 4]))
                sw = sw + w
                for k in range(4):
                    sx[k] = sx[k] + w * f64(rows[j, k])
            if np.isfinite(sw) and sw > 0:
                for k in range(4):
                    out[p, k] = f32(sx[k] / sw)
    return out
