"""Numpy restatement of the anchor-fitting arithmetic specified in include/mnyolo.h ("Anchor fitting"): fp32 operations one at a time
(numpy float32 arrays never contract), int64 fixed-point sums.  tests/test_anchor_ref_cpu.py checks it against hand-worked answers and
the oracle's loss; tests/test_gpu_anchors.py compares csrc/anchors.hip with it bit for bit."""
import numpy as np

F32 = np.float32
MIN_SIDE, MAX_SIDE = F32(2.0 ** -20), F32(65536.0)


def valid(wh):
    wh = np.asarray(wh, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return ((wh >= MIN_SIDE) & (wh <= MAX_SIDE)).all(1)          # NaN fails


def shape_iou(wh, anchors):
    """[N,2] x [k,2] -> v[N,k] fp32: inter = min(w,aw) * min(h,ah); v = inter / ((w*h + aw*ah) - inter)."""
    wh, a = np.asarray(wh, F32).reshape(-1, 2), np.asarray(anchors, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        inter = np.fmin(wh[:, None, 0], a[None, :, 0]) * np.fmin(wh[:, None, 1], a[None, :, 1])
        area = (wh[:, 0] * wh[:, 1])[:, None]
        a_area = (a[:, 0] * a[:, 1])[None, :]
        return inter / ((area + a_area) - inter)


def best(wh, anchors):
    """-> (index, value): the lowest index with the largest v (strict >, from -inf at index 0; a NaN never wins)."""
    v = shape_iou(wh, anchors)
    bi, bv = np.zeros(len(v), np.int32), np.full(len(v), -np.inf, F32)
    for j in range(v.shape[1]):
        with np.errstate(invalid="ignore"):
            up = v[:, j] > bv
        bv[up], bi[up] = v[up, j], j
    return bi, bv


def q(x):
    return np.rint(np.asarray(x, F32).astype(np.float64) * 2.0 ** 24).astype(np.int64)


def qi(v):
    return np.rint(np.asarray(v, F32).astype(np.float64) * 2.0 ** 32).astype(np.int64)


def kmeans_step(wh, centres):
    wh, c = np.asarray(wh, F32).reshape(-1, 2), np.array(centres, F32).reshape(-1, 2)
    ok = valid(wh)
    lab, _ = best(wh[ok], c)
    qw = q(wh[ok])
    for j in range(len(c)):
        mine = lab == j
        n = int(mine.sum())
        if n:
            s = qw[mine].sum(0, dtype=np.int64)
            c[j] = ((s.astype(np.float64) / np.float64(n)) * 2.0 ** -24).astype(F32)
    return c


def kmeans(wh, init, max_iter, trace=False):
    """-> dict(centres, labels, best_iou, state[, trace = the centres after every step that ran])."""
    wh = np.asarray(wh, F32).reshape(-1, 2)
    c = np.array(init, F32).reshape(-1, 2)
    steps, conv, tr = 0, 0, []
    for _ in range(max_iter):
        n = kmeans_step(wh, c)
        steps += 1
        same = n.tobytes() == c.tobytes()
        c = n
        tr.append(c.copy())
        if same:
            conv = 1
            break
    ok = valid(wh)
    lab, bv = best(wh, c)
    lab[~ok], bv[~ok] = -1, 0
    r = {"centres": c, "labels": lab, "best_iou": bv, "state": np.array([steps, conv, int((~ok).sum()), 0], np.int64)}
    if trace:
        r["trace"] = tr
    return r


def default_init(wh, k):
    """The shapes at the (2i+1)/(2k) quantiles of a stable sort of the valid boxes by fp32 area."""
    wh = np.asarray(wh, F32).reshape(-1, 2)
    ok = valid(wh)
    with np.errstate(all="ignore"):
        area = np.where(ok, wh[:, 0] * wh[:, 1], F32(np.inf)).astype(F32)
    order = np.argsort(area, kind="stable")
    m = int(ok.sum())
    idx = np.minimum(((2 * np.arange(k) + 1) * m) // (2 * k), len(wh) - 1)
    return wh[order[idx]].copy()


def fitness(wh, cand, thr):
    """cand[P,k,2] -> (FR int64 [P,2], valid count)."""
    wh, cand = np.asarray(wh, F32).reshape(-1, 2), np.asarray(cand, F32)
    ok = valid(wh)
    out = np.zeros((len(cand), 2), np.int64)
    for p in range(len(cand)):
        _, bv = best(wh[ok], cand[p])
        hit = bv > F32(thr)
        out[p] = int(qi(bv[hit]).sum(dtype=np.int64)), int(hit.sum())
    return out, int(ok.sum())


def evolve(wh, anchors, factors, thr, min_size):
    """-> (anchors, history int64 [G,2], the candidates of every generation)."""
    parent = np.array(anchors, F32).reshape(-1, 2)
    factors = np.asarray(factors, F32)
    hist, cands = np.zeros((len(factors), 2), np.int64), []
    for g in range(len(factors)):
        cand = np.fmax(parent[None] * factors[g], F32(min_size)).astype(F32)
        cand[0] = parent
        fr, _ = fitness(wh, cand, thr)
        win = int(np.argmax(fr[:, 0]))                 # the first maximum
        hist[g] = fr[win, 0], win
        parent = cand[win].copy()
        cands.append(cand)
    return parent, hist, cands


def _iou_ref(ax2, ay2, bx2, by2):
    """utils/iou.py:32-49 on [0,0,ax2,ay2] x [0,0,bx2,by2] in fp32, with fminf / fmaxf's NaN rule (csrc/iou.h iou_ref)."""
    z = F32(0)
    with np.errstate(all="ignore"):
        iw = np.fmax(np.fmin(ax2, bx2) - z, z)
        ih = np.fmax(np.fmin(ay2, by2) - z, z)
        inter = iw * ih
        aa = (ax2 - z) * (ay2 - z)
        ab = (bx2 - z) * (by2 - z)
        return inter / (aa + ab - inter)


def census(targets, anchors_all, mask, grids, iou_thresh):
    """targets[T,5] packed (label, cx, cy, w, h); anchors_all[n,2] fp32, already divided by the image size.  Follows yolo_assign_kernel
    (csrc/detect.hip).  -> dict(best[n], pos[H,A], orphans, outside[H]) int64."""
    t = np.asarray(targets, F32).reshape(-1, 5)
    a = np.asarray(anchors_all, F32).reshape(-1, 2)
    mask = np.asarray(mask, np.int64)
    H, A = mask.shape
    T = len(t)
    v = np.stack([_iou_ref(t[:, 3], t[:, 4], a[k, 0], a[k, 1]) for k in range(len(a))], 1).astype(F32) if T else np.zeros((0, len(a)), F32)
    best_n, best_v = np.zeros(T, np.int64), np.full(T, -np.inf, F32)
    for k in range(len(a)):
        with np.errstate(invalid="ignore"):
            up = (v[:, k] > best_v) | (np.isnan(v[:, k]) & ~np.isnan(best_v))
        best_v[up], best_n[up] = v[up, k], k
    pos, outside, anyhit = np.zeros((H, A), np.int64), np.zeros(H, np.int64), np.zeros(T, bool)
    for h in range(H):
        g = int(grids[h])
        gi = (t[:, 1] * F32(g)).astype(np.int32)
        gj = (t[:, 2] * F32(g)).astype(np.int32)
        inside = (gi >= 0) & (gi < g) & (gj >= 0) & (gj < g)
        outside[h] = int((~inside).sum())
        for k in range(A):
            am = int(mask[h, k])
            with np.errstate(invalid="ignore"):
                hit = inside & ((best_n == am) | (v[:, am] > F32(iou_thresh)))
            pos[h, k] = int(hit.sum())
            anyhit |= hit
    return {"best": np.bincount(best_n, minlength=len(a)).astype(np.int64), "pos": pos, "orphans": np.int64((~anyhit).sum()), "outside": outside}
