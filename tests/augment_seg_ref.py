"""TEST INFRASTRUCTURE — numpy restatement of the seg-map half of the reference's train-phase sample path, the contract
that TrainAugment(seg_classes=...) + mny_aug_seg_batch (csrc/augment.hip) reproduce.  Only tests/ may import this.

  * Geometry (utils/image_augmentation.py:14-52,114-116,157-159,301-330): the uint8 id map goes through to_tensor
    (/255), expand_od (border 0), random_crop_od (the image's window), to_pil_image (.mul(255).byte(), the identity for
    all 256 values) and flip_od.  No random draw of its own; the photometric chain does not touch it.  PINNED to the
    real reference by tests/golden/augseg_*.npz (tools/gen_golden_augment_seg.py).
  * Per-class maps (folder2lmdb.py:135-141,243-261): for c = 1..C, Image.fromarray(array == c).convert('L') (0 / 255),
    cv2.resize(..., INTER_AREA) to the S/16 grid, / 255.0.
  * The area resize restates OpenCV (modules/imgproc/src/resize.cpp: computeResizeAreaTab, ResizeArea_,
    ResizeAreaFast_) for uchar, one channel, both scales >= 1.  OpenCV itself is not available to the test suite, so
    this half is parity-UNPINNED; test_oracle_augment_seg.py bounds it against an exact fp64 area average instead.
"""
import numpy as np

F32, F64 = np.float32, np.float64
DBL_EPSILON = float(np.finfo(np.float64).eps)


# ---- geometry ---------------------------------------------------------------------------------------------------------
def geometry(seg_id, expand, crop, flip):
    """seg_id uint8 [h,w]; expand: None or (new_h, new_w, top, left); crop: None or (top, left, h, w); flip: bool."""
    a = np.asarray(seg_id)
    if expand is not None:
        nh, nw, top, left = expand
        canvas = np.zeros((nh, nw), np.uint8)                           # image_augmentation.py:36 torch.zeros
        canvas[top:top + a.shape[0], left:left + a.shape[1]] = a
        a = canvas
    if crop is not None:
        t, l, h, w = crop
        a = a[t:t + h, l:l + w]
    if flip:
        a = a[:, ::-1]
    return np.ascontiguousarray(a)


# ---- cv2.resize(..., INTER_AREA) for uchar, one channel, scale >= 1 ---------------------------------------------------
def area_scale(ssize, dsize):
    return 1.0 / (float(dsize) / ssize)


def area_is_fast(ssize, dsize):
    scale = area_scale(ssize, dsize)
    return abs(scale - int(scale)) < DBL_EPSILON


def area_tab(ssize, dsize):
    """computeResizeAreaTab: per destination index the taps [(source index, float32 weight)] in emission order."""
    scale = area_scale(ssize, dsize)
    if scale < 1.0:
        raise ValueError("INTER_AREA with scale < 1 is another OpenCV path (not restated)")
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1 = int(np.ceil(f1))
        s2 = min(int(np.floor(f2)), ssize - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            taps.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            taps.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(taps)
    return tab


def _padded(tab):
    """Tap table as arrays [dsize, kmax]; padding (index 0, weight 0) sits at the END, where `x + S*0` leaves x as is."""
    k = max(len(t) for t in tab)
    idx = np.zeros((len(tab), k), np.int64)
    wgt = np.zeros((len(tab), k), F32)
    for d, taps in enumerate(tab):
        for j, (s, a) in enumerate(taps):
            idx[d, j], wgt[d, j] = s, a
    return idx, wgt


def resize_area_u8(src, out_h, out_w):
    """uint8 [h,w] -> uint8 [out_h,out_w]; every binary-32 step is its own rounded operation (no FMA)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    h, w = src.shape
    if h < out_h or w < out_w:
        raise ValueError("INTER_AREA with scale < 1 is another OpenCV path (not restated)")
    if area_is_fast(h, out_h) and area_is_fast(w, out_w):                    # ResizeAreaFast_
        iy, ix = int(area_scale(h, out_h)), int(area_scale(w, out_w))
        isum = src[:out_h * iy, :out_w * ix].astype(np.int64).reshape(out_h, iy, out_w, ix).sum(axis=(1, 3))
        v = isum.astype(F32) * (F32(1.0) / F32(ix * iy))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    xi, xa = _padded(area_tab(w, out_w))
    yi, ya = _padded(area_tab(h, out_h))
    S = src.astype(F32)
    buf = np.zeros((h, out_w), F32)                                          # ResizeArea_: buf[dx] = 0, += S[sy][sx]*alpha in tap order
    for k in range(xi.shape[1]):
        buf = buf + S[:, xi[:, k]] * xa[None, :, k]
    total = ya[:, 0, None] * buf[yi[:, 0]]                                   # sum[dx] = beta*buf[dx] for the row's first tap ...
    for k in range(1, yi.shape[1]):
        total = total + ya[:, k, None] * buf[yi[:, k]]                       # ... and sum[dx] += beta*buf[dx] after it
    assert total.dtype == F32
    return np.clip(np.rint(total), 0, 255).astype(np.uint8)                   # saturate_cast<uchar>: nearest even


def seg_maps(new_seg_id, n_classes, grid):
    """folder2lmdb.py:137-141,244-248 for one sample: -> float32 [grid_h, grid_w, C]."""
    gh, gw = grid
    arr = np.asarray(new_seg_id)
    out = np.zeros((gh, gw, n_classes), F32)
    for c in range(1, n_classes + 1):
        binary = np.where(arr == c, 255, 0).astype(np.uint8)                 # '1' mode -> convert('L')
        out[..., c - 1] = resize_area_u8(binary, gh, gw).astype(F32) / F32(255.0)
    return out


def batch_maps(seg_ids, members, n_classes, size):
    """seg_ids: one uint8 map per single-image sample; members: their plans (augment_ref.plan_member dicts, keys expand /
    crop / flip).  -> float32 [N, size_h/16, size_w/16, C], collate_fn's fourth member."""
    grid = (int(size[0] / 16), int(size[1] / 16))
    return np.stack([seg_maps(geometry(s, m["expand"], m["crop"], m["flip"]), n_classes, grid) for s, m in zip(seg_ids, members)])


def exact_area_average(src, out_h, out_w):
    """fp64 area average over the exact source footprint of every destination pixel (an independent sanity reference)."""
    src = np.asarray(src, F64)

    def weights(ssize, dsize):
        scale = ssize / dsize
        W = np.zeros((dsize, ssize), F64)
        for d in range(dsize):
            a, b = d * scale, (d + 1) * scale
            lo = np.arange(ssize, dtype=F64)
            W[d] = np.clip(np.minimum(lo + 1, b) - np.maximum(lo, a), 0, None) / scale
        return W
    return weights(src.shape[0], out_h) @ src @ weights(src.shape[1], out_w).T
