"""numpy fp64 restatement of the random-perspective stage (include/mnyolo.h: mny_aug_warp_batch; augment.RandomPerspective): the
per-pixel gather with both filters, the forward matrix and the box maths.  Each numpy ufunc is one rounded fp64 operation, so nothing
is contracted.  tests/test_warp_ref_cpu.py pins the pixels to Pillow's Image.transform(PERSPECTIVE) byte for byte; the GPU tests
compare the kernel with this file and do not import PIL."""
import math

import numpy as np

FILL = (127, 127, 127)


def source_coords(c, h, w):
    """-> (xin [h,w], yin [h,w], ok [h,w]): the source coordinate of every output pixel centre; ok is False where den <= 0 or a
    coordinate is not finite (the fill)."""
    c = [float(v) for v in c]
    xi = (np.arange(w, dtype=np.float64) + 0.5)[None, :]
    yi = (np.arange(h, dtype=np.float64) + 0.5)[:, None]
    xin = c[0] * xi + c[1] * yi + c[2]
    yin = c[3] * xi + c[4] * yi + c[5]
    ok = np.ones((h, w), bool)
    if c[6] != 0.0 or c[7] != 0.0:
        den = c[6] * xi + c[7] * yi + 1.0
        ok = den > 0.0
        with np.errstate(all="ignore"):
            xin, yin = xin / den, yin / den
    ok = ok & np.isfinite(xin) & np.isfinite(yin)
    return xin, yin, ok


def corner_den(c, h, w):
    """den at the four output corners; den is linear, so its sign there covers every pixel."""
    return [c[6] * x + c[7] * y + 1.0 for x, y in ((0, 0), (w, 0), (0, h), (w, h))]


def warp_rgb(img, c, fill=FILL):
    """uint8 [h,w,3] -> uint8 [h,w,3], BILINEAR (Pillow bilinear_filter32RGB)."""
    h, w = img.shape[:2]
    xin, yin, ok = source_coords(c, h, w)
    with np.errstate(invalid="ignore"):
        ok = ok & ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))
    xs, ys = np.where(ok, xin, 0.5) - 0.5, np.where(ok, yin, 0.5) - 0.5
    fx, fy = np.floor(xs), np.floor(ys)
    X, Y = fx.astype(np.int64), fy.astype(np.int64)
    dx, dy = (xs - fx)[..., None], (ys - fy)[..., None]
    x0, x1, y0 = np.clip(X, 0, w - 1), np.clip(X + 1, 0, w - 1), np.clip(Y, 0, h - 1)
    p = img.astype(np.float64)
    v1 = p[y0, x0] + (p[y0, x1] - p[y0, x0]) * dx
    two = (Y + 1 >= 0) & (Y + 1 < h)
    y1 = np.where(two, Y + 1, y0)
    v2 = np.where(two[..., None], p[y1, x0] + (p[y1, x1] - p[y1, x0]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    out = v.astype(np.int64).astype(np.uint8)                     # (UINT8)v, v in 0..255
    out[~ok] = np.asarray(fill, np.uint8)
    return out


def warp_id(seg, c, fill=0):
    """uint8 [h,w] -> uint8 [h,w], NEAREST (Pillow nearest_filter8)."""
    h, w = seg.shape
    xin, yin, ok = source_coords(c, h, w)
    with np.errstate(invalid="ignore"):
        ok = ok & ~((xin < 0.0) | (yin < 0.0) | (xin >= w) | (yin >= h))
    xi, yi = np.where(ok, xin, 0.0).astype(np.int64), np.where(ok, yin, 0.0).astype(np.int64)
    out = seg[yi, xi].copy()
    out[~ok] = fill
    return out


IDENTITY_C = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def matrix(h, w, degrees=0.0, scale=1.0, shear_x=0.0, shear_y=0.0, tx=0.5, ty=0.5, px=0.0, py=0.0):
    """M = T . S . R . P . C, forward (source -> output)."""
    a = math.radians(degrees)
    C = np.array([[1, 0, -w / 2], [0, 1, -h / 2], [0, 0, 1]], np.float64)
    P = np.array([[1, 0, 0], [0, 1, 0], [px, py, 1]], np.float64)
    R = np.array([[scale * math.cos(a), scale * math.sin(a), 0], [-scale * math.sin(a), scale * math.cos(a), 0], [0, 0, 1]], np.float64)
    S = np.array([[1, math.tan(math.radians(shear_x)), 0], [math.tan(math.radians(shear_y)), 1, 0], [0, 0, 1]], np.float64)
    T = np.array([[1, 0, tx * w], [0, 1, ty * h], [0, 0, 1]], np.float64)
    return T @ S @ R @ P @ C


def coeffs(M):
    """forward 3x3 -> c[0..7] of the inverse map, the ninth normalised to 1."""
    M = np.asarray(M, np.float64)
    inv = np.linalg.inv(M)
    c = (inv / inv[2, 2]).reshape(9)[:8]
    if M[2, 0] == 0 and M[2, 1] == 0:
        c[6] = c[7] = 0.0                                         # the inverse of an affine map is affine, whatever the solver's rounding
    return c


def forward(M, x, y):
    """points through the forward matrix, with the perspective divide."""
    d = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    return (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / d, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / d


def box_corners(target, h, w):
    t = np.asarray(target, np.float64).reshape(-1, 5)
    return (t[:, 1] - t[:, 3] / 2) * w, (t[:, 2] - t[:, 4] / 2) * h, (t[:, 1] + t[:, 3] / 2) * w, (t[:, 2] + t[:, 4] / 2) * h


def boxes(target, M, h, w):
    """[n,5] cls,cx,cy,w,h normalised -> float32 [k,5] after the map: min / max of the four mapped corners, clipped to the image, kept
    iff w' > 2, h' > 2, aspect < 100 and area' / (area * |det M[:2,:2]| + 1e-16) > 0.1."""
    t = np.asarray(target, np.float64).reshape(-1, 5)
    M = np.asarray(M, np.float64)
    x1, y1, x2, y2 = box_corners(t, h, w)
    rows = []
    for i in range(len(t)):
        pts = [forward(M, x, y) for x, y in ((x1[i], y1[i]), (x2[i], y2[i]), (x1[i], y2[i]), (x2[i], y1[i]))]
        nx1, nx2 = min(max(min(p[0] for p in pts), 0.0), w), min(max(max(p[0] for p in pts), 0.0), w)
        ny1, ny2 = min(max(min(p[1] for p in pts), 0.0), h), min(max(max(p[1] for p in pts), 0.0), h)
        nw, nh = nx2 - nx1, ny2 - ny1
        if not (nw > 2 and nh > 2):
            continue
        area = (x2[i] - x1[i]) * (y2[i] - y1[i])
        det = abs(M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
        if max(nw / nh, nh / nw) < 100 and nw * nh / (area * det + 1e-16) > 0.1:
            rows.append((t[i, 0], (nx1 + nx2) / 2 / w, (ny1 + ny2) / 2 / h, nw / w, nh / h))
    return np.array(rows, np.float64).reshape(-1, 5).astype(np.float32)


def image(h, w, seed, channels=3):
    """A random uint8 image with structure at every scale: noise over a gradient, so that a one-pixel slip shows."""
    r = np.random.RandomState(seed)
    shape = (h, w, 3) if channels == 3 else (h, w)
    if channels == 1:
        return r.randint(0, 5, size=shape).astype(np.uint8)
    return r.randint(0, 256, size=shape).astype(np.uint8)


def random_coeffs(r, h, w, perspective):
    """Random forward matrix about the image centre -> its c; with `perspective` the division path.  Only cases whose den is
    positive at the four output corners are returned (the precondition under which Pillow is defined)."""
    while True:
        M = matrix(h, w, r.uniform(-180, 180), r.uniform(0.4, 2.2), r.uniform(-20, 20), r.uniform(-20, 20), r.uniform(0.3, 0.7), r.uniform(0.3, 0.7),
                   r.uniform(-1, 1) * 0.5 / max(w, 1) if perspective else 0.0, r.uniform(-1, 1) * 0.5 / max(h, 1) if perspective else 0.0)
        c = coeffs(M)
        if np.isfinite(c).all() and min(corner_den(c, h, w)) > 0:
            return M, c
