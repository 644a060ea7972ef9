"""CPU: tests/warp_ref.py, the numpy restatement the random-perspective kernel is held to, pinned against Pillow's
Image.transform(PERSPECTIVE) byte for byte, against answers worked by hand, and its box maths against the pixels it moves."""
import math

import numpy as np
import pytest

import warp_ref as W


# ---- against Pillow ------------------------------------------------------------------------------------------------
def pil_cases():
    """(h, w, perspective, seed): sizes from 1x1 up, affine and projective."""
    r = np.random.RandomState(11)
    cases = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5)] + [(int(r.randint(1, 41)), int(r.randint(1, 41))) for _ in range(55)]
    return [(h, w, bool(k % 2), 100 + k) for k, (h, w) in enumerate(cases)] + [(h, w, not bool(k % 2), 500 + k) for k, (h, w) in enumerate(cases)]


def pil_transform(img, c, resample, fill):
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(img)
    return np.asarray(im.transform((img.shape[1], img.shape[0]), Image.Transform.PERSPECTIVE, tuple(float(v) for v in c), resample, fillcolor=fill))


def test_pixels_equal_pillow_on_random_cases():
    Image = pytest.importorskip("PIL.Image")
    n_div = 0
    for h, w, persp, seed in pil_cases():
        r = np.random.RandomState(seed)
        _, c = W.random_coeffs(r, h, w, persp)
        assert min(W.corner_den(c, h, w)) > 0
        n_div += int(c[6] != 0 or c[7] != 0)
        rgb, seg = W.image(h, w, seed), W.image(h, w, seed + 1, channels=1)
        assert np.array_equal(W.warp_rgb(rgb, c), pil_transform(rgb, c, Image.Resampling.BILINEAR, W.FILL)), (h, w, persp, seed)
        assert np.array_equal(W.warp_id(seg, c), pil_transform(seg, c, Image.Resampling.NEAREST, 0)), (h, w, persp, seed)
    assert n_div == len(pil_cases()) // 2


@pytest.mark.parametrize("persp", [False, True])
def test_pixels_equal_pillow_on_a_voc_sized_image(persp):
    Image = pytest.importorskip("PIL.Image")
    h, w = 375, 500
    c = W.coeffs(W.matrix(h, w, 33.0, 0.8, 5.0, -7.0, 0.55, 0.45, 3e-4 if persp else 0.0, -2e-4 if persp else 0.0))
    assert min(W.corner_den(c, h, w)) > 0 and bool(c[6] != 0 or c[7] != 0) == persp
    rgb, seg = W.image(h, w, 1), W.image(h, w, 2, channels=1)
    got = W.warp_rgb(rgb, c)
    assert np.array_equal(got, pil_transform(rgb, c, Image.Resampling.BILINEAR, W.FILL))
    assert np.array_equal(W.warp_id(seg, c), pil_transform(seg, c, Image.Resampling.NEAREST, 0))
    inside = np.any(got != 127, axis=2).mean()
    assert 0.2 < inside < 1.0                                      # the case shows both the image and the fill


# ---- hand-worked answers -------------------------------------------------------------------------------------------
def test_identity_coefficients():
    rgb, seg = W.image(9, 13, 0), W.image(9, 13, 1, channels=1)
    assert np.array_equal(W.warp_rgb(rgb, W.IDENTITY_C), rgb)
    assert np.array_equal(W.warp_id(seg, W.IDENTITY_C), seg)


def test_integer_translation():
    """out(x, y) = in(x + 3, y - 2): c2 = 3, c5 = -2."""
    rgb, seg = W.image(8, 10, 2), W.image(8, 10, 3, channels=1)
    c = (1, 0, 3, 0, 1, -2, 0, 0)
    want = np.full_like(rgb, 127)
    want[2:, :7] = rgb[:6, 3:]
    assert np.array_equal(W.warp_rgb(rgb, c), want)
    want = np.zeros_like(seg)
    want[2:, :7] = seg[:6, 3:]
    assert np.array_equal(W.warp_id(seg, c), want)


def test_half_pixel_translation_truncates():
    """xin = xi + 0.5: dx = 0.5 between pixels x and x + 1, (uint8) truncates the .5; the last pixel's xin is exactly w: the fill."""
    row = np.array([[10, 13, 20, 21, 255, 0]], np.uint8)
    rgb = np.repeat(row[..., None], 3, axis=2)
    got = W.warp_rgb(rgb, (1, 0, 0.5, 0, 1, 0, 0, 0))
    assert got[0, :, 0].tolist() == [11, 16, 20, 138, 127, 127]   # 11.5, 16.5, 20.5, 138, 127.5, fill
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    got = W.warp_rgb(rgb, (1, 0, -0.5, 0, 1, 0, 0, 0), fill=(9, 9, 9))
    assert got[0, :, 0].tolist() == [10, 11, 16, 20, 138, 127]    # xin = 0 exactly: X = -1, x0 = x1 = 0, the pixel itself
    col = rgb.transpose(1, 0, 2).copy()
    got = W.warp_rgb(col, (1, 0, 0, 0, 1, 0.5, 0, 0))
    assert got[:, 0, 0].tolist() == [11, 16, 20, 138, 127, 127]
    got = W.warp_rgb(col, (1, 0, 0, 0, 1, 0.25, 0, 0))
    assert got[:, 0, 0].tolist() == [10, 14, 20, 79, 191, 0]      # dy = 0.25; on the last row Y + 1 == h: v2 = v1


def test_quarter_turn_of_a_square_is_a_permutation():
    """Source (xin, yin) = (yi, n - xi): every centre lands on a centre, dx = dy = 0."""
    n = 7
    rgb, seg = W.image(n, n, 4), W.image(n, n, 5, channels=1)
    c = (0, 1, 0, -1, 0, n, 0, 0)
    want = np.empty_like(rgb)
    for y in range(n):
        for x in range(n):
            want[y, x] = rgb[n - 1 - x, y]
    assert np.array_equal(W.warp_rgb(rgb, c), want)
    assert np.array_equal(W.warp_id(seg, c), want_id(seg, n))
    # and the same through matrix(): a rotation by 90 degrees about the centre
    M = W.matrix(n, n, degrees=90.0)
    cm = np.round(W.coeffs(M), 9) + 0.0
    assert sorted(np.abs(cm[[1, 3]]).tolist()) == [1.0, 1.0] and cm[0] == 0 and cm[4] == 0
    out = W.warp_rgb(rgb, cm)
    assert sorted(map(tuple, out.reshape(-1, 3).tolist())) == sorted(map(tuple, rgb.reshape(-1, 3).tolist()))


def want_id(seg, n):
    want = np.empty_like(seg)
    for y in range(n):
        for x in range(n):
            want[y, x] = seg[n - 1 - x, y]
    return want


def test_source_coordinate_exactly_zero_and_exactly_w():
    """xin = xi - 0.5 puts pixel 0 at exactly 0.0 (inside, blends with the clamped neighbour: itself); xin = xi + w - 0.5 puts it at
    exactly w (outside)."""
    rgb = W.image(1, 4, 6)
    seg = W.image(1, 4, 7, channels=1) + 1
    got = W.warp_rgb(rgb, (1, 0, -0.5, 0, 1, 0, 0, 0))
    assert np.array_equal(got[0, 0], rgb[0, 0])                    # xs = -0.5: X = -1, x0 = x1 = 0
    assert np.array_equal(W.warp_id(seg, (1, 0, -0.5, 0, 1, 0, 0, 0)), seg)         # xin = 0, 1, 2, 3: (int) of each is its pixel
    got = W.warp_rgb(rgb, (1, 0, 3.5, 0, 1, 0, 0, 0))
    assert np.all(got == 127)                                      # xin = 4.0 = w at pixel 0
    assert not W.warp_id(seg, (1, 0, 3.5, 0, 1, 0, 0, 0)).any()
    got = W.warp_id(seg, (1, 0, 3.5 - 2 ** -50, 0, 1, 0, 0, 0))    # just below w: the last pixel
    assert got[0, 0] == seg[0, 3] and not got[0, 1:].any()


def test_non_positive_denominator_is_the_fill():
    rgb, seg = W.image(4, 6, 8), W.image(4, 6, 9, channels=1) + 1
    c = (1, 0, 0, 0, 1, 0, -0.5, 0)                                # den = 1 - xi / 2: 0.75, 0.25, then negative; exactly 0 nowhere
    got = W.warp_rgb(rgb, c)
    assert np.all(got[:, 2:] == 127) and np.any(got[:, :2] != 127)
    assert not W.warp_id(seg, c)[:, 2:].any()
    c = (1, 0, 0, 0, 1, 0, -2.0, 0)                                # den = 1 - 2 xi: 0 at xi = 0.5 exactly
    assert np.all(W.warp_rgb(rgb, c) == 127) and not W.warp_id(seg, c).any()
    c = (1, 0, 0, 0, 1, 0, np.nan, 0)
    assert np.all(W.warp_rgb(rgb, c) == 127)


# ---- boxes -----------------------------------------------------------------------------------------------------------
T = np.array([[3, 0.5, 0.5, 0.2, 0.4], [1, 0.25, 0.3, 0.1, 0.2]], np.float32)


def test_boxes_identity():
    assert np.array_equal(W.boxes(T, np.eye(3), 100, 200), T)


def test_boxes_quarter_turn():
    """90 degrees about the centre of a square image: (x, y) -> (y, n - x) up to the sign convention; a centred box swaps its sides."""
    n = 100
    out = W.boxes(T[:1], W.matrix(n, n, degrees=90.0), n, n)
    assert np.allclose(out, [[3, 0.5, 0.5, 0.4, 0.2]], atol=1e-6)
    out = W.boxes(T[1:], W.matrix(n, n, degrees=90.0), n, n)
    assert out.shape == (1, 5) and np.allclose(out[0, 3:], [0.2, 0.1], atol=1e-6)
    x, y = W.forward(W.matrix(n, n, degrees=90.0), 25.0, 30.0)
    assert np.allclose(out[0, 1:3], [x / n, y / n], atol=1e-6)


def test_boxes_translation_clips_then_drops():
    h, w = 100, 200                                                # box 0: x 80..120, y 30..70
    M = W.matrix(h, w, tx=0.5 + 90 / w)                            # + 90 px: x 170..210 -> clipped to 170..200
    out = W.boxes(T[:1], M, h, w)
    assert np.allclose(out, [[3, 185 / w, 0.5, 30 / w, 0.4]], atol=1e-6)
    M = W.matrix(h, w, tx=0.5 + 117 / w)                           # x 197..237 -> 3 px left: under 0.1 of the area
    assert W.boxes(T[:1], M, h, w).shape == (0, 5)
    M = W.matrix(h, w, tx=0.5 + 130 / w)                           # wholly out
    assert W.boxes(T[:1], M, h, w).shape == (0, 5)
    assert W.boxes(np.zeros((0, 5), np.float32), M, h, w).shape == (0, 5)


def test_boxes_scale_half_area_and_two_pixel_rules():
    h, w = 100, 100
    M = W.matrix(h, w, scale=0.5)
    big = np.array([[0, 0.5, 0.5, 0.4, 0.4]], np.float32)
    out = W.boxes(big, M, h, w)
    assert np.allclose(out, [[0, 0.5, 0.5, 0.2, 0.2]], atol=1e-6)  # area ratio against area * det = 1: kept
    small = np.array([[0, 0.5, 0.5, 0.04, 0.4], [0, 0.5, 0.5, 0.0402, 0.4]], np.float32)
    out = W.boxes(small, M, h, w)                                  # 4 px -> 2 px is not > 2 px; 4.02 px -> 2.01 px is
    assert out.shape == (1, 5) and abs(out[0, 3] - 0.0201) < 1e-6
    thin = np.array([[0, 0.5, 0.5, 0.9, 0.0085]], np.float32)      # 45 px x 0.425 px after the map: 2 px rule
    assert W.boxes(thin, M, h, w).shape == (0, 5)
    long_ = np.array([[0, 0.5, 0.5, 0.9, 0.0099]], np.float32)
    assert W.boxes(long_, np.diag([1.0, 1.0, 1.0]), 1000, 1000).shape == (1, 5)         # 900 x 9.9 px: aspect 91
    assert W.boxes(long_, np.diag([1.0, 0.5, 1.0]), 1000, 1000).shape == (0, 5)         # 900 x 4.95 px: aspect 182


def test_matrix_and_coefficients_agree_with_the_pixels():
    """Warp a black image holding a filled rectangle, fill 0: every non-zero pixel centre lies inside the unclipped transformed box
    grown by 1 px (bilinear support is one pixel; a projective map with positive denominator keeps the rectangle's image inside the
    bounding box of its corners)."""
    r = np.random.RandomState(17)
    seen = 0
    for k in range(40):
        h, w = int(r.randint(20, 60)), int(r.randint(20, 60))
        persp = bool(k % 2)
        M = W.matrix(h, w, r.uniform(-180, 180), r.uniform(0.5, 1.5), r.uniform(-10, 10), r.uniform(-10, 10), r.uniform(0.4, 0.6), r.uniform(0.4, 0.6),
                     r.uniform(-1, 1) * 0.3 / w if persp else 0.0, r.uniform(-1, 1) * 0.3 / h if persp else 0.0)
        assert min(M[2, 0] * x + M[2, 1] * y + M[2, 2] for x, y in ((0, 0), (w, 0), (0, h), (w, h))) > 0
        c = W.coeffs(M)
        x1, y1 = int(r.randint(0, w - 8)), int(r.randint(0, h - 8))
        x2, y2 = int(r.randint(x1 + 4, w)), int(r.randint(y1 + 4, h))
        img = np.zeros((h, w, 3), np.uint8)
        img[y1:y2, x1:x2] = 255
        out = W.warp_rgb(img, c, fill=(0, 0, 0))
        ys, xs = np.nonzero(out.any(axis=2))
        if len(xs) == 0:
            continue
        seen += 1
        pts = [W.forward(M, float(x), float(y)) for x, y in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
        bx1, bx2 = min(p[0] for p in pts) - 1, max(p[0] for p in pts) + 1
        by1, by2 = min(p[1] for p in pts) - 1, max(p[1] for p in pts) + 1
        assert bx1 <= xs.min() + 0.5 and xs.max() + 0.5 <= bx2 and by1 <= ys.min() + 0.5 and ys.max() + 0.5 <= by2, (k, h, w)
        # and boxes() reports that box, clipped
        tgt = np.array([[0, (x1 + x2) / 2 / w, (y1 + y2) / 2 / h, (x2 - x1) / w, (y2 - y1) / h]], np.float64)
        b = W.boxes(tgt, M, h, w)
        if len(b):
            assert abs((b[0, 1] - b[0, 3] / 2) * w - min(max(bx1 + 1, 0), w)) < 1e-3 and abs((b[0, 2] + b[0, 4] / 2) * h - min(max(by2 - 1, 0), h)) < 1e-3
    assert seen >= 30
