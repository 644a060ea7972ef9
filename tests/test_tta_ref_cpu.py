"""CPU: the numpy restatement of the test-time-augmentation stages (tests/tta_ref.py) against hand-worked answers and against
torch.nn.functional.interpolate, and the argument validation of tta.TTA / tta.default_views (no GPU needed)."""
import numpy as np
import pytest
import torch

import tta_ref

f32 = np.float32


# ---- mny_tta_view ----------------------------------------------------------------------------------------------------
def test_view_2x2_to_3x3_by_hand():
    """scale 2/3: source coordinates max((i + 0.5) * 2/3 - 0.5, 0) = 0, 0.5, 1.1667 -> taps (0,1; l=0), (0,1; l=0.5), (1,1; l=0.1667): the
    last column / row interpolates a pixel with itself.  Every value below is exact in fp32."""
    src = np.array([[[[0.0, 2.0], [4.0, 6.0]]]], dtype=f32)
    want = np.array([[[[0, 1, 2], [2, 3, 4], [4, 5, 6]]]], dtype=f32)
    assert np.array_equal(tta_ref.tta_view(src, 3, 3, False), want)
    assert np.array_equal(tta_ref.tta_view(src, 3, 3, True), want[:, :, :, ::-1])


def test_view_mirror_is_an_exact_copy_and_zero_weights_are_skipped():
    src = np.array([[[[1.0, np.inf, -3.0, 0.5], [-0.25, 7.0, 1e-30, -2.0]]]], dtype=f32)
    got = tta_ref.tta_view(src, 2, 4, True)
    assert np.array_equal(got, src[:, :, :, ::-1])                # same size: l = 0 everywhere, the inf is copied and poisons nothing
    assert np.isfinite(got).sum() == 7
    assert np.array_equal(tta_ref.tta_view(src, 2, 4, False), src)


def test_view_1x1_source_is_constant():
    src = np.array([[[[-1.5]]], [[[0.75]]]], dtype=f32)
    got = tta_ref.tta_view(src, 4, 3, True)
    assert got.shape == (2, 1, 4, 3)
    assert np.array_equal(got, np.broadcast_to(src, got.shape))


def test_view_matches_torch_interpolate_on_random_sizes():
    """F.interpolate(mode="bilinear", align_corners=False) computes the same taps in fp32, so this comparison takes a tolerance — derived,
    not tuned.  Per axis torch forms scale = (float)Ss / Sd, s = scale * (i + 0.5) - 0.5 and l = s - floor(s) in fp32: three roundings (the
    quotient, the product, the difference; s - floor(s) is exact) of numbers below Ss, each at most Ss * 2^-24, so the weight differs by
    at most 3 * Ss * 2^-24 (the issue's "about size * 2^-23"; the restatement's own fp64 path adds nothing visible).  The bilinear surface is
    continuous (also across a tap change, where l wraps from 1 to 0, and at the clamped border) with slope at most R = max - min of the
    pixels per unit of either weight, so the value moves by at most 3 * (Hs + Ws) * 2^-24 * R.  On top, torch evaluates
    w00*a + w01*b + w10*c + w11*d in fp32: 4 weight products, 4 pixel products, 3 sums, and one final rounding here: 12 operations of
    relative error 2^-24 on magnitudes up to M = max |pixel|: 12 * 2^-24 * M.  Observed worst error / bound: LAB_NOTES.md."""
    rng = np.random.default_rng(5)
    pairs = [((1, 1), (4, 4)), ((1, 1), (1, 7)), ((1, 5), (3, 3)), ((2, 2), (3, 3)), ((5, 7), (3, 4)), ((64, 64), (32, 32)),
             ((64, 64), (96, 96)), ((33, 65), (32, 32)), ((32, 32), (64, 64)), ((7, 3), (7, 3))]
    while len(pairs) < 20:
        pairs.append(((int(rng.integers(1, 70)), int(rng.integers(1, 70))), (int(rng.integers(1, 100)), int(rng.integers(1, 100)))))
    worst = 0.0
    for k, ((hs, ws), (hd, wd)) in enumerate(pairs):
        src = rng.uniform(-2.0, 2.0, size=(2, 3, hs, ws)).astype(f32)
        flip = bool(k % 2)
        got = tta_ref.tta_view(src, hd, wd, flip)
        t = torch.from_numpy(src[:, :, :, ::-1].copy() if flip else src)
        want = torch.nn.functional.interpolate(t, size=(hd, wd), mode="bilinear", align_corners=False).numpy()
        R, M = float(src.max() - src.min()), float(np.abs(src).max())
        tol = 3 * (hs + ws) * 2.0 ** -24 * R + 12 * 2.0 ** -24 * M
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        worst = max(worst, err / tol)
        assert err <= tol, ((hs, ws), (hd, wd), flip, err, tol)
    print("tta_view restatement vs F.interpolate: worst error / bound = %.3f" % worst)


# ---- mny_det_append ----------------------------------------------------------------------------------------------------
def test_append_by_hand():
    src = np.arange(2 * 2 * 7, dtype=f32).reshape(2, 2, 7) / f32(64.0)
    dst = np.full((2, 3, 7), -9.0, dtype=f32)
    counts = np.array([1, 2], dtype=np.int32)
    tta_ref.det_append(src, np.array([2, 2], dtype=np.int32), True, dst, counts)
    assert counts.tolist() == [3, 3]                               # image 1: two rows offered, one fits (clamped to dst_stride)
    r = src[0, 1]
    assert np.array_equal(dst[0, 2], np.array([f32(1) - r[2], r[1], f32(1) - r[0], r[3], r[4], r[5], r[6]], dtype=f32))
    assert np.all(dst[0, 0] == -9.0) and np.all(dst[1, :2] == -9.0)
    assert np.array_equal(dst[1, 2, 3:], src[1, 0, 3:])


# ---- mny_nms_merge -----------------------------------------------------------------------------------------------------
def _row(x1, y1, x2, y2, conf, cls_score, cls):
    return [x1, y1, x2, y2, conf, cls_score, cls]


def test_merge_three_member_cluster_mean_by_hand():
    """weights 0.5, 0.25, 0.25 (conf * class score, exact); IoU(A, B) = IoU(A, C) = 0.21875 / 0.28125 = 0.78 > 0.45.  A far box of the
    same class and an overlapping box of another class are no members."""
    rows = np.array([_row(0.0, 0.0, 0.5, 0.5, 0.5, 1.0, 3),
                     _row(0.0625, 0.0, 0.5625, 0.5, 0.5, 0.5, 3),
                     _row(0.0, 0.0, 0.5, 0.5, 1.0, 1.0, 4),                      # other class, identical box
                     _row(0.0, 0.0625, 0.5, 0.5625, 0.25, 1.0, 3),
                     _row(0.75, 0.75, 1.0, 1.0, 1.0, 1.0, 3)], dtype=f32)       # same class, disjoint
    assert tta_ref.merge_members(rows, 0, 0.45) == [0, 1, 3]
    out = tta_ref.nms_merge(rows, [0, 4, 2], 0.45)
    assert np.array_equal(out[0], np.array([0.015625, 0.015625, 0.515625, 0.515625, 0.5, 1.0, 3], dtype=f32))
    assert np.array_equal(out[1], rows[4]) and np.array_equal(out[2], rows[2])   # single-member clusters: (w * x) / w == x


def test_merge_pair_exactly_at_threshold_is_not_merged():
    """IoU = 0.5 / (1 + 0.5 - 0.5) = 0.5 exactly in fp32; the compare is the strict (double)iou > thr of the NMS."""
    rows = np.array([_row(0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0), _row(0.0, 0.0, 1.0, 0.5, 0.5, 1.0, 0)], dtype=f32)
    assert tta_ref.iou32(rows[0], rows[1]) == f32(0.5)
    assert tta_ref.merge_members(rows, 0, 0.5) == [0]
    assert np.array_equal(tta_ref.nms_merge(rows, [0, 1], 0.5), rows)
    below = float(np.nextafter(0.5, 0.0))
    assert tta_ref.merge_members(rows, 0, below) == [0, 1]
    got = tta_ref.nms_merge(rows, [0], below)[0]
    assert np.array_equal(got[:4], np.array([0.0, 0.0, 1.0, f32((1.0 + 0.25) / 1.5)], dtype=f32))


def test_merge_zero_area_kept_box_keeps_itself():
    """a zero-area box has IoU 0 / 0 = NaN with itself (no compare holds) and is a member all the same: j == i"""
    rows = np.array([_row(0.3, 0.3, 0.3, 0.3, 0.9, 0.5, 1), _row(0.3, 0.3, 0.3, 0.3, 0.9, 0.5, 1)], dtype=f32)
    assert np.isnan(tta_ref.iou32(rows[0], rows[0]))
    assert tta_ref.merge_members(rows, 0, 0.45) == [0] and tta_ref.merge_members(rows, 1, 0.45) == [1]
    assert np.array_equal(tta_ref.nms_merge(rows, [0, 1], 0.45), rows)


def test_merge_zero_weights_fall_back_to_the_kept_row():
    rows = np.array([_row(0.0, 0.0, 0.5, 0.5, 0.0, 1.0, 2), _row(0.0625, 0.0, 0.5625, 0.5, 0.5, 0.0, 2)], dtype=f32)
    assert tta_ref.merge_members(rows, 0, 0.45) == [0, 1]
    assert np.array_equal(tta_ref.nms_merge(rows, [0], 0.45)[0], rows[0])


# ---- argument validation (no GPU) ---------------------------------------------------------------------------------------
def _cpu_model():
    from mobilenet_yolo_pytorch_amd import yolo
    from oracle import procedural
    return yolo(procedural.VOC_CONFIG)


def test_default_views():
    from mobilenet_yolo_pytorch_amd.tta import default_views
    assert default_views(352) == [(352, False), (320, True), (256, False)]      # 0.83 * 352 = 292.2, 0.67 * 352 = 235.8, up to 32s
    assert default_views(640) == [(640, False), (544, True), (448, False)]      # Ultralytics' sizes at 640
    assert default_views(32) == [(32, False), (32, True)]                       # the third view repeats the first: left out
    assert default_views(96) == [(96, False), (96, True)]
    for bad in (0, -32, 100, 352.0, None):
        with pytest.raises(ValueError):
            default_views(bad)


def test_tta_argument_validation():
    from mobilenet_yolo_pytorch_amd import MnyError
    from mobilenet_yolo_pytorch_amd.tta import TTA
    m = _cpu_model().eval()
    t = TTA(m, views=[(96, False), (64, True)], merge=False, nms_thr=0.5)
    assert t.views == [(96, False), (64, True)] and t.merge is False and t.nms_thr == 0.5
    for bad in ([], None, [(96, True)], [(100, False)], [(96, False), (48, True)], [(96, False), (64,)], [96], [(96, False), (0, False)],
                [(96, False), (64.0, True)], [(96, False), (64, "yes")]):
        with pytest.raises(ValueError):
            TTA(m, views=bad)
    with pytest.raises(ValueError):
        TTA(m, views=[(96, False)], nms_thr=float("nan"))
    m.train()
    with pytest.raises(MnyError, match="model.eval"):                            # refused before anything touches a device
        t(torch.zeros(1, 3, 96, 96))
