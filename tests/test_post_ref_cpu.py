"""CPU: the numpy restatement of the post-processing stages (tests/post_ref.py) on hand-worked answers and against the oracles, the
validation of PostProcess, and the argument errors of the three entry points (no compute call: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import post_ref
from oracle import nms_ref, procedural, yolo_ref

f32 = np.float32
INF = np.inf


def one_cell_head(cls_logits, obj_logit=INF):
    """a [1,1,1,5+C] head: tx = ty = tw = th = 0, objectness and class logits as given"""
    return np.array([0, 0, 0, 0, obj_logit] + list(cls_logits), dtype=f32).reshape(1, 1, 1, -1)


ANCHOR = np.array([[0.5, 0.25]], dtype=f32)


def test_one_cell_scores_are_exact():
    """logits from {-inf, 0, +inf}: sigmoid = {0, 0.5, 1} exactly, so conf * cls is in {0, 0.25, 0.5, 1}; tw = th = 0: the box is the
    anchor round the cell centre (0.5, 0.5)"""
    for obj, conf in ((0.0, 0.5), (INF, 1.0)):
        rows = post_ref.decode_candidates(one_cell_head([-INF, 0.0, INF], obj), ANCHOR, [0], 0.25, multi_label=True)[0]
        assert np.array_equal(rows, np.array([[0.25, 0.375, 0.75, 0.625, conf, 0.0, 0], [0.25, 0.375, 0.75, 0.625, conf, 0.5, 1],
                                              [0.25, 0.375, 0.75, 0.625, conf, 1.0, 2]], dtype=f32))
        assert np.array_equal(rows[:, 4] * rows[:, 5], np.array([0.0, 0.5 * conf, conf], dtype=f32))
    assert len(post_ref.decode_candidates(one_cell_head([0.0, 0.0, 0.0], -INF), ANCHOR, [0], 0.0, multi_label=True)[0]) == 0   # conf 0 > 0 fails


@pytest.mark.parametrize("obj,score_thr,want", [(0.0, 0.25, [2]),          # scores 0, 0.25, 0.5: 0.25 > 0.25 fails
                                                (0.0, 0.5, []),            # 0.5 > 0.5 fails
                                                (INF, 0.5, [2]),           # scores 0, 0.5, 1
                                                (INF, 0.25, [1, 2]),
                                                (0.0, 0.0, [1, 2]),        # 0 > 0 fails
                                                (0.0, -1.0, [0, 1, 2])])   # the score test is off: a score of 0 passes
def test_strict_compares_drop_the_equal_case(obj, score_thr, want):
    head = one_cell_head([-INF, 0.0, INF], obj)
    rows = post_ref.decode_candidates(head, ANCHOR, [0], 0.25, score_thr, multi_label=True)[0]
    assert rows[:, 6].tolist() == want
    single = post_ref.decode_candidates(head, ANCHOR, [0], 0.25, score_thr, multi_label=False)[0]
    assert single[:, 6].tolist() == ([2] if 2 in want else [])                     # the best class or nothing
    # the objectness compare is strict too: conf 0.5 against obj_thr 0.5
    assert len(post_ref.decode_candidates(one_cell_head([INF] * 3, 0.0), ANCHOR, [0], 0.5, multi_label=True)[0]) == 0
    assert len(post_ref.decode_candidates(one_cell_head([INF] * 3, 0.0), ANCHOR, [0], np.nextafter(f32(0.5), f32(0)), multi_label=True)[0]) == 3


def test_nan_fails_every_compare_and_first_maximum_wins():
    nan = one_cell_head([0.0, 0.0, 0.0], np.nan)
    assert len(post_ref.decode_candidates(nan, ANCHOR, [0], 0.0, multi_label=True)[0]) == 0
    rows = post_ref.decode_candidates(one_cell_head([0.0, np.nan, INF, INF]), ANCHOR, [0], 0.5, 0.25, multi_label=True)[0]
    assert rows[:, 6].tolist() == [0, 2, 3]                                          # the NaN class score fails the score test
    rows = post_ref.decode_candidates(one_cell_head([0.0, np.nan, INF, INF]), ANCHOR, [0], 0.5, multi_label=False)[0]
    assert rows[:, 5:].tolist() == [[1.0, 2.0]]                                      # first of the two maxima


def test_class_mask_across_the_word_boundary():
    C = 33
    words = post_ref.class_mask_words([0, 31, 32], C)
    assert words.dtype == np.uint32 and words.tolist() == [0x80000001, 1]
    head = one_cell_head([INF] * C)
    assert post_ref.decode_candidates(head, ANCHOR, [0], 0.5, multi_label=True, class_mask=words)[0][:, 6].tolist() == [0, 31, 32]
    assert post_ref.decode_candidates(head, ANCHOR, [0], 0.5, multi_label=True, class_mask=post_ref.class_mask_words([30, 32], C))[0][:, 6].tolist() == [30, 32]
    # single label: the best class (first maximum: 0) must itself be allowed
    assert len(post_ref.decode_candidates(head, ANCHOR, [0], 0.5, class_mask=post_ref.class_mask_words([31, 32], C))[0]) == 0
    best32 = one_cell_head([0.0] * 32 + [INF])
    assert post_ref.decode_candidates(best32, ANCHOR, [0], 0.5, class_mask=post_ref.class_mask_words([32], C))[0][:, 6].tolist() == [32]
    assert len(post_ref.decode_candidates(best32, ANCHOR, [0], 0.5, class_mask=post_ref.class_mask_words([31], C))[0]) == 0


def test_capacity_rule():
    cands = [np.arange(35, dtype=f32).reshape(5, 7), np.zeros((0, 7), dtype=f32), np.ones((2, 7), dtype=f32)]
    rows = np.full((3, 4, 7), -7, dtype=f32)
    counts, dropped = post_ref.decode_ex(cands, rows, 4, base_counts=[1, 0, 9])
    assert counts.tolist() == [4, 0, 9] and dropped.tolist() == [2, 0, 2]             # a base outside 0..row_stride writes nothing
    assert np.array_equal(rows[0, 1:], cands[0][:3]) and (rows[0, 0] == -7).all() and (rows[1:] == -7).all()


@pytest.mark.parametrize("hi,g", [(0, 11), (1, 22)])
def test_single_label_decode_equals_the_oracle(hi, g):
    """against oracle.yolo_ref.decode_rows at the decode tolerance of test_gpu_detect.py (rtol=0, atol=1e-4, class column exact)"""
    spec = yolo_ref.specs_from_config(procedural.VOC_CONFIG)[hi]
    spec.val_conf = 0.3
    N, A, T = 3, len(spec.mask), spec.attrs
    head = torch.from_numpy(np.random.default_rng(5 + hi).normal(0.0, 1.5, size=(N, g, g, A * T)).astype(f32))
    want = yolo_ref.decode_rows(head, spec, [352, 352], layout="nhwc")
    anchors = np.array([(aw / 352, ah / 352) for aw, ah in spec.anchors], dtype=f32)
    m_obj, _ = post_ref.margins(head.numpy(), anchors, spec.mask, 0.3)
    assert m_obj > 1e-5, "a conf within 1e-5 of the threshold: pick another seed"
    got = post_ref.decode_candidates(head.numpy(), anchors, spec.mask, 0.3)
    assert sum(len(r) for r in got) > 100
    for a, b in zip(got, want):
        b = b.numpy()
        assert a.shape == b.shape
        np.testing.assert_allclose(a[:, :6], b[:, :6], rtol=0, atol=1e-4)
        assert np.array_equal(a[:, 6], b[:, 6])


def _dense_rows(n, C, seed):
    """boxes on a coarse lattice (dense overlaps, exact IoU ties) and quantised scores (ties), as test_nms_indices_bit_exact's quant"""
    r = np.random.RandomState(seed)
    xy = np.round(r.rand(n, 2) * 16) / 16
    wh = 0.125 + np.round(r.rand(n, 2) * 4) / 16
    conf = np.round(r.rand(n, 1), 1) + 0.05
    return np.concatenate((xy - wh / 2, xy + wh / 2, conf, np.ones((n, 1)), r.randint(0, C, size=(n, 1))), 1).astype(f32)


@pytest.mark.parametrize("n", [0, 1, 65, 700])
def test_agnostic_nms_equals_the_oracle_on_class_zeroed_rows(n):
    rows = _dense_rows(n, 7, seed=n)
    zeroed = rows.copy()
    zeroed[:, 6] = 0
    _, want = nms_ref.nms_rows(torch.from_numpy(zeroed), 1, 0.45)
    got = post_ref.nms_agnostic(rows, 0.45)
    assert np.array_equal(got, want.numpy())
    if n == 700:
        _, per_class = nms_ref.nms_rows(torch.from_numpy(rows), 7, 0.45)
        assert len(per_class) > len(got) > 10                                        # the flag does something


def test_topk_order_ties_and_nan():
    rows = np.zeros((8, 7), dtype=f32)
    rows[:, 4] = 1.0
    rows[:, 5] = [0.5, 0.9, 0.5, np.nan, 0.9, -0.0, 0.0, np.inf]
    kept = np.array([6, 5, 4, 3, 2, 1, 0, 7])                                        # NMS output order: position r -> row kept[r]
    # +NaN ahead of +inf, then 0.9 twice (positions 2 and 5: rows 4, 1), 0.5 twice (rows 2, 0), +0 (row 6) ahead of -0 (row 5)
    order = [3, 7, 4, 1, 2, 0, 6, 5]
    assert post_ref.det_topk(rows, kept, 100).tolist() == order
    max_det = 4
    for k in (0, 1, max_det - 1, max_det, max_det + 1):
        got = post_ref.det_topk(rows, kept[:k], max_det)
        full = post_ref.det_topk(rows, kept[:k], 100)
        assert len(got) == min(k, max_det) and got.tolist() == full[:max_det].tolist()
        assert sorted(full.tolist()) == sorted(kept[:k].tolist())                    # k <= max_det only reorders
    assert post_ref.det_topk(rows, kept, 1).tolist() == [3]
    neg_nan = rows.copy()
    neg_nan[3, 5] = np.array([0xFFC00000], dtype=np.uint32).view(f32)[0]             # a NaN with the sign bit set sorts behind everything
    assert post_ref.det_topk(neg_nan, kept, 100).tolist() == [7, 4, 1, 2, 0, 6, 5, 3]


def test_postprocess_validation():
    from mobilenet_yolo_pytorch_amd import PostProcess
    p = PostProcess()
    assert (p.conf_thres, p.score_thres, p.iou_thres, p.multi_label, p.agnostic, p.max_det, p.classes, p.max_candidates) == \
        (None, None, 0.45, False, False, None, None, None)
    for kw in (dict(conf_thres=-0.1), dict(conf_thres=1.5), dict(score_thres=float("nan")), dict(iou_thres=2), dict(iou_thres=None),
               dict(multi_label="yes"), dict(agnostic=2), dict(max_det=0), dict(max_det=2.5), dict(max_det=True), dict(max_candidates=0),
               dict(classes=[]), dict(classes=[-1]), dict(classes=[1.0]), dict(classes=3)):
        with pytest.raises((ValueError, TypeError)):
            PostProcess(**kw)
    p = PostProcess(classes=[3, 1, 3], multi_label=True, max_det=1)
    assert p.classes == [1, 3]
    p.check_classes(4)
    with pytest.raises(ValueError, match=r"0\.\.2"):
        p.check_classes(3)
    # the default row stride: the worst case of the mode
    assert PostProcess().stride(1815, 20) == 1815 and PostProcess(classes=[1]).stride(1815, 20) == 1815
    assert PostProcess(multi_label=True).stride(1815, 20) == 1815 * 20 and p.stride(1815, 20) == 1815 * 2
    assert PostProcess(multi_label=True).stride(1815, 1) == 1815                     # multi_label with one class behaves as False
    assert PostProcess(multi_label=True, max_candidates=5000).stride(1815, 20) == 5000
    assert PostProcess(max_candidates=5000).stride(1815, 20) == 1815


def test_argument_errors_do_not_need_a_gpu():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    hp = _lib.YoloHead(1, 1, 1, 3, 1, 0.5, 0.2, 0.01)
    buf = ctypes.create_string_buffer(64)
    q = ctypes.c_void_p(ctypes.addressof(buf))                                       # (never dereferenced: every call fails its checks)
    with pytest.raises(_lib.MnyError, match="null pointer"):
        _lib.call("mny_yolo_decode_ex", None, None, None, ctypes.byref(hp), 0.1, -1.0, 0, None, None, 8, None, None, None, None)
    with pytest.raises(_lib.MnyError, match="null pointer"):                         # `dropped` is not optional
        _lib.call("mny_yolo_decode_ex", q, q, q, ctypes.byref(hp), 0.1, -1.0, 0, None, q, 8, None, q, None, None)
    with pytest.raises(_lib.MnyError, match="row_stride 0"):
        _lib.call("mny_yolo_decode_ex", q, q, q, ctypes.byref(hp), 0.1, -1.0, 0, None, q, 0, None, q, q, None)
    with pytest.raises(_lib.MnyError, match="NaN"):
        _lib.call("mny_yolo_decode_ex", q, q, q, ctypes.byref(hp), float("nan"), -1.0, 0, None, q, 8, None, q, q, None)
    bad = _lib.YoloHead(1, 1, 1, 0, 1, 0.5, 0.2, 0.01)
    with pytest.raises(_lib.MnyError, match="bad head spec"):
        _lib.call("mny_yolo_decode_ex", q, q, q, ctypes.byref(bad), 0.1, -1.0, 0, None, q, 8, None, q, q, None)
    with pytest.raises(_lib.MnyError, match="null pointer"):
        _lib.call("mny_nms_agnostic", None, None, None, 1, 8, 0, 0.45, None, None, None, None, None)
    with pytest.raises(_lib.MnyError, match="bad sizes"):
        _lib.call("mny_nms_agnostic", q, q, q, 0, 8, 0, 0.45, q, q, None, q, None)
    for max_det in (0, -3):
        with pytest.raises(_lib.MnyError, match="max_det"):
            _lib.call("mny_det_topk", q, q, 1, 8, max_det, q, q, None, q, q, None)
    with pytest.raises(_lib.MnyError, match="null pointer"):
        _lib.call("mny_det_topk", q, None, 1, 8, 5, q, q, None, q, q, None)
    _lib.call("mny_det_topk", None, None, 0, 0, 5, None, None, None, None, None, None)      # S == 0, no prefix asked for: nothing to do
    lib = _lib.load()
    assert lib.mny_nms_agnostic_ws_bytes(4, 1000) == lib.mny_nms_ws_bytes(4, 1000, 1)
    assert lib.mny_nms_agnostic_status_offset(4, 1000) == lib.mny_nms_status_offset(4, 1000, 1)
    assert lib.mny_nms_agnostic_prefix_offset(4, 1000) == lib.mny_nms_prefix_offset(4, 1000, 1)
    assert lib.mny_det_topk_ws_bytes(4, 1000) >= 1000 * 4 + 2 * 1000 * 8
