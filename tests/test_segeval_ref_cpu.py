"""CPU: the numpy restatement of the segmentation evaluator (tests/segeval_ref.py) against hand-worked answers and against
torch.nn.functional.interpolate, the argument checks of the three bindings (no GPU needed), and the input condition of every GPU
case of tests/test_gpu_segeval.py (so that a seed with too many near-ties is found here, not on the device)."""
import ctypes

import numpy as np
import pytest

import segeval_ref as R


def logit(p):
    return np.log(p / (1 - p))


def head_of(p):
    """probabilities [h,w,C] -> float64 logits (the hand cases tolerate the round trip: 1e-12)."""
    return logit(np.asarray(p, np.float64))


def test_2x2_to_4x4_by_hand():
    assert R.positions(4, 2)[0].tolist() == [0, 0, 0, 1] and R.positions(4, 2)[1].tolist() == [0, 1, 1, 1]
    assert R.positions(4, 2)[2].tolist() == [0.75, 0.25, 0.75, 0.25]     # row 0: both neighbours clamp to row 0, the weight is moot
    p = np.array([[[0.2], [0.6]], [[0.4], [0.8]]])
    v = R.upsample(head_of(p), 4, 4)[0]
    row = lambda a, b: np.array([a, .75 * a + .25 * b, .25 * a + .75 * b, b])
    top, bot = row(.2, .6), row(.4, .8)
    want = np.stack([top, .75 * top + .25 * bot, .25 * top + .75 * bot, bot])
    assert np.abs(v - want).max() < 1e-12
    assert abs(v[1, 1] - 0.35) < 1e-12 and abs(v[2, 2] - 0.65) < 1e-12


def test_identity_size_returns_the_probabilities():
    x = np.random.RandomState(0).normal(0, 2, (5, 6, 3))
    assert all((t == 0).all() for t in (R.positions(5, 5)[2], R.positions(6, 6)[2]))
    assert np.array_equal(R.upsample(x, 5, 6), R.sigmoid(x).transpose(2, 0, 1))


def test_one_row_head_and_edge_clamp():
    p = np.array([[[0.1], [0.5], [0.9]]])                    # h = 1: every output row reads row 0 twice
    v = R.upsample(head_of(p), 4, 6)[0]
    assert np.abs(v - v[0]).max() == 0
    assert np.abs(v[0] - np.array([.1, .2, .4, .6, .8, .9])).max() < 1e-12     # columns 0 and 5 sit outside the centres: clamped
    y0, y1, t = R.positions(48, 3)
    assert y0[0] == 0 and y1[0] == 0 and y0[-1] == 2 and y1[-1] == 2 and y0.min() == 0 and y1.max() == 2
    assert (R.positions(1, 4)[0] == 1).all() and R.positions(1, 4)[2][0] == 0.5                  # a 1-pixel image reads the middle


def test_tie_nan_and_threshold_rules():
    v = np.zeros((3, 1, 6))
    v[:, 0, 0] = [0.7, 0.7, 0.6]                              # tie above the threshold: the lowest channel
    v[:, 0, 1] = [0.5, 0.5, 0.5]                              # exactly 0.5 is not above it
    v[:, 0, 2] = [np.nan, 0.6, 0.2]                           # a NaN never wins
    v[:, 0, 3] = [np.nan, np.nan, np.nan]                     # ... and never passes the threshold
    v[:, 0, 4] = [0.2, 0.3, 0.9]
    v[:, 0, 5] = [0.2, 0.5 + 1e-7, 0.1]
    pred, amb = R.predict(v)
    assert pred[0].tolist() == [1, 0, 2, 0, 3, 2]
    assert amb[0].tolist() == [True, True, False, False, False, True]


def test_ignore_id_and_confusion_by_hand():
    pred = np.array([[0, 1, 2, 2], [1, 1, 0, 2]], np.uint8)
    lab = np.array([[0, 1, 1, 255], [3, 2, 0, 2]], np.uint8)
    conf, ign = R.confusion(pred, lab, 2)
    assert ign == 2 and conf.tolist() == [[2, 0, 0], [0, 1, 1], [0, 1, 1]]
    m = R.metrics(conf)
    assert m[0] == 1.0 and m[1] == 1 / 3 and m[2] == 1 / 3
    assert abs(m[3] - (1 + 2 / 3) / 3) < 1e-15 and abs(m[4] - 1 / 3) < 1e-15 and m[5] == 4 / 6


def test_iou_is_nan_at_an_empty_class():
    conf = np.array([[5, 0, 0], [0, 0, 0], [1, 0, 3]])
    m = R.metrics(conf)
    assert m[0] == 5 / 6 and np.isnan(m[1]) and m[2] == 3 / 4
    assert abs(m[3] - (5 / 6 + 3 / 4) / 2) < 1e-15 and m[4] == 3 / 4 and m[5] == 8 / 9
    assert np.isnan(R.metrics(np.zeros((3, 3), np.int64))).all()


@pytest.mark.parametrize("hw,HW", [((3, 5), (48, 80)), ((4, 7), (8, 21)), ((4, 7), (50, 90)), ((9, 11), (4, 5)), ((6, 6), (1, 1)), ((5, 4), (5, 4))])
def test_values_match_torch_interpolate(hw, HW):
    import torch
    x = np.random.RandomState(3).normal(0, 2, hw + (3,)).astype(np.float32)
    p = torch.sigmoid(torch.from_numpy(x).double()).permute(2, 0, 1)[None]
    want = torch.nn.functional.interpolate(p, size=HW, mode="bilinear", align_corners=False)[0].numpy()
    assert np.abs(R.upsample(x, *HW) - want).max() < 1e-12


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_case_meets_its_ambiguity_condition(name):
    x, labels = R.make_case(name)
    C = R.CASES[name][3]
    res = R.evaluate(x, labels, C)
    ok, n_amb, n_pix = R.ambiguity_ok(name, res)
    assert ok, "%s: %d of %d pixels are ambiguous" % (name, n_amb, n_pix)
    assert res["conf"].sum() + res["ignored"] == n_pix


# ---- the bindings check their arguments before they need a GPU -------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def test_confusion_argument_errors_do_not_need_a_gpu(lib):
    one = ctypes.c_void_p(4096)                              # never dereferenced: every check below fails before the first launch
    off = (ctypes.c_int64 * 2)(0, 4096)
    sz = (ctypes.c_int32 * 4)(48, 80, 48, 80)

    def run(match, head=one, N=2, h=3, w=5, C=2, labels=one, off=off, sz=sz, conf=one, ign=one, pred=None):
        with pytest.raises(lib.MnyError, match=match):
            lib.call("mny_seg_confusion", head, N, h, w, C, labels, off, sz, conf, ign, pred, None)
    run("null pointer", head=None)
    run("null pointer", off=None)
    run("null pointer", sz=None)
    run("null pointer", labels=None)                         # neither labels nor pred_out
    run("null pointer", conf=None)
    run("null pointer", ign=None)
    run("seg classes", C=0)
    run("seg classes", C=17)
    run("bad head shape", N=0)
    run("bad head shape", h=0)
    run("bad head shape", w=16385)
    run("LDS stage", w=6145, C=1)
    run("LDS stage", w=385, C=16)
    run("has size", sz=(ctypes.c_int32 * 4)(48, 80, 0, 80))
    run("has size", sz=(ctypes.c_int32 * 4)(48, 80, 48, 16385))
    run("multiple of 16", off=(ctypes.c_int64 * 2)(0, 3848))
    run("multiple of 16", off=(ctypes.c_int64 * 2)(0, -16))
    run("aligned", labels=ctypes.c_void_p(4100))
    run("aligned", pred=ctypes.c_void_p(4104))
    run("aligned", conf=ctypes.c_void_p(4100))


def test_upsample_argument_errors_do_not_need_a_gpu(lib):
    one = ctypes.c_void_p(4096)
    off = (ctypes.c_int64 * 1)(0)
    sz = (ctypes.c_int32 * 2)(48, 80)

    def run(match, head=one, N=1, h=3, w=5, C=2, sz=sz, off=off, out=one):
        with pytest.raises(lib.MnyError, match=match):
            lib.call("mny_seg_upsample", head, N, h, w, C, sz, off, out, None)
    run("null pointer", head=None)
    run("null pointer", sz=None)
    run("null pointer", off=None)
    run("null pointer", out=None)
    run("aligned", out=ctypes.c_void_p(4100))
    run("seg classes", C=17)
    run("bad head shape", h=16385)
    run("has size", sz=(ctypes.c_int32 * 2)(16385, 80))
    run("multiple of 4", off=(ctypes.c_int64 * 1)(6))


def test_metrics_argument_errors_do_not_need_a_gpu(lib):
    one = ctypes.c_void_p(4096)
    for args, match in (((None, 2, one, None), "null pointer"), ((one, 2, None, None), "null pointer"), ((one, 0, one, None), "seg classes"),
                        ((one, 17, one, None), "seg classes")):
        with pytest.raises(lib.MnyError, match=match):
            lib.call("mny_seg_metrics", *args)


def test_python_wrappers_check_before_they_launch(lib):
    import torch
    from mobilenet_yolo_pytorch_amd import segeval
    with pytest.raises(ValueError, match="outside 1..16"):
        segeval.SegEvaluator(17)
    with pytest.raises(ValueError, match="class_names"):
        segeval.SegEvaluator(2, class_names=["background", "direct"])
    with pytest.raises(ValueError, match=r"\[N,h,w,C\]"):
        segeval.upsample(torch.zeros(3, 5, 2), [(4, 4)])
    with pytest.raises(RuntimeError, match="CUDA"):
        segeval.predict(torch.zeros(1, 3, 5, 2), [(4, 4)])
