"""CPU: known answers of the validation-report specification (tests/report_ref.py, the restatement the device kernels of
csrc/detreport.hip are compared with in tests/test_gpu_report.py), and the argument checks of its binding, which need no GPU.
The cases and their hand-worked integer answers are in tests/report_cases.py; the fp64 values expected here are worked out by hand
from the rules in include/mnyolo.h."""
import ctypes

import numpy as np
import pytest

import coco_ref
import report_cases as cases
import report_ref

F = np.float32


def check_counts(r, want):
    for k in ("npos", "tp", "fp"):
        assert np.array_equal(r[k], np.array(want[k], np.int64)), k


def test_two_classes_every_count_by_hand():
    args, want = cases.curves_two_class()
    r = report_ref.curves(*args, grid=5, smooth=1)
    check_counts(r, want)                                    # .25 and .5 sit on grid values and are counted there; NaN / -0.1 nowhere; 1.5 everywhere
    assert r["precision"][0] == pytest.approx([2 / 3, 2 / 3, 1 / 2, 1, 1]) and r["precision"][0, 4] == 1.0     # no detection left: 1.0
    assert r["recall"][0] == pytest.approx([2 / 3, 2 / 3, 1 / 3, 1 / 3, 0])
    assert r["f1"][0] == pytest.approx([2 / 3, 2 / 3, .4, .5, 0])
    assert r["precision"][1] == pytest.approx([1 / 3] * 4 + [0]) and r["recall"][1] == pytest.approx([.5] * 4 + [0])
    assert r["f1"][1] == pytest.approx([.4] * 4 + [0]) and r["f1"][1, 4] == 0.0
    mean = [(2 / 3 + .4) / 2, (2 / 3 + .4) / 2, .4, .45, 0]
    assert r["mean_f1"] == pytest.approx(mean)
    assert np.array_equal(r["smooth_f1"], r["mean_f1"])      # W = 1: x / 1.0
    assert r["best"] == 0 and r["best_conf"] == 0.0          # points 0 and 1 tie: the first
    assert r["at_best"] == pytest.approx(np.array([[2 / 3, 2 / 3, 2 / 3], [1 / 3, .5, .4], [.5, 7 / 12, mean[0]]]))
    # F1 is exactly the stated expression, in the stated order
    P, R = 2.0 / 3.0, 2.0 / 3.0
    assert r["f1"][0, 0] == ((2.0 * P) * R) / ((P + R) + 1e-16)


def test_smoothing_window_is_clamped_at_both_ends():
    args, _ = cases.curves_two_class()
    m = report_ref.curves(*args, grid=5, smooth=1)["mean_f1"]
    r3, r5 = report_ref.curves(*args, grid=5, smooth=3), report_ref.curves(*args, grid=5, smooth=5)
    assert np.array_equal(r3["mean_f1"], m)
    want3 = [(((0.0 + m[0]) + m[0]) + m[1]) / 3.0, (((0.0 + m[0]) + m[1]) + m[2]) / 3.0, (((0.0 + m[1]) + m[2]) + m[3]) / 3.0,
             (((0.0 + m[2]) + m[3]) + m[4]) / 3.0, (((0.0 + m[3]) + m[4]) + m[4]) / 3.0]
    assert r3["smooth_f1"].tolist() == want3 and r3["best"] == 0
    assert r5["smooth_f1"][0] == (((((0.0 + m[0]) + m[0]) + m[0]) + m[1]) + m[2]) / 5.0
    assert r5["smooth_f1"][4] == (((((0.0 + m[2]) + m[3]) + m[4]) + m[4]) + m[4]) / 5.0
    assert r3["smooth_f1"] == pytest.approx([.5333333, .4888889, .4611111, .2833333, .15], abs=1e-6)


def test_grid_point_follows_the_detection_set_exactly():
    """G = 2: c = 0 and 1.  G = 4: c = 0, 1/3, 2/3, 1; float32 0.33333334 (> the double 1/3) is counted at point 1, 0.3333333 is not."""
    lab, ig = np.array([1, 1], F), np.zeros(2, np.uint8)
    up, dn = np.nextafter(F(1 / 3), F(1)), np.nextafter(F(1 / 3), F(0))
    assert float(F(1 / 3)) > 1 / 3 > float(dn)
    r = report_ref.curves(lab, np.array([F(1 / 3), dn], F), np.array([0, -1], np.int32), ig, np.array([1], F), np.zeros(1, F), 2, grid=4, smooth=1)
    assert r["tp"].tolist() == [[1, 1, 0, 0]] and r["fp"].tolist() == [[1, 0, 0, 0]]
    r = report_ref.curves(lab, np.array([1.0, up], F), np.array([0, -1], np.int32), ig, np.array([1], F), np.zeros(1, F), 2, grid=2, smooth=1)
    assert r["tp"].tolist() == [[1, 1]] and r["fp"].tolist() == [[1, 0]]


def test_class_without_detections_and_class_without_objects():
    args, want = cases.curves_one_sided()
    r = report_ref.curves(*args, grid=5, smooth=3)
    check_counts(r, want)
    assert (r["precision"][0] == 1.0).all() and (r["recall"][0] == 0.0).all() and (r["f1"][0] == 0.0).all()
    assert (r["precision"][1] == -1).all() and (r["recall"][1] == -1).all() and (r["f1"][1] == -1).all()
    assert (r["mean_f1"] == 0.0).all() and r["best"] == 0
    assert r["at_best"].tolist() == [[1.0, 0.0, 0.0], [-1.0, -1.0, -1.0], [1.0, 0.0, 0.0]]           # the means skip class 2


def test_no_positives_anywhere():
    args, want = cases.curves_no_positives()
    r = report_ref.curves(*args, grid=5, smooth=3)
    check_counts(r, want)
    for k in ("precision", "recall", "f1", "mean_f1", "smooth_f1", "at_best"):
        assert (r[k] == -1).all(), k
    assert r["best"] == 0 and r["best_conf"] == 0.0
    r = report_ref.curves(np.zeros(0, F), np.zeros(0, F), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, F), np.zeros(0, F), 2, grid=2, smooth=1)
    assert r["tp"].tolist() == [[0, 0]] and (r["at_best"] == -1).all()


@pytest.mark.parametrize("name", sorted(cases.CONFUSION))
def test_confusion_by_hand(name):
    images, nc, kw, matrix, det_gt = cases.CONFUSION[name]
    r = report_ref.confusion(*cases.pack(images), nc, **kw)
    assert r["matrix"].tolist() == matrix and r["det_gt"].tolist() == det_gt
    assert r["matrix"][-1, -1] == 0


def test_confusion_with_a_nan_box_and_image_sizes():
    """a NaN coordinate makes every IoU of the box NaN: never a candidate; image sizes scale both boxes and leave these IoUs unchanged"""
    images = [([([0, 0, cases.NAN, .5], 1, .9), (cases.Q, 1, .8)], [(cases.Q, 2, 0)])]
    r = report_ref.confusion(*cases.pack(images), 3, image_sizes=np.array([[640, 480]], F))
    assert r["det_gt"].tolist() == [-1, 0] and r["matrix"].tolist() == [[0, 1, 1], [0, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("seed,n_images,nc", [(0, 1, 2), (1, 7, 3), (2, 40, 21), (5, 25, 6)])
def test_random_cases_agree_with_the_coco_restatement(seed, n_images, nc):
    """recall at c = 0 is the COCO recall at the same threshold, bit for bit (ground truths of synthetic.map_case have positive area, its
    scores are positive), and the counts at c = 0 are all counted detections"""
    from mobilenet_yolo_pytorch_amd import synthetic
    case = synthetic.map_case(n_images, nc, seed=seed)
    coco = coco_ref.evaluate(*case, nc, iou_thrs=[0.5], area_rngs=[[0, 1e10]], max_dets=[100], stat_desc=[[0, 0, 0, 0]])
    m, ig = coco["det_match"][0, 0], coco["det_ignore"][0, 0]
    r = report_ref.curves(case[1], case[2], m, ig, case[5], case[6], nc, grid=11, smooth=3)
    assert np.array_equal(r["recall"][:, 0].view(np.int64), coco["recall"][0, :, 0, 0].view(np.int64))
    counted = (m != -2) & (ig == 0)
    assert np.array_equal((r["tp"] + r["fp"])[:, 0], np.bincount(case[1][counted].astype(int), minlength=nc)[1:])
    assert (np.diff(r["tp"], axis=1) <= 0).all() and (np.diff(r["fp"], axis=1) <= 0).all() and (r["tp"][:, -1] == 0).all()
    c = report_ref.confusion(*case, nc)
    considered = c["det_gt"] != -2
    assert considered.sum() == (case[2] > 0.25).sum()
    assert c["matrix"][:-1].sum() == (c["det_gt"] == -1).sum() + ((c["det_gt"] >= 0) & (case[6][c["det_gt"].clip(0)] == 0)).sum()
    assert c["matrix"][:, :-1].sum() == (case[6] == 0).sum() and c["matrix"][-1, -1] == 0
    hit = c["det_gt"][c["det_gt"] >= 0]
    assert len(np.unique(hit)) == len(hit)                   # one-to-one


@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def test_python_parameter_checks_come_before_any_launch():
    import torch
    from mobilenet_yolo_pytorch_amd import evalmap
    z, zi, zb = torch.zeros(0), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8)
    for kw, word in (({"grid": 1}, "grid"), ({"grid": 4097}, "grid"), ({"smooth": 4}, "smooth"), ({"smooth": 0}, "smooth"),
                     ({"grid": 5, "smooth": 7}, "smooth"), ({"n_classes": 256}, "n_classes")):
        with pytest.raises(ValueError, match=word):
            evalmap.det_curves(z, z, zi, zb, z, z, kw.pop("n_classes", 3), **kw)
    off = torch.zeros(1, dtype=torch.int32)
    for kw, word in (({"conf": 1.5}, "conf"), ({"conf": float("nan")}, "conf"), ({"iou_thr": -0.1}, "iou_thr"), ({"n_classes": 1}, "n_classes")):
        with pytest.raises(ValueError, match=word):
            evalmap.det_confusion(z.reshape(0, 4), z, z, off, z.reshape(0, 4), z, z, off, kw.pop("n_classes", 3), **kw)
    with pytest.raises(ValueError, match="different numbers"):
        evalmap.det_confusion(z.reshape(0, 4), z, z, off, z.reshape(0, 4), z, z, torch.zeros(2, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        evalmap.det_curves(z, z, zi, zb, z, z, 3)
    ev = evalmap.Evaluator(["background", "a", "b"])
    ev.add_packed(torch.zeros(0, 7), [0], [np.zeros((1, 5), F)])
    with pytest.raises(ValueError, match="image_size"):
        ev.compute_report()
    with pytest.raises(TypeError, match="unknown"):
        ev.compute_report(image_size=(10, 10), colour="red")


def test_library_limits_are_error_codes_with_a_text(lib):
    L = lib.load()
    one = ctypes.c_void_p(8)                                # never dereferenced: every check below fails before the first launch

    def curves(D=0, T=0, nc=3, G=1000, W=101):
        rc = L.mny_det_curves(None, None, None, None, D, None, None, T, nc, G, W, *([one] * 12), None)
        return rc, L.mny_last_error().decode(), L.mny_det_curves_ws_bytes(D, T, nc, G, W)

    for kw, word in (({"nc": 256}, "n_classes"), ({"nc": 1}, "n_classes"), ({"D": (1 << 30) + 1}, "D="), ({"T": (1 << 30) + 1}, "T="), ({"G": 1}, "grid"),
                     ({"G": 4097}, "grid"), ({"W": 100}, "window"), ({"G": 50, "W": 51}, "window"), ({"W": -1}, "window")):
        rc, msg, nb = curves(**kw)
        assert rc == -1 and word in msg and nb == 0, (kw, rc, msg, nb)
    assert L.mny_det_curves_ws_bytes(0, 0, 2, 2, 1) > 0 and L.mny_det_curves_ws_bytes(600000, 200000, 11, 1000, 101) >= 600000 * 16
    rc, msg, _ = curves(D=5)
    assert rc == -1 and "null detection" in msg

    def confusion(n_images=1, D=0, T=0, nc=3, conf=0.25, thr=0.45, acc=0):
        rc = L.mny_det_confusion(None, None, None, None, None, None, None, None, None, n_images, D, T, nc, conf, thr, acc, one, None, one, None)
        return rc, L.mny_last_error().decode(), L.mny_det_confusion_ws_bytes(D, T, n_images, nc)

    for kw, word in (({"nc": 256}, "n_classes"), ({"n_images": 1 << 24}, "n_images"), ({"D": (1 << 30) + 1}, "D="), ({"T": -1}, "T=")):
        rc, msg, nb = confusion(**kw)
        assert rc == -1 and word in msg and nb == 0, (kw, rc, msg, nb)
    for kw, word in (({"conf": float("nan")}, "NaN"), ({"thr": float("nan")}, "NaN"), ({"acc": 2}, "accumulate"), ({"D": 3}, "null detection"),
                     ({"T": 3}, "null ground-truth")):
        rc, msg, nb = confusion(**kw)
        assert rc == -1 and word in msg and nb > 0, (kw, rc, msg, nb)
