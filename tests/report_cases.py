"""Hand-worked cases of the validation report (include/mnyolo.h: mny_det_curves, mny_det_confusion), shared by the CPU test of the
restatement (tests/test_report_ref_cpu.py) and the GPU test of the kernels (tests/test_gpu_report.py).  Every expected value is
worked out by hand from the rules in the header; box coordinates are multiples of 1/8, so every IoU below is an exact double."""
import numpy as np

F = np.float32
NAN = float("nan")


# ---- curves: (args of report_ref.curves before grid / smooth, expected integer outputs) --------------------------------------------------
def curves_two_class():
    """K = 2, made for G = 5 (c = 0, .25, .5, .75, 1).  Class 1: TPs at .9 and .25 (on a grid value), an FP at .5 (on a grid value), and
    four detections that do not count (ignored, not evaluated, label 0, label 1.5).  Class 2: a TP and an FP tied at .8, an FP at 1.5
    (counted everywhere), TPs with a NaN score and at -0.1 (counted nowhere).  Ground truths: 3 of class 1 + a crowd, 2 of class 2."""
    #                 0    1    2    3    4    5    6    7     8    9   10   11
    labels = np.array([1, 1, 1, 1, 2, 2, 2, 2, 2, 1, 0, 1.5], F)
    scores = np.array([.9, .5, .25, .6, .8, .8, NAN, 1.5, -.1, .7, .9, .9], F)
    match = np.array([3, -1, 0, -1, -1, 1, 2, -1, 5, -2, 1, 1], np.int32)
    ignore = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    tl, tc = np.array([1, 1, 1, 2, 2, 1], F), np.array([0, 0, 0, 0, 0, 1], F)
    want = {"npos": [3, 2], "tp": [[2, 2, 1, 1, 0], [1, 1, 1, 1, 0]], "fp": [[1, 1, 1, 0, 0], [2, 2, 2, 2, 1]]}
    return (labels, scores, match, ignore, tl, tc, 3), want


def curves_one_sided():
    """class 1 has ground truths and no detection (P 1, R 0, F1 0), class 2 detections and no ground truth (-1, counts still exact)"""
    labels, scores = np.array([2, 2, 2], F), np.array([.9, .5, .1], F)
    match, ignore = np.array([-1, -1, -1], np.int32), np.zeros(3, np.uint8)
    return (labels, scores, match, ignore, np.array([1, 1], F), np.zeros(2, F), 3), {"npos": [2, 0], "tp": [[0] * 5] * 2, "fp": [[0] * 5, [3, 2, 2, 1, 0]]}


def curves_no_positives():
    labels, scores = np.array([1, 2], F), np.array([.9, .5], F)
    match, ignore = np.array([-1, -1], np.int32), np.zeros(2, np.uint8)
    return (labels, scores, match, ignore, np.zeros(0, F), np.zeros(0, F), 3), {"npos": [0, 0], "tp": [[0] * 5] * 2, "fp": [[1, 1, 1, 1, 0], [1, 1, 1, 0, 0]]}


# ---- confusion ---------------------------------------------------------------------------------------------------------------------------
def pack(images):
    """images: [(dets, gts)] with dets = [(box, label, score)], gts = [(box, label, crowd)] -> the eight packed arrays"""
    db, dl, ds, do, tb, tl, tc, to = [], [], [], [0], [], [], [], [0]
    for dets, gts in images:
        for b, l, s in dets:
            db.append(b); dl.append(l); ds.append(s)
        for b, l, c in gts:
            tb.append(b); tl.append(l); tc.append(c)
        do.append(len(dl)); to.append(len(tl))
    return (np.array(db, F).reshape(-1, 4), np.array(dl, F), np.array(ds, F), np.array(do, np.int32),
            np.array(tb, F).reshape(-1, 4), np.array(tl, F), np.array(tc, F), np.array(to, np.int32))


Q = [0, 0, .5, .5]            # a quarter of the image
UPPER = [0, 0, .5, .25]       # its upper half: IoU with Q exactly 0.5
RIGHT = [.5, 0, 1, .5]        # the quarter beside Q
BETWEEN = [.25, 0, .75, .5]   # half on Q, half on RIGHT: IoU 1/3 with both, the same double
FAR = [.5, .5, 1, 1]

# name -> (images, n_classes, {conf, iou_thr}, matrix, det_gt); matrix rows = predicted class, columns = true class, last = background
CONFUSION = {
    # the lower-scored detection fits better and takes the ground truth: scores decide nothing beyond the conf gate
    "two_detections_on_one_object": ([([(UPPER, 1, .9), (Q, 1, .8)], [(Q, 1, 0)])], 3, {"iou_thr": .45},
                                     [[1, 0, 1], [0, 0, 0], [0, 0, 0]], [-1, 0]),
    # equal IoUs: the smaller ground-truth index wins; it has class 2, so the match lands off the diagonal and object 1 is missed
    "one_detection_between_two_objects": ([([(BETWEEN, 1, .9)], [(Q, 2, 0), (RIGHT, 1, 0)])], 3, {"iou_thr": .3},
                                          [[0, 1, 0], [0, 0, 0], [1, 0, 0]], [0]),
    # equal IoUs: the smaller stored detection index wins, whatever the scores
    "duplicate_detections": ([([(Q, 2, .5), (Q, 2, .9)], [(Q, 2, 0)])], 3, {},
                             [[0, 0, 0], [0, 1, 1], [0, 0, 0]], [0, -1]),
    "iou_equal_to_the_threshold_is_no_match": ([([(UPPER, 1, .9)], [(Q, 1, 0)])], 3, {"iou_thr": .5},
                                               [[0, 0, 1], [0, 0, 0], [1, 0, 0]], [-1]),
    "score_equal_to_conf_is_not_considered": ([([(Q, 1, .25), (FAR, 2, .5)], [(Q, 1, 0)])], 3, {"conf": .25},
                                              [[0, 0, 0], [0, 0, 1], [1, 0, 0]], [-2, -1]),
    # the crowd and the detection on it add nothing; a second detection on the crowd finds it taken (one-to-one) and is a false positive
    "crowd_match": ([([(Q, 1, .9), (Q, 2, .8), (RIGHT, 2, .7)], [(Q, 1, 1), (RIGHT, 1, 0)])], 3, {},
                    [[0, 0, 0], [1, 0, 1], [0, 0, 0]], [0, -1, 1]),
    # image 0: detections only; image 1: objects only; image 2: nothing; image 3: a plain hit.  Labels 0 and 2.5 are nobody's class
    "empty_images": ([([(Q, 1, .9), (FAR, 2, .9), (Q, 0, .9)], []), ([], [(Q, 2, 0), (FAR, 2, 1), (Q, 2.5, 0)]), ([], []),
                      ([(FAR, 2, .3)], [(FAR, 2, 0)])], 3, {},
                     [[0, 0, 1], [0, 1, 1], [0, 1, 0]], [-1, -1, -2, 3]),
}
