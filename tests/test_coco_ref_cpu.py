"""CPU: known answers of the COCO-metric specification (tests/coco_ref.py, the restatement the device kernels of
csrc/cocoeval.hip are compared with in tests/test_gpu_coco.py), and the argument checks of its binding, which need no GPU.
Every expected value below is worked out by hand from the rules in include/mnyolo.h."""
import ctypes

import numpy as np
import pytest

import coco_ref

F = np.float32
NAMES = coco_ref.STAT_NAMES


def pack(images, n_classes=2, sizes=None, **kw):
    """images: [(dets, gts)] with dets = [(box, label, score)], gts = [(box, label, crowd)] -> coco_ref.evaluate(...)"""
    db, dl, ds, do, tb, tl, tc, to = [], [], [], [0], [], [], [], [0]
    for dets, gts in images:
        for b, l, s in dets:
            db.append(b); dl.append(l); ds.append(s)
        for b, l, c in gts:
            tb.append(b); tl.append(l); tc.append(c)
        do.append(len(dl)); to.append(len(tl))
    sizes = np.array(sizes if sizes is not None else [(100, 100)] * len(images), F)
    return coco_ref.evaluate(np.array(db, F).reshape(-1, 4), np.array(dl, F), np.array(ds, F), np.array(do, np.int32),
                             np.array(tb, F).reshape(-1, 4), np.array(tl, F), np.array(tc, F), np.array(to, np.int32), n_classes,
                             image_sizes=sizes, **kw)


def stats(r):
    return dict(zip(NAMES, r["stats"]))


def test_hand_case():
    r = pack([([([.1, .1, .3, .3], 1, .9), ([.4, .1, .5, .2], 1, .8), ([.6, .6, .9, .9], 1, .7)],
               [([.1, .1, .3, .3], 1, 0), ([.6, .6, .9, .9], 1, 0)])])
    assert (r["det_match"][:2] == np.array([0, -1, 1])).all() and not r["det_ignore"][:2].any()   # TP, FP, TP at every threshold
    assert r["det_ignore"][2:].all()                         # medium / large: the objects and the stray detection are all out of range
    s = stats(r)
    want = (51 + 50 * 2 / 3) / 101
    for k in ("AP", "AP50", "AP75", "APs"):                  # both objects are < 32^2 px
        assert abs(s[k] - want) < 1e-12, (k, s[k])
    assert abs(want - 0.834983) < 1e-6
    assert s["APm"] == -1 and s["APl"] == -1 and s["ARm"] == -1 and s["ARl"] == -1
    assert s["AR1"] == 0.5 and s["AR10"] == 1 and s["AR100"] == 1 and s["ARs"] == 1
    assert abs(r["per_class_ap"][0] - want) < 1e-12
    assert r["precision"].shape == (10, 101, 1, 4, 3) and r["recall"].shape == (10, 1, 4, 3)


def test_later_ground_truth_wins_an_iou_tie():
    box = [.2, .2, .6, .6]
    r = pack([([(box, 1, .9), (box, 1, .8)], [(box, 1, 0), (box, 1, 0)])])
    assert (r["det_match"][0, :, 0] == 1).all() and (r["det_match"][0, :, 1] == 0).all()
    assert stats(r)["AP"] > 1 - 1e-12


def test_stop_rule_keeps_a_counted_match_over_a_better_ignored_one():
    # det 30x30 px; A 23x23 px (IoU .588, small); B 33x33 px (IoU .826, > 32^2: ignored by the small range only)
    r = pack([([([.1, .1, .4, .4], 1, .9)], [([.1, .1, .33, .33], 1, 0), ([.1, .1, .43, .43], 1, 0)])])
    m, ig = r["det_match"], r["det_ignore"]
    assert m[0, 0, 0] == 1 and ig[0, 0, 0] == 0              # all areas: both count, the higher IoU wins
    assert m[1, 0, 0] == 0 and m[1, 1, 0] == 0 and ig[1, 0, 0] == 0      # small range, t = .50 / .55: A holds, the scan stops at B
    assert m[1, 2, 0] == 1 and ig[1, 2, 0] == 1              # t = .60: A misses, B (ignored) takes it and the detection is ignored
    assert m[1, 7, 0] == -1 and ig[1, 7, 0] == 0             # t = .85: nothing; the detection (900 px^2) is inside the small range: FP


def test_crowd_absorbs_detections():
    crowd = ([.1, .1, .9, .9], 1, 1)
    plain = ([.0, .0, .09, .09], 1, 0)
    dets = [([.2, .2, .4, .4], 1, .9), ([.5, .5, .7, .7], 1, .8), ([.3, .5, .5, .7], 1, .7), ([.0, .0, .09, .09], 1, .6),
            ([.82, .2, .92, .4], 1, .5)]                      # the last: 80 % inside the crowd -> IoU = inter / area(det) = .8
    r = pack([(dets, [crowd, plain])])
    m, ig = r["det_match"][0], r["det_ignore"][0]
    assert (m[:, :3] == 0).all() and (ig[:, :3] == 1).all()   # three detections on one crowd, none of them FP
    assert (m[:, 3] == 1).all() and not ig[:, 3].any()
    assert (m[:6, 4] == 0).all() and (ig[:6, 4] == 1).all()   # t <= .75: on the crowd (a box IoU would be 160 / 6440)
    assert (m[7:, 4] == -1).all() and not ig[7:, 4].any()     # t >= .85: unmatched, counted as FP
    assert abs(r["recall"][0, 0, 0, 2] - 1) < 1e-12 and abs(r["stats"][1] - 1) < 1e-12       # AP50: one TP, nothing else counted
    assert abs(r["stats"][0] - 1) < 1e-12                     # the FP at the high thresholds sits BELOW the TP: precision stays 1 up to recall 1


def test_unmatched_detection_outside_the_area_range_is_ignored():
    # a 50x50 px false positive at the top score, a 20x20 px object found below it
    r = pack([([([.4, .4, .9, .9], 1, .9), ([.1, .1, .3, .3], 1, .8)], [([.1, .1, .3, .3], 1, 0)])])
    s = stats(r)
    assert r["det_ignore"][1, 0, 0] == 1 and r["det_match"][1, 0, 0] == -1 and r["det_ignore"][0, 0, 0] == 0
    assert abs(s["AP"] - 0.5) < 1e-12 and abs(s["APs"] - 1) < 1e-12 and s["APm"] == -1


def test_segment_is_cut_at_the_last_cap():
    # 130 detections stored in ASCENDING score; only the one of rank 110 covers the object
    dets = [([.5, .5, .6, .6], 1, 0.1 + 0.005 * i) for i in range(130)]
    dets[129 - 110] = ([.1, .1, .3, .3], 1, dets[129 - 110][2])
    gts = [([.1, .1, .3, .3], 1, 0)]
    r = pack([(dets, gts)])
    assert (r["det_match"][:, :, :30] == -2).all() and (r["det_match"][:, :, 30:] == -1).all()
    assert stats(r)["AR100"] == 0 and stats(r)["AP"] == 0
    r = pack([(dets, gts)], max_dets=(1, 10, 200))
    assert (r["det_match"][0, :, 129 - 110] == 0).all() and r["stats"][8] == 1


def test_no_countable_object_gives_minus_one():
    # class 1: only a crowd; class 2: detections but no object; class 3: neither
    r = pack([([([.1, .1, .3, .3], 1, .9), ([.1, .1, .3, .3], 2, .8)], [([.1, .1, .3, .3], 1, 1)])], n_classes=4)
    assert (r["precision"] == -1).all() and (r["recall"] == -1).all()
    assert (r["stats"] == -1).all() and (r["per_class_ap"] == -1).all()
    assert r["det_match"][0, 0, 0] == 0 and r["det_ignore"][0, 0, 0] == 1 and r["det_match"][0, 0, 1] == -1


def test_score_ties_keep_image_then_stored_order():
    g = [.1, .1, .3, .3]
    r = pack([([([.5, .5, .7, .7], 1, .5)], []), ([(g, 1, .5), (g, 1, .5)], [(g, 1, 0)])])
    assert r["det_match"][0, 0].tolist() == [-1, 0, -1]       # inside the image the first stored of two equal scores takes the object
    assert abs(stats(r)["AP"] - 0.5) < 1e-12                  # the FP of image 0 sorts before the TP of image 1: precision 1/2
    r = pack([([(g, 1, .5), (g, 1, .5)], [(g, 1, 0)]), ([([.5, .5, .7, .7], 1, .5)], [])])
    assert abs(stats(r)["AP"] - 1) < 1e-12


def test_labels_outside_the_range_and_signed_zero_scores():
    g = [.1, .1, .3, .3]
    r = pack([([(g, 0, .9), (g, 1.5, .9), (g, 3, .9), (g, 1, -0.0), (g, 1, 0.0)], [(g, 1, 0), (g, 2.5, 0)])], n_classes=3)
    assert (r["det_match"][0, 0, :3] == -2).all() and r["det_match"][0, 0, 3] == 0 and r["det_match"][0, 0, 4] == -1
    assert r["recall"][0, 0, 0, 2] == 1 and (r["recall"][:, 1] == -1).all()


# ---- the binding checks its arguments before it needs a GPU ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def test_argument_errors_do_not_need_a_gpu(lib):
    import torch
    from mobilenet_yolo_pytorch_amd import evalmap
    z4, z1, off = torch.zeros(0, 4), torch.zeros(0), torch.zeros(2, dtype=torch.int32)
    base = (z4, z1, z1, off, z4, z1, z1, off, 3)
    with pytest.raises(ValueError, match="iou_thrs"):
        evalmap.coco_eval(*base, iou_thrs=np.linspace(.1, .9, 17))
    with pytest.raises(ValueError, match="rec_thrs"):
        evalmap.coco_eval(*base, rec_thrs=np.linspace(0, 1, 129))
    with pytest.raises(ValueError, match="max_dets"):
        evalmap.coco_eval(*base, max_dets=(10, 1, 100))
    with pytest.raises(ValueError, match="area_rngs"):
        evalmap.coco_eval(*base, area_rngs=np.zeros((9, 2)))
    with pytest.raises(ValueError, match="n_classes"):
        evalmap.coco_eval(*base[:-1], 300)
    with pytest.raises(ValueError, match="different numbers of images"):
        evalmap.coco_eval(z4, z1, z1, off, z4, z1, z1, torch.zeros(3, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        evalmap.coco_eval(*base)
    ev = evalmap.Evaluator(["background", "a", "b"])
    ev.add_packed(torch.zeros(0, 7), [0, 0], [np.zeros((0, 5), F), np.zeros((1, 5), F)])
    with pytest.raises(ValueError, match="image_size"):
        ev.compute_coco()
    with pytest.raises(ValueError, match="sizes"):
        ev.add_packed(torch.zeros(0, 7), [0], [np.zeros((0, 5), F)], sizes=[(1, 1), (2, 2)])
    with pytest.raises(ValueError, match="crowd"):
        ev.add_packed(torch.zeros(0, 7), [0], [np.zeros((2, 5), F)], crowd=[[1]])
    assert len(evalmap.COCO_STAT_NAMES) == 12


def test_library_limits_are_error_codes_with_a_text(lib):
    L = lib.load()
    thr = (ctypes.c_double * 129)(*([0.5] * 129))
    caps = (ctypes.c_int32 * 5)(1, 10, 100, 100, 100)
    area = (ctypes.c_double * 18)(*([0.0, 1e10] * 9))
    one = ctypes.c_void_p(8)                               # never dereferenced: every check below fails before the first launch

    def run(n_images=1, D=0, T=0, nc=3, n_iou=10, n_rec=101, n_cap=3, n_area=4):
        rc = L.mny_coco_eval(None, None, None, None, None, None, None, None, None, n_images, D, T, nc, thr, n_iou, thr, n_rec, caps, n_cap,
                             area, n_area, None, 0, one, one, None, one, None, None, one, None)
        return rc, L.mny_last_error().decode()

    for kw, word in (({"nc": 256}, "n_classes"), ({"n_images": 1 << 24}, "n_images"), ({"D": (1 << 30) + 1}, "D="), ({"n_iou": 17}, "IoU"),
                     ({"n_rec": 129}, "recall"), ({"n_cap": 5}, "caps"), ({"n_area": 9}, "area")):
        rc, msg = run(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
        assert L.mny_coco_ws_bytes(kw.get("D", 0), 0, kw.get("n_images", 1), kw.get("nc", 3), kw.get("n_iou", 10), kw.get("n_rec", 101),
                                   kw.get("n_area", 4), kw.get("n_cap", 3)) == 0
    assert L.mny_coco_ws_bytes(1000, 100, 10, 21, 10, 101, 4, 3) > 0
    caps[1] = 0
    rc, msg = run()
    assert rc == -1 and "ascending" in msg
