"""Validation report on the GPU (mny_det_curves / mny_det_confusion through the C ABI) against the float64 restatement
tests/report_ref.py on seeded inputs.  No tolerance anywhere: every integer output (tp, fp, npos, best, matrix, det_gt) is equal and
every fp64 output is equal bit for bit (the kernels are compiled with -ffp-contract=off and sum in the restatement's order).
Inputs are synthetic.map_case with its `difficult` flag as the crowd flag and the image sizes of tests/test_gpu_coco.py; the match
flags fed to the curves are the COCO restatement's (tests/coco_ref.py) at IoU 0.5, all areas, 100 detections per (image, class)."""
import numpy as np
import pytest
import torch

import coco_ref
import report_cases as cases
import report_ref

pytestmark = pytest.mark.gpu
_REF = {}
F = np.float32
COCO = {"iou_thrs": [0.5], "area_rngs": [[0, 1e10]], "max_dets": [100], "stat_desc": [[0, 0, 0, 0]]}
INT_KEYS, F64_KEYS = ("tp", "fp", "npos", "best"), ("precision", "recall", "f1", "mean_f1", "smooth_f1", "best_conf", "at_best")


@pytest.fixture(scope="module")
def em():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import evalmap
    return evalmap


def sizes_of(seed, n):
    r = np.random.RandomState(1000 + seed)
    return np.stack((r.randint(64, 1281, n), r.randint(48, 961, n)), 1).astype(np.float32)


def make(seed, n_images, nc, **kw):
    from mobilenet_yolo_pytorch_amd import synthetic
    return synthetic.map_case(n_images, nc, seed=seed, **kw), sizes_of(seed, n_images)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if not k.startswith("_")}


def flags(key, case, nc, sizes):
    """the COCO restatement's match flags, computed once per case and never modified"""
    if ("flags", key) not in _REF:
        r = coco_ref.evaluate(*case, nc, image_sizes=sizes, **COCO)
        _REF[("flags", key)] = (r["det_match"][0, 0].copy(), r["det_ignore"][0, 0].copy())
    return _REF[("flags", key)]


def same_bits(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def check_curves(em, key, args, G, W):
    """args: det_labels, det_scores, det_match, det_ignore, true_labels, true_crowd, n_classes"""
    if ("curves", key, G, W) not in _REF:
        _REF[("curves", key, G, W)] = report_ref.curves(*args, grid=G, smooth=W)
    ref = _REF[("curves", key, G, W)]
    got = host(em.det_curves(*[dev(a) for a in args[:6]], args[6], grid=G, smooth=W))
    for k in INT_KEYS:
        assert np.array_equal(got[k].reshape(-1), np.asarray(ref[k], got[k].dtype).reshape(-1)), k
    for k in F64_KEYS:
        assert same_bits(got[k], ref[k]), k                                       # bit for bit
    assert got["tp"].dtype == np.int64 and got["best"].dtype == np.int32 and got["precision"].shape == (args[6] - 1, G)
    return got, ref


def check_confusion(em, key, case, nc, sizes, **kw):
    if ("confusion", key) not in _REF:
        _REF[("confusion", key)] = report_ref.confusion(*case, nc, image_sizes=sizes, **kw)
    ref = _REF[("confusion", key)]
    got = host(em.det_confusion(*[dev(a) for a in case], nc, image_sizes=None if sizes is None else dev(sizes), **kw))
    assert np.array_equal(got["matrix"], ref["matrix"]) and got["matrix"].dtype == np.int64
    assert np.array_equal(got["det_gt"], ref["det_gt"]) and got["det_gt"].dtype == np.int32
    return got, ref


def check_both(em, key, case, nc, sizes, G, W, **kw):
    m, ig = flags(key, case, nc, sizes)
    c = check_curves(em, key, (case[1], case[2], m, ig, case[5], case[6], nc), G, W)
    return c, check_confusion(em, key, case, nc, sizes, **kw)


@pytest.mark.parametrize("seed,n_images,nc,G,W", [(0, 1, 2, 2, 1), (1, 7, 3, 5, 5), (2, 40, 21, 1000, 101), (4, 30, 255, 4096, 4095)])
def test_random_vs_restatement(em, seed, n_images, nc, G, W):
    case, sizes = make(seed, n_images, nc)
    (got, ref), (cgot, cref) = check_both(em, ("base", seed), case, nc, sizes, G, W)
    assert case[1].size <= 4096                                                   # the sort stays inside one LDS chunk
    assert np.diff(case[3]).max() * np.diff(case[7]).max() <= 4096                # every image's IoUs fit the LDS table
    if seed == 2:
        assert (ref["npos"] > 0).sum() >= 15 and 0 < ref["best"] < G - 1 and 0.2 < ref["smooth_f1"][ref["best"]] < 1
        assert np.trace(cref["matrix"]) > 30 and cref["matrix"][-1].sum() > 5 and cref["matrix"][:, -1].sum() > 5
        off = cref["matrix"][:-1, :-1].sum() - np.trace(cref["matrix"][:-1, :-1])
        assert off > 0                                                            # wrong-class matches land off the diagonal
    if seed == 4:
        assert (ref["npos"] == 0).sum() > 100 and (ref["at_best"][:-1][ref["npos"] == 0] == -1).all()


@pytest.mark.parametrize("G,W", [(2, 1), (5, 1), (5, 3), (1000, 1), (1000, 999), (4096, 101)])
def test_grid_sizes_and_windows(em, G, W):
    case, sizes = make(2, 40, 21)
    m, ig = flags(("base", 2), case, 21, sizes)
    check_curves(em, ("base", 2), (case[1], case[2], m, ig, case[5], case[6], 21), G, W)


def long_case():
    return make(15, 30, 2, mean_gt=40.0, det_per_gt=3.0, clutter=50.0)


def test_sort_beyond_one_chunk_and_class_segment_beyond_one_scan_block(em):
    """> 4096 detections: the pair sort leaves its LDS chunk; one class keeps > 1024 counted detections: its segment spans scan
    workgroups.  Most images have more pairs than the confusion kernel's LDS table holds, so their IoUs are recomputed."""
    case, sizes = long_case()
    assert case[1].size >= 4097
    m, ig = flags("long", case, 2, sizes)
    assert ((m != -2) & (ig == 0)).sum() > 2048 and (m == -2).sum() > 0
    (got, ref), (cgot, cref) = check_both(em, "long", case, 2, sizes, 1000, 101)
    assert ref["tp"][0, 0] > 500 and ref["fp"][0, 0] > 500
    pairs = np.diff(case[3]) * np.diff(case[7])
    assert (pairs > 4096).sum() >= 10 and (pairs <= 4096).sum() >= 1            # both forms of the matcher in one launch
    assert (cref["det_gt"] >= 0).sum() > 500


def test_three_classes_with_long_segments(em):
    """the TP scan runs over the whole sorted run: later classes start at a non-zero count inside a scan block"""
    case, sizes = make(12, 6, 3, mean_gt=60.0, det_per_gt=4.0, clutter=300.0)
    (got, ref), _ = check_both(em, "crowded", case, 3, sizes, 101, 11)
    assert (ref["tp"][:, 0] > 100).all() and ((ref["tp"] + ref["fp"])[:, 0] > 400).all()


def test_image_beyond_the_lds_table(em):
    case, sizes = make(13, 3, 2, mean_gt=300.0, det_per_gt=1.0, clutter=50.0)
    assert np.diff(case[7]).max() == 326 and (np.diff(case[3]) * np.diff(case[7])).max() > 50000
    _, ref = check_confusion(em, "wide", case, 2, sizes)
    assert (ref["det_gt"] >= 0).sum() > 300


def test_no_detections_and_no_objects(em):
    case, sizes = make(6, 9, 4, no_detections=True)
    assert case[1].size == 0
    z = (np.zeros(0, np.int32), np.zeros(0, np.uint8))
    got, _ = check_curves(em, "nodet", (case[1], case[2], z[0], z[1], case[5], case[6], 4), 50, 5)
    assert (got["tp"] == 0).all() and (got["fp"] == 0).all() and (got["npos"] > 0).all() and (got["precision"] == 1.0).all() and (got["f1"] == 0.0).all()
    cg, _ = check_confusion(em, "nodet", case, 4, sizes)
    assert cg["matrix"][-1, :-1].sum() == (case[6] == 0).sum() and cg["matrix"][:-1].sum() == 0
    case, sizes = make(6, 9, 4)
    case = list(case)
    case[4], case[5], case[6], case[7] = np.zeros((0, 4), F), np.zeros(0, F), np.zeros(0, F), np.zeros(10, np.int32)
    m, ig = flags("nogt", case, 4, sizes)
    got, _ = check_curves(em, "nogt", (case[1], case[2], m, ig, case[5], case[6], 4), 50, 5)
    assert (got["npos"] == 0).all() and (got["smooth_f1"] == -1).all() and got["best"][0] == 0 and got["fp"][:, 0].sum() == (ig == 0).sum() > 90
    cg, _ = check_confusion(em, "nogt", case, 4, sizes)
    assert cg["matrix"][:-1, -1].sum() == (case[2] > 0.25).sum() and cg["matrix"][:, :-1].sum() == 0


def test_every_detection_flagged_not_evaluated(em):
    case, sizes = make(1, 7, 3)
    m = np.full(case[1].size, -2, np.int32)
    got, _ = check_curves(em, "allskipped", (case[1], case[2], m, np.zeros(case[1].size, np.uint8), case[5], case[6], 3), 20, 3)
    assert (got["tp"] == 0).all() and (got["fp"] == 0).all() and (got["recall"][got["npos"] > 0] == 0).all()
    got, _ = check_curves(em, "allignored", (case[1], case[2], np.zeros_like(m), np.ones(case[1].size, np.uint8), case[5], case[6], 3), 20, 3)
    assert (got["tp"] == 0).all() and (got["fp"] == 0).all()


def test_duplicated_scores_and_boxes(em):
    """scores rounded to eighths tie everywhere and sit exactly on the points of a 9-point grid; every second detection and object
    repeats its neighbour's box, so equal IoUs meet the tie order of the matcher"""
    case, sizes = make(11, 30, 5, crafted=True)
    case = [a.copy() for a in case]
    case[2] = (np.round(case[2] * 8) / 8).astype(F)
    n = case[0].shape[0] // 2
    case[0][1:2 * n:2] = case[0][0:2 * n:2]
    n = case[4].shape[0] // 2
    case[4][1:2 * n:2] = case[4][0:2 * n:2]
    (got, ref), (cgot, cref) = check_both(em, "ties", case, 5, sizes, 9, 3)
    on_grid = np.isin(case[2].astype(np.float64), np.arange(9) / 8)
    assert on_grid.all() and (cref["det_gt"] >= 0).sum() > 10


def test_special_scores_and_labels(em):
    case, sizes = make(13, 20, 6)
    case = [a.copy() for a in case]
    case[2][::9], case[2][1::9], case[2][2::9] = np.nan, 1.5, -0.25
    case[1][3::7], case[1][4::7], case[1][5::7] = 0.0, 2.5, 6.0                   # background, fractional, == n_classes
    case[5][::5] = 0.0
    (got, ref), (cgot, cref) = check_both(em, "special", case, 6, sizes, 33, 5)
    assert (cref["det_gt"][3::7] == -2).all() and (cref["det_gt"][::9] == -2).all()
    assert (ref["fp"][:, -1] > 0).any()                                           # scores above 1 are still counted at c = 1


def test_without_image_sizes(em):
    case, _ = make(8, 20, 5)
    check_confusion(em, "nosize", case, 5, None, conf=0.1, iou_thr=0.3)


def test_accumulate_over_three_calls_equals_one_call(em):
    case, sizes = make(7, 30, 6)
    _, ref = check_confusion(em, "accum", case, 6, sizes)
    out = None
    for lo, hi in ((0, 11), (11, 12), (12, 30)):
        d0, d1, g0, g1 = case[3][lo], case[3][hi], case[7][lo], case[7][hi]
        part = (case[0][d0:d1], case[1][d0:d1], case[2][d0:d1], case[3][lo:hi + 1] - d0, case[4][g0:g1], case[5][g0:g1], case[6][g0:g1],
                case[7][lo:hi + 1] - g0)
        r = em.det_confusion(*[dev(a) for a in part], 6, image_sizes=dev(sizes[lo:hi]), out=out)
        assert out is None or r["matrix"] is out
        out = r["matrix"]
        assert np.array_equal(host(r)["det_gt"], np.where(ref["det_gt"][d0:d1] >= 0, ref["det_gt"][d0:d1] - g0, ref["det_gt"][d0:d1]))
    assert np.array_equal(out.cpu().numpy(), ref["matrix"])
    fresh = host(em.det_confusion(*[dev(a) for a in case], 6, image_sizes=dev(sizes)))   # without out= the matrix starts from zero
    assert np.array_equal(fresh["matrix"], ref["matrix"])


def test_two_runs_are_byte_identical(em):
    case, sizes = long_case()
    m, ig = flags("long", case, 2, sizes)
    args = [dev(a) for a in (case[1], case[2], m, ig, case[5], case[6])]
    a, b = host(em.det_curves(*args, 2)), host(em.det_curves(*args, 2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    a, b = host(em.det_confusion(*[dev(x) for x in case], 2, image_sizes=dev(sizes))), host(em.det_confusion(*[dev(x) for x in case], 2, image_sizes=dev(sizes)))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["curves_two_class", "curves_one_sided", "curves_no_positives"])
def test_hand_worked_curves(em, name):
    args, want = getattr(cases, name)()
    for W in (1, 3, 5):
        got, _ = check_curves(em, name, args, 5, W)
        for k in ("npos", "tp", "fp"):
            assert np.array_equal(got[k], np.array(want[k], np.int64)), k
    if name == "curves_two_class":
        assert got["best"][0] == 0 and got["at_best"][2, 0] == 0.5
    if name == "curves_no_positives":
        assert (got["at_best"] == -1).all() and (got["mean_f1"] == -1).all()


@pytest.mark.parametrize("name", sorted(cases.CONFUSION))
def test_hand_worked_confusion(em, name):
    images, nc, kw, matrix, det_gt = cases.CONFUSION[name]
    got = host(em.det_confusion(*[dev(a) for a in cases.pack(images)], nc, **kw))
    assert got["matrix"].tolist() == matrix and got["det_gt"].tolist() == det_gt


def test_evaluator_end_to_end(em):
    """[k,7] rows shaped like the NMS stage's output + per-image sizes -> add_packed -> compute_report, against the restatements on the
    same rows (eval_pack of the oracle, COCO flags of coco_ref, curves and matrix of report_ref)."""
    from oracle import map_ref
    r = np.random.RandomState(9)
    nc, n_img = 6, 12
    names = ["background"] + ["c%d" % i for i in range(1, nc)]
    ev = em.Evaluator(names)
    rows_all, tg_all, crowd_all, counts, do, to = [], [], [], [], [0], [0]
    sizes = sizes_of(9, n_img)
    for i in range(n_img):
        t = r.randint(0, 5)
        cxy, wh = 0.2 + 0.6 * r.rand(t, 2), 0.05 + 0.3 * r.rand(t, 2)
        tg = np.concatenate((r.randint(1, nc, (t, 1)), cxy, wh), 1).astype(F)
        k = 0 if i == 3 else t * 2 + r.randint(0, 5)
        rows = np.zeros((k, 7), F)
        for j in range(k):
            if t and j < 2 * t:
                g = tg[j % t]
                rows[j, :4] = [g[1] - g[3] / 2, g[2] - g[4] / 2, g[1] + g[3] / 2, g[2] + g[4] / 2] + r.randn(4) * 0.01
                rows[j, 6] = g[0] - 1 if r.rand() > 0.2 else r.randint(0, nc - 1)
            else:
                c, s = 0.2 + 0.6 * r.rand(2), 0.1 + 0.3 * r.rand(2)
                rows[j, :4] = np.concatenate((c - s / 2, c + s / 2))
                rows[j, 6] = r.randint(0, nc - 1)
            rows[j, 4:6] = 0.2 + 0.8 * r.rand(2)
        rows_all.append(rows); tg_all.append(tg); crowd_all.append((r.rand(t) < 0.2).astype(F))
        counts.append(k); do.append(do[-1] + k); to.append(to[-1] + t)
    half = n_img // 2
    for lo, hi in ((0, half), (half, n_img)):
        ev.add_packed(torch.from_numpy(np.concatenate(rows_all[lo:hi])).cuda(), counts[lo:hi], tg_all[lo:hi], sizes=sizes[lo:hi],
                      crowd=crowd_all[lo:hi])
    out = ev.compute_report(grid=50, smooth=5, conf=0.3, iou_thr=0.4)
    db, dl, ds, tb, tl, td = map_ref.eval_pack(np.concatenate(rows_all), np.concatenate(tg_all))
    do, to, crowd = np.array(do, np.int32), np.array(to, np.int32), np.concatenate(crowd_all)
    coco = coco_ref.evaluate(db, dl, ds, do, tb, tl, crowd, to, nc, image_sizes=sizes, **COCO)
    ref = report_ref.curves(dl, ds, coco["det_match"][0, 0], coco["det_ignore"][0, 0], tl, crowd, nc, grid=50, smooth=5)
    cref = report_ref.confusion(db, dl, ds, do, tb, tl, crowd, to, nc, image_sizes=sizes, conf=0.3, iou_thr=0.4)
    assert set(out) == {"best_conf", "P", "R", "F1", "per_class", "confusion", "curves"} and list(out["per_class"]) == names[1:]
    assert np.array_equal(out["confusion"], cref["matrix"]) and np.trace(cref["matrix"]) > 5
    assert same_bits([out["best_conf"], out["P"], out["R"], out["F1"]], [ref["best_conf"]] + ref["at_best"][-1].tolist())
    for k, name in enumerate(names[1:]):
        P, R, F1, n = out["per_class"][name]
        assert same_bits([P, R, F1], ref["at_best"][k]) and n == ref["npos"][k] and isinstance(n, int)
    for k in ("precision", "recall", "f1", "mean_f1", "smooth_f1"):
        assert same_bits(out["curves"][k], ref[k]), k
    assert np.array_equal(out["curves"]["tp"], ref["tp"]) and np.array_equal(out["curves"]["fp"], ref["fp"])
    assert same_bits(out["curves"]["conf"], np.array([j / 49 for j in range(50)]))
    assert 0 < out["best_conf"] < 1 and 0 < out["F1"] < 1
