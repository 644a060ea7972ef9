"""COCO-style metrics on the GPU (mny_coco_eval through the C ABI) against the float64 restatement tests/coco_ref.py on seeded inputs.
Match and ignore flags are equal, precision / recall (one fp64 division of exact counts each) are equal bit for bit, the means
(stats, per_class_ap) are within n * 2^-52 of the reference, n the number of entries averaged: a reordered sum of n values in
[0, 1] moves by no more than that.  Inputs are synthetic.map_case with its `difficult` flag as the crowd flag."""
import numpy as np
import pytest
import torch

import coco_ref

pytestmark = pytest.mark.gpu
_REF = {}


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


def reference(key, case, nc, sizes, **params):
    """the restatement's answer, computed once per case and never modified"""
    if key not in _REF:
        _REF[key] = coco_ref.evaluate(*case, nc, image_sizes=sizes, **params)
    return _REF[key]


def run(em, case, nc, sizes, **params):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = em.coco_eval(*[dev(a) for a in case], nc, image_sizes=None if sizes is None else dev(sizes), matches=True, **params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if not k.startswith("_")}


def n_averaged(ref, stat_desc):
    """entries > -1 of each statistic's slice, and of each class's AP slice"""
    P, R = ref["precision"], ref["recall"]
    ns = []
    for is_recall, ti, a, m in stat_desc:
        s = R[:, :, a, m] if is_recall else P[:, :, :, a, m]
        s = s if ti < 0 else s[ti:ti + 1]
        ns.append(int((s > -1).sum()))
    return np.array(ns), np.array([int((P[:, :, k, 0, -1] > -1).sum()) for k in range(P.shape[2])])


def compare(got, ref, stat_desc=coco_ref.DEFAULT_STATS):
    assert np.array_equal(got["det_match"], ref["det_match"])
    assert np.array_equal(got["det_ignore"], ref["det_ignore"])
    assert got["precision"].shape == ref["precision"].shape and got["recall"].shape == ref["recall"].shape
    assert np.array_equal(got["precision"].view(np.int64), ref["precision"].view(np.int64))        # bit for bit
    assert np.array_equal(got["recall"].view(np.int64), ref["recall"].view(np.int64))
    ns, nk = n_averaged(ref, stat_desc)
    for name, g, w, n in (("stats", got["stats"], ref["stats"], ns), ("per_class_ap", got["per_class_ap"], ref["per_class_ap"], nk)):
        err = np.abs(g - w)
        print(name, "max error %.3g, bound %.3g" % (err.max() if err.size else 0, (n * 2.0 ** -52).max() if n.size else 0))
        assert (err <= n * 2.0 ** -52).all(), (name, g, w)
        assert ((g == -1) == (n == 0)).all()


def check(em, key, case, nc, sizes, **params):
    ref = reference(key, case, nc, sizes, **params)
    got = run(em, case, nc, sizes, **params)
    compare(got, ref, np.asarray(params.get("stat_desc", coco_ref.DEFAULT_STATS)))
    return got, ref


@pytest.mark.parametrize("seed,n_images,nc", [(0, 1, 2), (1, 7, 3), (2, 40, 21), (3, 150, 21), (4, 64, 81)])
def test_random_vs_restatement(em, seed, n_images, nc):
    case, sizes = make(seed, n_images, nc)
    _, ref = check(em, ("base", seed), case, nc, sizes)
    m, ig = ref["det_match"], ref["det_ignore"]
    if seed == 2:
        per_t = (m[0] >= 0).sum(1)
        assert per_t[0] == 62 and per_t[-1] == 5 and (np.diff(per_t) <= 0).all()
        hit = m[0, 0][m[0, 0] >= 0]
        assert (case[6][hit] != 0).sum() == 9                                     # matches on crowds
        assert ((m[2, 0] == -1) & (ig[2, 0] == 1)).sum() == 194                   # unmatched, ignored by the medium range
    if seed == 3:
        assert (ref["stats"][3:6] > -1).all() and (ref["stats"][9:12] > -1).all()  # all four area ranges populated
    if seed == 4:
        empty = (ref["per_class_ap"] == -1).mean()
        assert 0.15 <= empty <= 0.25 and (ref["precision"][:, :, ref["per_class_ap"] == -1] == -1).all()


def crowded():
    return make(12, 6, 3, mean_gt=60.0, det_per_gt=4.0, clutter=300.0)


def test_capped_segments_and_runs_beyond_one_scan_chunk(em):
    case, sizes = crowded()
    _, ref = check(em, "crowded", case, 3, sizes)
    assert case[1].size == 3147
    cls, img = case[1].astype(int), np.searchsorted(case[3], np.arange(case[1].size), side="right") - 1
    seg = np.bincount(img * 3 + cls, minlength=18)
    assert (seg > 100).sum() == 12 and ((ref["det_match"][0, 0] == -2).sum() == (seg - 100).clip(0).sum())
    gseg = np.bincount((np.searchsorted(case[7], np.arange(case[5].size), side="right") - 1) * 3 + case[5].astype(int), minlength=18)
    assert gseg.max() == 35
    assert seg.reshape(6, 3).sum(0).max() > 1024                                  # a class run longer than one scan chunk


def test_kept_detections_of_a_class_beyond_one_scan_chunk(em):
    """Detections past the last cap leave the class's run before the scan, so the run above is short; here > 1024 stay in one."""
    case, sizes = make(15, 14, 2, mean_gt=40.0, det_per_gt=3.0, clutter=50.0)
    p = {"iou_thrs": [0.5, 0.75], "stat_desc": [[0, -1, 0, 2], [0, 1, 0, 2], [1, -1, 0, 2], [0, -1, 2, 2]]}
    _, ref = check(em, "longrun", case, 2, sizes, **p)
    assert (ref["det_match"][0, 0] != -2).sum() > 1024


def test_iou_table_beyond_lds_is_recomputed(em):
    case, sizes = make(13, 3, 2, mean_gt=300.0, det_per_gt=1.0, clutter=50.0)
    assert np.diff(case[7]).max() == 326                                          # 100 x 326 fp64 IoUs: no table
    check(em, "wide", case, 2, sizes)


def test_more_objects_than_the_lds_lists_hold(em):
    """> 512 objects of one class in one image: object list and matched words live in the workspace.  One threshold and two area
    ranges keep the restatement's loops short."""
    case, sizes = make(14, 2, 2, mean_gt=700.0, det_per_gt=0.3, clutter=20.0)
    assert np.diff(case[7]).max() > 600
    p = {"iou_thrs": [0.5], "area_rngs": [[0, 1e10], [0, 150 ** 2]], "stat_desc": [[0, 0, 0, 2], [1, 0, 1, 2]]}
    _, ref = check(em, "huge", case, 2, sizes, **p)
    assert (ref["det_match"][0, 0] >= 0).sum() > 20


def test_crafted_duplicate_empty_image_and_image_without_detections(em):
    case, sizes = make(5, 12, 4, crafted=True)
    check(em, "crafted", case, 4, sizes)
    assert case[7][3] == case[7][2] and case[3][5] == case[3][4]


def test_score_ties_keep_stored_order(em):
    case, sizes = make(11, 30, 5)
    case = list(case)
    case[2] = (np.round(case[2] * 8) / 8).astype(np.float32)                     # 8 distinct scores: ties everywhere
    check(em, "ties", case, 5, sizes)


def test_empty_halves(em):
    case, sizes = make(6, 9, 4, no_detections=True)
    got, _ = check(em, "nodet", case, 4, sizes)
    assert case[1].size == 0 and set(np.unique(got["precision"])) <= {-1.0, 0.0} and set(np.unique(got["recall"])) <= {-1.0, 0.0}
    case, sizes = make(6, 9, 4)
    case = list(case)
    case[4], case[5], case[6], case[7] = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(10, np.int32)
    got, _ = check(em, "nogt", case, 4, sizes)
    assert (got["precision"] == -1).all() and (got["stats"] == -1).all() and (got["det_match"] < 0).all()


def test_non_default_parameters(em):
    case, sizes = make(7, 30, 6)
    p = {"iou_thrs": [0.6], "max_dets": (5, 50), "area_rngs": [[0, 200 ** 2]], "rec_thrs": np.linspace(0, 1, 11),
         "stat_desc": [[0, 0, 0, 1], [0, -1, 0, 0], [1, 0, 0, 0], [1, -1, 0, 1]]}
    got, _ = check(em, "params", case, 6, sizes, **p)
    assert got["precision"].shape == (1, 11, 5, 1, 2)


def test_more_than_64_area_threshold_pairs(em):
    """7 area ranges x 16 thresholds = 112 lanes: two waves per segment, two mask words per detection."""
    case, sizes = make(9, 25, 4, mean_gt=4.0)
    edges = [0, 40 ** 2, 80 ** 2, 120 ** 2, 200 ** 2, 320 ** 2, 1e10]
    p = {"iou_thrs": np.linspace(.2, .95, 16), "area_rngs": [[0, 1e10]] + [[edges[i], edges[i + 1]] for i in range(6)],
         "stat_desc": [[0, -1, 0, 2], [0, 15, 6, 2], [1, -1, 5, 1], [0, 3, 4, 0], [1, 9, 6, 2]]}
    _, ref = check(em, "pairs112", case, 4, sizes, **p)
    assert (ref["stats"] > -1).all() and (ref["det_match"][6, 0] >= 0).any() and (ref["det_match"][5] >= 0).any()


def test_without_image_sizes(em):
    case, _ = make(8, 20, 5)
    p = {"area_rngs": [[0, 1e10], [0, 0.04], [0.04, 0.1], [0.1, 1e10]]}           # normalised boxes: areas of the unit square
    check(em, "nosize", case, 5, None, **p)


def test_labels_outside_the_class_range_are_never_evaluated(em):
    case, sizes = make(13, 20, 6)
    case = list(case)
    dl = case[1].copy()
    dl[::7], dl[1::7], dl[2::7] = 0.0, 2.5, 6.0                                   # background, fractional, == n_classes
    case[1] = dl
    tl = case[5].copy()
    tl[::5] = 0.0
    case[5] = tl
    got, _ = check(em, "labels", case, 6, sizes)
    assert (got["det_match"][:, :, ::7] == -2).all() and (got["det_match"][:, :, 1::7] == -2).all() and (got["det_match"][:, :, 2::7] == -2).all()


def test_two_runs_are_byte_identical(em):
    case, sizes = crowded()
    a, b = run(em, case, 3, sizes), run(em, case, 3, sizes)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_evaluator_end_to_end(em):
    """[k,7] rows shaped like the NMS stage's output + per-image sizes -> add_packed -> compute_coco, against the restatement on the same
    rows; compute() (VOC07) of the same evaluator still equals the oracle."""
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
        tg = np.concatenate((r.randint(1, nc, (t, 1)), cxy, wh), 1).astype(np.float32)
        k = 0 if i == 3 else t * 2 + r.randint(0, 5)
        rows = np.zeros((k, 7), np.float32)
        for j in range(k):
            if t and j < 2 * t:
                g = tg[j % t]
                rows[j, :4] = [g[1] - g[3] / 2, g[2] - g[4] / 2, g[1] + g[3] / 2, g[2] + g[4] / 2] + r.randn(4) * 0.01
                rows[j, 6] = g[0] - 1
            else:
                c, s = 0.2 + 0.6 * r.rand(2), 0.1 + 0.3 * r.rand(2)
                rows[j, :4] = np.concatenate((c - s / 2, c + s / 2))
                rows[j, 6] = r.randint(0, nc - 1)
            rows[j, 4:6] = 0.2 + 0.8 * r.rand(2)
        rows_all.append(rows); tg_all.append(tg); crowd_all.append((r.rand(t) < 0.2).astype(np.float32))
        counts.append(k); do.append(do[-1] + k); to.append(to[-1] + t)
    half = n_img // 2
    for lo, hi in ((0, half), (half, n_img)):
        ev.add_packed(torch.from_numpy(np.concatenate(rows_all[lo:hi])).cuda(), counts[lo:hi], tg_all[lo:hi], sizes=sizes[lo:hi],
                      crowd=crowd_all[lo:hi])
    out = ev.compute_coco()
    db, dl, ds, tb, tl, td = map_ref.eval_pack(np.concatenate(rows_all), np.concatenate(tg_all))
    do, to = np.array(do, np.int32), np.array(to, np.int32)
    ref = coco_ref.evaluate(db, dl, ds, do, tb, tl, np.concatenate(crowd_all), to, nc, image_sizes=sizes)
    ns, nk = n_averaged(ref, coco_ref.DEFAULT_STATS)
    assert list(out)[:12] == list(coco_ref.STAT_NAMES) and list(out["per_class_AP"]) == names[1:]
    assert (np.abs(np.array([out[k] for k in coco_ref.STAT_NAMES]) - ref["stats"]) <= ns * 2.0 ** -52).all()
    assert (np.abs(np.array(list(out["per_class_AP"].values())) - ref["per_class_ap"]) <= nk * 2.0 ** -52).all()
    assert 0 < out["AP"] < 1 and out["AR100"] > out["AR1"] > 0
    aps, m, tp, fp = ev.compute()
    ap_o, m_o, tp_o, fp_o, _ = map_ref.calculate_map(db, dl, ds, do, tb, tl, td, to, nc)
    assert list(tp.values()) == tp_o.tolist() and list(fp.values()) == fp_o.tolist() and abs(m - float(m_o)) < 1e-6
