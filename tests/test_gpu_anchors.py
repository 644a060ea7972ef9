"""Anchor fitting on the GPU (csrc/anchors.hip through mobilenet_yolo_pytorch_amd.anchors) against the numpy restatement
tests/anchor_ref.py, BIT FOR BIT: labels, centres after every single step and at the end, state, F, R, history, final anchors and the
census arrays.  The fp32 operations are IEEE on both sides and every reduction is an integer, so there is no tolerance anywhere in this
file; a test that needs a margin has found a bug.  The census is also cross-checked with the hot path: the positive count of
mny_yolo_loss.  Inputs: tests/anchor_cases.py (their convergence in the restatement is asserted by tests/test_anchor_ref_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import anchor_cases as AC
import anchor_ref as R
import crowded_cases as CC
from oracle import procedural, yolo_ref

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def anchors():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import anchors as a
    return a


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the shared cases are read-only


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _same(got, want, what):
    """Equal in shape, type and every bit (a NaN equals the same NaN, -0 does not equal 0)."""
    g = np.ascontiguousarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got).reshape(-1)
    w = np.ascontiguousarray(want).reshape(-1)
    assert tuple(got.shape) == tuple(np.shape(want)) and g.dtype == w.dtype, (what, tuple(got.shape), np.shape(want), g.dtype, w.dtype)
    bad = np.flatnonzero(g.view("u%d" % g.itemsize) != w.view("u%d" % w.itemsize))
    assert len(bad) == 0, "%s: %d of %d differ, first at %d: %r != %r" % (what, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]])


# ---- k-means --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.KMEANS))
def test_kmeans_every_step_and_the_run(anchors, name):
    wh, k, init = AC.kmeans_case(name)
    ref = AC.kmeans_ref(name)
    steps = int(ref["state"][0])
    d = _dev(wh)
    # one step at a time, from the centres the previous step left
    c = _dev(init)
    for i in range(steps):
        c, st = anchors.kmeans(d, k, init=c, max_iter=1)
        _same(c, ref["trace"][i], "%s: centres after step %d" % (name, i + 1))
    assert st.tolist() == [1, 1, int(ref["state"][2]), 0]               # the last step changed nothing
    # the whole run, queued without a host synchronisation; the steps after convergence must leave the same result
    c, st, lab, best = anchors.kmeans(d, k, init=_dev(init), max_iter=AC.MAX_STEPS, with_labels=True)
    _same(c, ref["centres"], name + ": centres")
    _same(st, ref["state"], name + ": state")
    _same(lab, ref["labels"], name + ": labels")
    _same(best, ref["best_iou"], name + ": best_iou")
    # fixed point: one more step changes nothing
    c2, st2 = anchors.kmeans(d, k, init=c, max_iter=1)
    _same(c2, ref["centres"], name + ": one more step")
    assert st2.tolist()[:2] == [1, 1]
    # stopped short of convergence: exactly the trace, not converged
    if steps > 2:
        c3, st3 = anchors.kmeans(d, k, init=_dev(init), max_iter=steps - 2)
        _same(c3, ref["trace"][steps - 3], name + ": stopped early")
        assert st3.tolist()[:2] == [steps - 2, 0]


def test_kmeans_default_init_is_the_quantile_rule(anchors):
    for name in ("invalid-300-k6", "int-1000-k6", "n65-k32"):           # the integer set has equal areas: the sort must be stable
        wh, k, _ = AC.kmeans_case(name)
        _same(anchors.default_init(_dev(wh), k), R.default_init(wh, k), name)
    wh, k, init = AC.kmeans_case("int-1000-k6")
    _same(anchors.kmeans(_dev(wh), k, max_iter=AC.MAX_STEPS)[0], AC.kmeans_ref("int-1000-k6")["centres"], "default init run")


def test_kmeans_zero_steps_only_labels(anchors):
    wh, k, init = AC.kmeans_case("invalid-300-k6")
    c, st, lab, best = anchors.kmeans(_dev(wh), k, init=_dev(init), max_iter=0, with_labels=True)
    r = R.kmeans(wh, init, 0)
    _same(c, init, "centres")
    _same(st, r["state"], "state")
    _same(lab, r["labels"], "labels")
    _same(best, r["best_iou"], "best_iou")


# ---- fitness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.FITNESS))
def test_fitness_counts(anchors, name):
    maker, n, seed, P, k = AC.FITNESS[name]
    wh = maker(n, seed)
    cand = AC.candidates(wh, P, k, seed)
    d, dc = _dev(wh), _dev(cand)
    for thr in (0.25, 0.0):
        want, nvalid = R.fitness(wh, cand, thr)
        fr, valid = anchors.fitness_counts(d, dc, thr)
        _same(fr, want, "%s thr %g: F, R" % (name, thr))
        assert valid.tolist() == [nvalid]
        if P > 8:
            break                                                       # the wide cases once
    mean, rec = anchors.fitness(d, dc, 0.25)
    want, nvalid = R.fitness(wh, cand, 0.25)
    _same(mean, want[:, 0].astype(np.float64) * 2.0 ** -32 / nvalid, name + ": mean best IoU")
    _same(rec, want[:, 1].astype(np.float64) / nvalid, name + ": recall")


def test_fitness_threshold_equal_to_an_attained_iou(anchors):
    wh = np.array([[10, 10], [5, 10], [4, 4]], F32)
    cand = np.array([[[10, 10]], [[2, 8]]], F32)
    for thr in (F32(0.5), np.nextafter(F32(0.5), F32(0)), F32(8) / F32(24), np.nextafter(F32(8) / F32(24), F32(0)), F32(1.0)):
        _same(anchors.fitness_counts(_dev(wh), _dev(cand), float(thr))[0], R.fitness(wh, cand, thr)[0], "thr %r" % thr)
    assert anchors.fitness_counts(_dev(wh), _dev(cand), 0.5)[0].tolist()[0] == [2 ** 32, 1]


def test_one_kmeans_step_past_the_grid_stride(anchors):
    maker, n, seed, P, k = AC.FITNESS["n600001-p1-k6"]
    wh = maker(n, seed)
    init = R.default_init(wh, k)
    c, st = anchors.kmeans(_dev(wh), k, init=_dev(init), max_iter=1)
    _same(c, R.kmeans_step(wh, init), "centres after one step, 586 tiles on 512 workgroups")


# ---- evolution --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.EVOLVE))
def test_evolve(anchors, name):
    maker, n, seed, P, k = AC.EVOLVE[name]
    wh = maker(n, seed)
    parent = R.default_init(wh, k)
    factors = AC.draw_factors(seed, AC.G, P, k)
    thr, min_size = 0.25, 2.0
    want, hist, cands = R.evolve(wh, parent, factors, thr, min_size)
    got, h = anchors.evolve(_dev(wh), _dev(parent), AC.G, P, thr, min_size=min_size, factors=factors)
    _same(h, hist, name + ": history")
    _same(got, want, name + ": anchors")
    hh = h.cpu().numpy()
    assert (np.diff(hh[:, 0]) >= 0).all(), "F decreased"
    # candidate 0 is the parent verbatim: generation 0's parent scores what the fitness entry gives it, and never less is kept
    f0 = anchors.fitness_counts(_dev(wh), _dev(parent), thr)[0].tolist()[0][0]
    assert hh[0, 0] >= f0 and (hh[0, 1] != 0 or hh[0, 0] == f0)
    assert anchors.fitness_counts(_dev(wh), got, thr)[0].tolist()[0][0] == hh[-1, 0]
    if P == 1:
        _same(got, parent, "P = 1 keeps the parent")
        assert (hh[:, 1] == 0).all()
    # the same draw through the public seed argument
    got2, h2 = anchors.evolve(_dev(wh), _dev(parent), AC.G, P, thr, seed=seed, min_size=min_size)
    assert _bits(got2) == _bits(got) and _bits(h2) == _bits(h)


def test_evolve_min_size_clamps(anchors):
    wh = AC._uniform(257, 50)
    parent = np.array([[2.5, 2.5], [100, 100]], F32)
    factors = np.full((3, 4, 2, 2), 0.5, F32)
    want, hist, _ = R.evolve(wh, parent, factors, 0.0, 2.0)
    got, h = anchors.evolve(_dev(wh), _dev(parent), 3, 4, 0.0, min_size=2.0, factors=factors)
    _same(got, want, "anchors")
    _same(h, hist, "history")
    assert got.min().item() >= 2.0


# ---- census ---------------------------------------------------------------------------------------------------------------------
def _loss_count(head_nchw, tg, spec, img):
    from mobilenet_yolo_pytorch_amd import ops
    N, _, g, _ = head_nchw.shape
    anchors_all = torch.tensor([(aw / img, ah / img) for aw, ah in spec.anchors], dtype=torch.float32).cuda()
    mask = torch.tensor(spec.mask, dtype=torch.int32).cuda()
    hp = ops.make_head(N, g, len(spec.mask), spec.num_classes, len(spec.anchors), spec.ignore_thresh, spec.iou_thresh, spec.iou_weighting)
    off = np.zeros(N + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in tg])
    allt = torch.cat([t.reshape(-1, 5) for t in tg]) if off[-1] else torch.zeros(1, 5)
    out7, _ = ops.yolo_loss(head_nchw.permute(0, 2, 3, 1).contiguous().cuda(), allt.float().contiguous().cuda(), torch.from_numpy(off).cuda(),
                            anchors_all, mask, hp)
    v = float(out7[6].cpu()) * N                      # out7[6] = count / N in fp32: the integer is recovered by rounding
    assert abs(v - round(v)) < 1e-3 * max(1.0, v)
    return round(v)


def _census_both(anchors, tg, cfg, img, grids):
    y = cfg["yolo"]
    got = anchors.census(tg, y["anchors"], y["mask"], y["iou_thresh"], [img, img], grids)
    packed = torch.cat([t.reshape(-1, 5) for t in tg]).numpy() if sum(len(t) for t in tg) else np.zeros((0, 5), F32)
    a = np.array([(aw / img, ah / img) for aw, ah in y["anchors"]]).astype(F32)
    want = R.census(packed, a, y["mask"], grids, y["iou_thresh"])
    for key in ("best", "pos", "outside"):
        _same(got[key], want[key], "census " + key)
    assert got["orphans"].tolist() == [int(want["orphans"])]
    return got


@pytest.mark.parametrize("case_id", sorted(CC.ALL))
def test_census_equals_the_loss_kernel_on_crowded_scenes(anchors, case_id):
    cfg_name, N, g, hi, _, _, _ = CC.ALL[case_id]
    spec, img, head, tg = CC.make(case_id)
    got = _census_both(anchors, tg, CC.config(cfg_name), img, [g, g])
    assert int(got["pos"][hi].sum()) == _loss_count(head, tg, spec, img)


@pytest.mark.parametrize("seed", [0, 1])
def test_census_equals_the_loss_kernel_on_random_heads_both_heads(anchors, seed):
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    N = 16
    tg = procedural.targets(N, seed=60 + seed, empty_every=5, boxes_per_image=4 + seed)
    tg[2] = torch.cat((tg[2], torch.tensor([[3.0, 1.02, 0.5, 0.2, 0.2], [4.0, 0.5, -0.2, 0.3, 0.1], [5.0, 0.5, -0.01, 0.3, 0.1]])))
    got = _census_both(anchors, tg, procedural.VOC_CONFIG, 352, [11, 22])
    assert got["outside"].tolist() == [2, 2]
    for hi, g in ((0, 11), (1, 22)):
        head = torch.randn(N, 75, g, g, generator=torch.Generator().manual_seed(seed)) * 0.7
        assert int(got["pos"][hi].sum()) == _loss_count(head, tg, specs[hi], 352)


def test_census_of_no_targets_and_of_device_anchors(anchors):
    y = procedural.VOC_CONFIG["yolo"]
    got = anchors.census([torch.zeros(0, 5)], y["anchors"], y["mask"], y["iou_thresh"], 352, [11, 22])
    assert all(int(v.sum()) == 0 for v in got.values())
    tg = procedural.targets(8, seed=70, empty_every=0, boxes_per_image=9)
    a = anchors.census(tg, y["anchors"], y["mask"], y["iou_thresh"], 352, [11, 22])
    b = anchors.census(torch.cat(tg).cuda(), torch.tensor(y["anchors"], dtype=torch.float32).cuda(), y["mask"], y["iou_thresh"], 352, [11, 22])
    assert all(_bits(a[key]) == _bits(b[key]) for key in a)


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_autoanchor_report_and_invariants(anchors):
    cfg = procedural.VOC_CONFIG
    tg = procedural.targets(64, seed=80, empty_every=16, boxes_per_image=6)
    fit = anchors.autoanchor(tg, cfg, generations=30, population=16, seed=1)
    rep = fit["report"]
    k = len(cfg["yolo"]["anchors"])
    assert fit["mask"] == [[0, 1, 2], [3, 4, 5]] and len(fit["anchors"]) == k and all(isinstance(v, int) and v >= 1 for a in fit["anchors"] for v in a)
    areas = [w * h for w, h in fit["anchors"]]
    assert areas == sorted(areas, reverse=True)
    assert rep["boxes"] == sum(len(t) for t in tg) and rep["skipped"] == 0 and rep["kmeans_converged"]
    assert rep["evolved"]["fitness"] >= rep["kmeans"]["fitness"]              # evolution's invariant
    assert rep["before"]["anchors"] == [[float(w), float(h)] for w, h in cfg["yolo"]["anchors"]]
    # every stage's figures are what the pieces give for its anchors
    wh = anchors.wh_from_targets(tg, cfg["img_w"])
    _same(wh, (torch.cat(tg).numpy()[:, 3:5] * F32(352)).astype(F32), "wh_from_targets")
    for stage in ("before", "kmeans", "evolved", "rounded"):
        a = np.array(rep[stage]["anchors"], F32)
        fr, n = R.fitness(wh.cpu().numpy(), a[None], 0.25)
        assert rep[stage]["fitness"] == float(fr[0, 0]) * 2.0 ** -32 / n and rep[stage]["recall"] == fr[0, 1] / n
        assert sum(rep[stage]["best"]) == rep["boxes"] and rep[stage]["outside"] == [0, 0]
    assert rep["rounded"]["anchors"] == [[float(w), float(h)] for w, h in fit["anchors"]]
    # the result drops into the config and the model takes it
    from mobilenet_yolo_pytorch_amd import yolo
    cfg2 = dict(cfg, yolo=dict(cfg["yolo"], anchors=fit["anchors"], mask=fit["mask"]))
    assert yolo(cfg2).yolo_losses[0].anchors == [tuple(a) for a in fit["anchors"]]


def test_argument_errors_do_not_launch(anchors):
    from mobilenet_yolo_pytorch_amd import _lib
    wh = _dev(AC._uniform(64, 0))
    with pytest.raises(_lib.MnyError, match="P = 257"):
        anchors.fitness_counts(wh, torch.ones(257, 3, 2).cuda())
    with pytest.raises(_lib.MnyError, match="k = 33"):
        anchors.fitness_counts(wh, torch.ones(2, 33, 2).cuda())
    with pytest.raises(_lib.MnyError, match="min_size"):
        anchors.evolve(wh, torch.ones(3, 2).cuda() * 20, 2, 4, min_size=0.0)
    with pytest.raises(_lib.MnyError, match="names none"):
        anchors.census([torch.tensor([[1.0, 0.5, 0.5, 0.1, 0.1]])], [[10, 10], [20, 20]], [[0], [2]], 0.5, 352, [11, 22])
    torch.cuda.synchronize()
    assert ctypes.c_int(_lib.load().mny_version()).value == 100
