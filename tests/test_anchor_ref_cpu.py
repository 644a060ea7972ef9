"""CPU: the numpy restatement of the anchor-fitting arithmetic (tests/anchor_ref.py) against answers worked by hand, against the
oracle's loss (the census reproduces get_target's positive count), and the convergence of every k-means input the GPU tests use.
Also: the argument errors of the mny_anchor_* entry points, which need no GPU."""
import numpy as np
import pytest
import torch

import anchor_cases as AC
import anchor_ref as R
import crowded_cases as CC
from oracle import procedural, yolo_ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- hand-worked ----------------------------------------------------------------------------------------------------------------
def test_four_boxes_two_centres_by_hand():
    wh = np.array([[10, 10], [12, 12], [100, 100], [120, 80]], F32)
    c0 = np.array([[10, 10], [100, 100]], F32)
    v = R.shape_iou(wh, c0)
    # (12,12) x (10,10): inter 100, union 144 + 100 - 100;  (120,80) x (100,100): inter 8000, union 9600 + 10000 - 8000
    assert v[0, 0] == F32(1.0) and v[1, 0] == F32(100) / F32(144) and v[3, 1] == F32(8000) / F32(11600) and v[3, 0] == F32(100) / F32(9600)
    lab, bv = R.best(wh, c0)
    assert lab.tolist() == [0, 0, 1, 1] and bv[2] == F32(1.0)
    c1 = R.kmeans_step(wh, c0)
    assert c1.tolist() == [[11.0, 11.0], [110.0, 90.0]]            # means of (10,12) and of (100,120) / (100,80): exact
    r = R.kmeans(wh, c0, 10, trace=True)
    # step 2 labels the same way and changes nothing
    assert r["state"].tolist() == [2, 1, 0, 0] and _bits(r["centres"]) == _bits(c1) and r["labels"].tolist() == [0, 0, 1, 1]
    assert r["best_iou"][0] == F32(100) / F32(121)


def test_shape_iou_is_find_jaccard_overlap_on_origin_boxes():
    """The specification's three-line shape IoU, the census's box IoU and the oracle's pair_iou (utils/iou.py:32-49) agree in every bit
    on valid shapes."""
    wh = AC._lognormal(2000, 90)
    a = AC._uniform(9, 91)
    v = R.shape_iou(wh, a)
    boxes = lambda s: torch.cat((torch.zeros(len(s), 2), torch.from_numpy(s)), 1)  # noqa: E731
    assert _bits(v) == _bits(yolo_ref.pair_iou(boxes(wh), boxes(a)).numpy())
    assert _bits(v) == _bits(np.stack([R._iou_ref(wh[:, 0], wh[:, 1], a[k, 0], a[k, 1]) for k in range(9)], 1))


def test_fixed_point_is_round_to_nearest_even():
    assert R.q([1.0, 2.0 ** -20, 65536.0]).tolist() == [2 ** 24, 16, 2 ** 40]
    assert R.q([F32(2.0 ** -25), F32(3 * 2.0 ** -25)]).tolist() == [0, 2]          # ties: 0.5 -> 0, 1.5 -> 2
    assert R.qi([1.0, 0.5, F32(2.0 ** -33), F32(3 * 2.0 ** -33)]).tolist() == [2 ** 32, 2 ** 31, 0, 2]


def test_exact_tie_goes_to_the_lower_index():
    wh = np.array([[4, 4]], F32)
    v = R.shape_iou(wh, [[2, 8], [8, 2], [4, 4]])
    assert v[0, 0] == v[0, 1] == F32(8) / F32(24) and v[0, 2] == 1
    assert R.best(wh, [[2, 8], [8, 2]])[0].tolist() == [0]
    assert R.best(wh, [[8, 2], [2, 8]])[0].tolist() == [0]
    assert R.best(wh, [[2, 8], [8, 2], [4, 4], [4, 4]])[0].tolist() == [2]


def test_empty_cluster_keeps_its_centre():
    wh = np.array([[10, 10], [12, 14], [9, 11]], F32)
    c = R.kmeans_step(wh, [[10, 10], [1000, 1000]])
    assert c[1].tolist() == [1000.0, 1000.0]
    s = R.q(wh).sum(0)
    assert _bits(c[0]) == _bits(((s.astype(np.float64) / 3.0) * 2.0 ** -24).astype(F32))
    r = R.kmeans(wh, [[10, 10], [1000, 1000]], 20)
    assert r["state"][1] == 1 and r["centres"][1].tolist() == [1000.0, 1000.0] and set(r["labels"].tolist()) == {0}


def test_skipped_boxes_take_part_in_nothing():
    good = np.array([[10, 10], [30, 30], [2.0 ** -20, 65536.0]], F32)
    bad = np.array([[0, 10], [-3, 10], [np.nan, 10], [10, np.inf], [1e6, 10], [2.0 ** -21, 10], [10, 65537]], F32)
    wh = np.concatenate((bad[:3], good, bad[3:]))
    assert R.valid(wh).tolist() == [False] * 3 + [True] * 3 + [False] * 4
    init = [[10, 10], [30, 30]]
    a, b = R.kmeans(wh, init, 5), R.kmeans(good, init, 5)
    assert _bits(a["centres"]) == _bits(b["centres"]) and a["state"].tolist() == [b["state"][0], 1, 7, 0] and b["state"][2] == 0
    assert a["labels"].tolist() == [-1] * 3 + b["labels"].tolist() + [-1] * 4
    assert a["best_iou"][[0, 1, 2, 6]].tolist() == [0, 0, 0, 0]
    fa, na = R.fitness(wh, [init], 0.0)
    fb, nb = R.fitness(good, [init], 0.0)
    assert na == nb == 3 and fa.tolist() == fb.tolist()


def test_fitness_at_a_threshold_equal_to_an_attained_iou():
    wh = np.array([[10, 10], [5, 10], [4, 4]], F32)
    cand = np.array([[[10, 10]], [[2, 8]]], F32)
    third = F32(8) / F32(24)                                         # (4,4) x (2,8)
    assert R.shape_iou(wh, cand[0])[:, 0].tolist() == [1.0, 0.5, float(F32(16) / F32(100))]
    fr, n = R.fitness(wh, cand, 0.5)                                 # strict >: the box at exactly 0.5 is out
    assert n == 3 and fr[0].tolist() == [2 ** 32, 1]
    fr, _ = R.fitness(wh, cand, np.nextafter(F32(0.5), F32(0)))
    assert fr[0].tolist() == [2 ** 32 + 2 ** 31, 2]
    fr, _ = R.fitness(wh, cand, 0.0)
    assert fr[0].tolist() == [2 ** 32 + 2 ** 31 + int(R.qi(F32(16) / F32(100))), 3]
    assert R.fitness(wh[2:], cand[1:], third)[0].tolist() == [[0, 0]]
    assert R.fitness(wh[2:], cand[1:], np.nextafter(third, F32(0)))[0].tolist() == [[int(R.qi(third)), 1]]


def test_evolution_keeps_the_parent_and_never_loses_fitness():
    wh, k, init = AC.kmeans_case("uniform-5000-k6")
    f = AC.draw_factors(3, 12, 8, k)
    a, hist, cands = R.evolve(wh, init, f, 0.25, 2.0)
    assert _bits(cands[0][0]) == _bits(init) and all(_bits(cands[g + 1][0]) == _bits(cands[g][hist[g, 1]]) for g in range(11))
    assert (np.diff(hist[:, 0]) >= 0).all() and hist[:, 0].max() > hist[0, 0] and _bits(a) == _bits(cands[-1][hist[-1, 1]])
    assert hist[0, 0] >= R.fitness(wh, [init], 0.25)[0][0, 0]


# ---- the census against the oracle's loss ---------------------------------------------------------------------------------------
def _census_of(tg, spec_cfg, img, grids):
    y = spec_cfg["yolo"]
    anchors = np.array([(aw / img, ah / img) for aw, ah in y["anchors"]]).astype(F32)
    packed = torch.cat([t.reshape(-1, 5) for t in tg]).numpy() if sum(len(t) for t in tg) else np.zeros((0, 5), F32)
    return R.census(packed, anchors, y["mask"], grids, y["iou_thresh"])


@pytest.mark.parametrize("case_id", sorted(CC.ALL))
def test_census_count_equals_the_oracle_loss_on_crowded_scenes(case_id):
    cfg_name, N, g, hi, _, _, _ = CC.ALL[case_id]
    spec, img, head, tg = CC.make(case_id)
    count_per_image = yolo_ref.loss_forward(head, tg, spec, [img, img], skip_outside=True)[6]
    grids = [g, g]
    c = _census_of(tg, CC.config(cfg_name), img, grids)
    assert int(c["pos"][hi].sum()) == round(count_per_image * N) and abs(count_per_image * N - round(count_per_image * N)) < 1e-6
    assert int(c["best"].sum()) == sum(len(t) for t in tg)


@pytest.mark.parametrize("hi,g", [(0, 11), (1, 22)])
def test_census_count_equals_the_oracle_loss_on_voc_both_heads(hi, g):
    spec = yolo_ref.specs_from_config(procedural.VOC_CONFIG)[hi]
    N = 6
    tg = procedural.targets(N, seed=40 + hi, empty_every=4, boxes_per_image=5)
    # two targets outside the grid (skipped) and one whose cy * g in (-1, 0) truncates to cell 0 (taken)
    tg[1] = torch.cat((tg[1], torch.tensor([[3.0, 1.02, 0.5, 0.2, 0.2], [4.0, 0.5, -0.2, 0.3, 0.1], [5.0, 0.5, -0.01, 0.3, 0.1]])))
    head = torch.randn(N, 75, g, g, generator=torch.Generator().manual_seed(hi)) * 0.5
    count = yolo_ref.loss_forward(head, tg, spec, [352, 352], skip_outside=True)[6] * N
    c = _census_of(tg, procedural.VOC_CONFIG, 352, [11, 22])
    assert int(c["pos"][hi].sum()) == round(count) and abs(count - round(count)) < 1e-6
    assert c["outside"].tolist() == [2, 2] and c["orphans"] == 2


def test_census_by_hand():
    # anchors (0.1,0.1) (0.2,0.2) (0.4,0.4) (0.8,0.8); heads {2,3} on a 2-grid and {0,1} on a 4-grid; iou_thresh 0.5
    a = np.array([[0.1, 0.1], [0.2, 0.2], [0.4, 0.4], [0.8, 0.8]], F32)
    t = np.array([[1, 0.5, 0.5, 0.1, 0.1],        # best 0: head 1 slot 0
                  [1, 0.3, 0.3, 0.16, 0.16],      # best 1 (0.64); anchor 0: 0.39 -> head 1 slot 1 only
                  [1, 0.7, 0.2, 0.3, 0.3],        # best 2 (0.5625); anchor 1: 0.444 -> head 0 slot 0
                  [1, 0.2, 0.9, 0.75, 0.75],      # best 3 (0.879) -> head 0 slot 1
                  [1, 1.0, 0.5, 0.1, 0.1],        # cx * g = g: outside both heads -> orphan
                  [1, 0.5, 0.5, 0.15, 0.15]],     # best 1 (0.5625), anchor 0: 0.444 -> head 1 slot 1
                 F32)
    c = R.census(t, a, [[2, 3], [0, 1]], [2, 4], 0.5)
    assert c["best"].tolist() == [2, 2, 1, 1] and c["pos"].tolist() == [[1, 1], [1, 2]] and c["orphans"] == 1 and c["outside"].tolist() == [1, 1]
    # a lower threshold lets the second anchor of a nested pair in: target 1 also hits anchor 0 (0.39), target 2 anchor 1 (0.444, in
    # head 1 beside its best anchor's head 0), target 5 anchor 0 (0.444)
    c = R.census(t, a, [[2, 3], [0, 1]], [2, 4], 0.38)
    assert c["pos"].tolist() == [[1, 1], [3, 3]] and c["orphans"] == 1


# ---- convergence: a condition on the inputs of the GPU trajectories ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AC.KMEANS))
def test_every_kmeans_input_converges_in_the_restatement(name):
    r = AC.kmeans_ref(name)
    print(name, "steps", int(r["state"][0]), "skipped", int(r["state"][2]))
    assert r["state"][1] == 1 and r["state"][0] <= AC.MAX_STEPS
    wh, k, init = AC.kmeans_case(name)
    assert _bits(R.kmeans_step(wh, r["centres"])) == _bits(r["centres"])      # a fixed point
    if name.startswith("empty-cluster"):
        assert _bits(r["centres"][2]) == _bits(init[2]) and 2 not in r["labels"]
    if name.startswith("identical"):
        assert set(r["labels"].tolist()) == {0} and r["state"][0] == 1
    if name.startswith("invalid"):
        assert r["state"][2] == 10 and (r["labels"] == -1).sum() == 10


# ---- argument errors need no GPU (tests/test_abi.py's style) ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def test_argument_errors_return_einval_without_a_launch(lib):
    L = lib.load()
    buf = (np.zeros(64, np.int64))
    p = buf.ctypes.data                                          # a 16-byte aligned host address: never dereferenced by a refused call
    p += -p % 16
    assert L.mny_anchor_ws_bytes(6, 64) >= 64 * 6 * 8 and L.mny_anchor_ws_bytes(0, 1) == 0 and L.mny_anchor_ws_bytes(33, 1) == 0
    assert L.mny_anchor_ws_bytes(6, 257) == 0 and b"outside" in L.mny_last_error()
    bad = [
        ("mny_anchor_kmeans", (p, 0, p, 6, 10, p, None, p, p, None), "N = 0"),
        ("mny_anchor_kmeans", (p, 2 ** 22 + 1, p, 6, 10, p, None, p, p, None), "N = "),
        ("mny_anchor_kmeans", (p, 100, p, 0, 10, p, None, p, p, None), "k = 0"),
        ("mny_anchor_kmeans", (p, 100, p, 33, 10, p, None, p, p, None), "k = 33"),
        ("mny_anchor_kmeans", (p, 100, p, 6, -1, p, None, p, p, None), "max_iter"),
        ("mny_anchor_kmeans", (None, 100, p, 6, 10, p, None, p, p, None), "null pointer"),
        ("mny_anchor_kmeans", (p, 100, p, 6, 10, None, None, p, p, None), "null pointer"),
        ("mny_anchor_kmeans", (p + 8, 100, p, 6, 10, p, None, p, p, None), "16-byte"),
        ("mny_anchor_fitness", (p, 100, p, 0, 6, 0.25, p, p, None), "P = 0"),
        ("mny_anchor_fitness", (p, 100, p, 257, 6, 0.25, p, p, None), "P = 257"),
        ("mny_anchor_fitness", (p, 100, None, 8, 6, 0.25, p, p, None), "null pointer"),
        ("mny_anchor_fitness", (p, 100, p, 8, 6, float("nan"), p, p, None), "NaN"),
        ("mny_anchor_evolve", (p, 100, p, 6, p, 0, 8, 0.25, 2.0, p, p, p, None), "G = 0"),
        ("mny_anchor_evolve", (p, 100, p, 6, None, 5, 8, 0.25, 2.0, p, p, p, None), "null pointer"),
        ("mny_anchor_evolve", (p, 100, p, 6, p, 5, 8, 0.25, 0.0, p, p, p, None), "min_size"),
        ("mny_anchor_census", (p, 10, p, 0, p, p, 2, 3, 0.5, p, None), "anchors outside"),
        ("mny_anchor_census", (p, 10, p, 6, p, p, 5, 3, 0.5, p, None), "heads"),
        ("mny_anchor_census", (p, -1, p, 6, p, p, 2, 3, 0.5, p, None), "T = -1"),
        ("mny_anchor_census", (None, 10, p, 6, p, p, 2, 3, 0.5, p, None), "null pointer"),
    ]
    for name, args, msg in bad:
        assert getattr(L, name)(*args) == -1, (name, msg)                     # MNY_EINVAL
        assert msg.encode() in L.mny_last_error(), (name, msg, L.mny_last_error())
        with pytest.raises(lib.MnyError, match=name):
            lib.call(name, *args)
    # mask and grids are host arrays, checked before any launch
    mask, grids = np.array([[0, 1, 2], [3, 4, 6]], np.int32), np.array([11, 22], np.int32)
    hp = lambda a: a.ctypes.data  # noqa: E731
    assert L.mny_anchor_census(p, 10, p, 6, hp(mask), hp(grids), 2, 3, 0.5, p, None) == -1 and b"names none" in L.mny_last_error()
    mask[1, 2], grids[1] = 5, 0
    assert L.mny_anchor_census(p, 10, p, 6, hp(mask), hp(grids), 2, 3, 0.5, p, None) == -1 and b"grid 0" in L.mny_last_error()


def test_python_interface_refuses_host_tensors_and_bad_shapes():
    from mobilenet_yolo_pytorch_amd import anchors
    with pytest.raises(RuntimeError, match="CUDA"):
        anchors.kmeans(torch.ones(10, 2), 3)
    with pytest.raises(ValueError, match=r"\[N,2\]"):
        anchors.fitness(torch.ones(10, 3), torch.ones(3, 2))
    f = anchors.draw_factors(0, 4, 5, 6)
    assert f.shape == (4, 5, 6, 2) and f.dtype == np.float32 and f.min() >= F32(0.3) and f.max() <= 3 and (f == 1).mean() > 0.05
    assert _bits(f) == _bits(AC.draw_factors(0, 4, 5, 6)) and _bits(f) == _bits(anchors.draw_factors(0, 4, 5, 6)) != _bits(anchors.draw_factors(1, 4, 5, 6))
