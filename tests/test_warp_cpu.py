"""CPU: the host half of the random-perspective stage (augment.RandomPerspective: draws, matrices, records, boxes, validation; the
TrainAugment wiring) against tests/warp_ref.py.  No GPU; the library is only asked for its argument errors."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest

import warp_ref as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


@pytest.fixture(scope="module")
def M():
    from mobilenet_yolo_pytorch_amd import augment
    return augment


def mixed_sizes(n, seed=0):
    r = np.random.RandomState(seed)
    return [(int(r.randint(1, 400)), int(r.randint(1, 400))) for _ in range(n)]


FULL = dict(degrees=10.0, translate=0.1, scale=0.5, shear=5.0, perspective=2e-4, p=0.8)


def test_plan_is_a_function_of_the_seed_and_the_batch_size(M):
    sizes = mixed_sizes(300)
    a, b, c = (M.RandomPerspective(seed, device="cpu", **FULL).plan(sizes) for seed in (5, 5, 6))
    assert a["records"].dtype == M.WARP and a["records"].tobytes() == b["records"].tobytes() != c["records"].tobytes()
    assert np.array_equal(a["matrices"], b["matrices"]) and np.array_equal(a["identity"], b["identity"])
    s = M.RandomPerspective(5, device="cpu", **FULL)
    first, second = s.plan(sizes), s.plan(sizes)                    # the generator advances from batch to batch
    assert first["records"].tobytes() == a["records"].tobytes() != second["records"].tobytes()
    # the draws do not depend on the image sizes, only on how many there are
    d0, d1 = M.RandomPerspective(5, device="cpu", **FULL).draw(300), M.RandomPerspective(5, device="cpu", **FULL).draw(300)
    assert all(np.array_equal(d0[k], d1[k]) for k in d0)
    other = M.RandomPerspective(5, device="cpu", **FULL).plan(mixed_sizes(300, seed=1))
    assert np.array_equal(other["identity"], a["identity"])


def test_plan_never_touches_python_random(M):
    random.seed(1234)
    state = random.getstate()
    M.RandomPerspective(1, device="cpu", **FULL).plan(mixed_sizes(200))
    M.RandomPerspective(device="cpu").plan([(5, 5)])
    assert random.getstate() == state


def test_defaults_are_hyp_scratch_low(M):
    w = M.RandomPerspective(0, device="cpu")
    assert (w.degrees, w.translate, w.scale, w.shear, w.perspective, w.p) == (0.0, 0.1, 0.5, 0.0, 0.0, 1.0)
    p = w.plan(mixed_sizes(50))
    assert not p["identity"].any()
    assert np.all(p["records"]["c"][:, 6:] == 0) and np.all(p["records"]["c"][:, [1, 3]] == 0)     # scale and translation only
    assert np.all(p["records"]["fill"] == 127) and np.all(p["records"]["reserved"] == 0)


def test_draw_order_ranges_and_gate(M):
    w = M.RandomPerspective(11, device="cpu", **FULL)
    d = w.draw(N)
    assert list(d) == ["gate", "a", "s", "shx", "shy", "tx", "ty", "px", "py"]
    k = int(d["gate"].sum())
    assert abs(k - N * 0.8) <= 5 * math.sqrt(N * 0.8 * 0.2)
    for name, lo, hi in (("a", -10, 10), ("s", 0.5, 1.5), ("shx", -5, 5), ("shy", -5, 5), ("tx", 0.4, 0.6), ("ty", 0.4, 0.6), ("px", -2e-4, 2e-4),
                         ("py", -2e-4, 2e-4)):
        v = d[name]
        assert v.shape == (N,) and lo <= v.min() and v.max() <= hi, name
        assert v.min() < lo + 0.01 * (hi - lo) and v.max() > hi - 0.01 * (hi - lo), name        # and the range is used
        assert abs(v.mean() - (lo + hi) / 2) < 0.02 * (hi - lo), name
    # the same stream, drawn by hand in the documented order
    g = np.random.Generator(np.random.PCG64(11))
    assert np.array_equal(d["gate"], g.random(N) < 0.8) and np.array_equal(d["a"], g.uniform(-10, 10, N)) and np.array_equal(d["s"], g.uniform(0.5, 1.5, N))


def test_records_follow_the_draws(M):
    sizes = mixed_sizes(64, seed=3)
    w = M.RandomPerspective(7, device="cpu", **FULL)
    d = M.RandomPerspective(7, device="cpu", **FULL).draw(len(sizes))
    p = w.plan(sizes)
    assert 0 < p["identity"].sum() < len(sizes) and np.array_equal(p["identity"], ~d["gate"])
    assert np.array_equal(p["records"]["identity"] != 0, p["identity"])
    for i, (h, wd) in enumerate(sizes):
        if p["identity"][i]:
            assert np.array_equal(p["matrices"][i], np.eye(3)) and tuple(p["records"]["c"][i]) == W.IDENTITY_C
            continue
        ref = W.matrix(h, wd, d["a"][i], d["s"][i], d["shx"][i], d["shy"][i], d["tx"][i], d["ty"][i], d["px"][i], d["py"][i])
        assert np.array_equal(p["matrices"][i], ref)
        assert np.array_equal(p["records"]["c"][i], W.coeffs(ref))


def test_zero_parameters_give_identity_items(M):
    w = M.RandomPerspective(3, degrees=0, translate=0, scale=0, shear=0, perspective=0, device="cpu")
    p = w.plan(mixed_sizes(100, seed=4))
    assert p["identity"].all() and np.all(p["matrices"] == np.eye(3))


def test_struct_size_matches_the_header(M):
    src = open(os.path.join(REPO, "include", "mnyolo.h")).read()
    m = re.search(r"\}\s*mny_aug_warp_item;\s*/\*\s*(\d+) bytes\s*\*/", src)
    assert m and int(m.group(1)) == M.WARP.itemsize == 72
    body = re.sub(r"/\*.*?\*/", "", src[src.index("typedef struct mny_aug_warp_item"):m.start()], flags=re.S)
    fields = re.findall(r"\b(?:double|int32_t|uint8_t)\s+([^;]+);", body)
    names = [re.sub(r"\[\d+\]", "", n).strip() for f in fields for n in f.split(",")]
    assert names == list(M.WARP.names)
    assert [M.WARP.fields[n][1] for n in M.WARP.names] == [0, 64, 68, 71]


def test_fixed_validation(M):
    ok = W.matrix(40, 60, degrees=20.0, scale=0.9)
    p = M.RandomPerspective.fixed([ok, np.eye(3)], device="cpu").plan([(40, 60), (8, 8)])
    assert p["identity"].tolist() == [False, True] and np.array_equal(p["records"]["c"][0], W.coeffs(ok))
    with pytest.raises(ValueError, match="image 1"):
        M.RandomPerspective.fixed([ok, np.zeros((3, 3))], device="cpu")                    # singular
    bad = ok.copy()
    bad[0, 1] = np.nan
    with pytest.raises(ValueError, match="image 0"):
        M.RandomPerspective.fixed([bad], device="cpu")
    with pytest.raises(ValueError, match="2 images"):
        M.RandomPerspective.fixed([ok, ok], device="cpu").plan([(40, 60)])


def test_source_corner_denominator_is_checked_by_name(M):
    m = W.matrix(100, 100, px=0.03)                                  # den = 0.03 (x - 50) + 1: negative at x = 0
    with pytest.raises(ValueError, match="image 2"):
        M.RandomPerspective.fixed([np.eye(3), np.eye(3), m], device="cpu").plan([(100, 100)] * 3)
    m = W.matrix(20, 20, px=0.03)                                    # sound on a small image: den 0.7 .. 1.3
    M.RandomPerspective.fixed([m], device="cpu").plan([(20, 20)])
    with pytest.raises(ValueError, match="image 0"):
        M.RandomPerspective(1, perspective=0.5, device="cpu").plan([(375, 500)])      # |px| * 250 + |py| * 187.5 > 1 for this seed


def test_boxes_equal_the_restatement(M):
    r = np.random.RandomState(8)
    seen_drop = seen_keep = 0
    for k in range(60):
        h, w = int(r.randint(30, 400)), int(r.randint(30, 400))
        mat = W.matrix(h, w, r.uniform(-30, 30), r.uniform(0.3, 1.7), r.uniform(-10, 10), r.uniform(-10, 10), r.uniform(0.2, 0.8), r.uniform(0.2, 0.8),
                       r.uniform(-1, 1) * 0.3 / w, r.uniform(-1, 1) * 0.3 / h)
        n = int(r.randint(0, 6))
        t = np.concatenate([r.randint(0, 20, (n, 1)), r.uniform(0.1, 0.9, (n, 2)), r.uniform(0.005, 0.5, (n, 2))], 1).astype(np.float32)
        got, want = M.RandomPerspective.boxes(t, mat, h, w), W.boxes(t, mat, h, w)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), k
        seen_drop += n - len(got)
        seen_keep += len(got)
    assert seen_drop > 10 and seen_keep > 10


def small_groups():
    from mobilenet_yolo_pytorch_amd import synthetic
    shapes = [(60, 67), (48, 50), (64, 40), (33, 61), (50, 50), (64, 64), (41, 57)]
    tg = [t.numpy() for t in synthetic.targets(len(shapes), seed=3, boxes_per_image=2)]
    return shapes, tg, [[(shapes[0], tg[0])], [(shapes[1], tg[1])], [(s, t) for s, t in zip(shapes[2:6], tg[2:6])], [(shapes[6], tg[6])]]


def test_train_augment_plan_with_an_all_identity_warp_is_that_of_none(M):
    _, _, groups = small_groups()
    outs = []
    for warp in (None, M.RandomPerspective(2, degrees=0, translate=0, scale=0, shear=0, perspective=0, device="cpu"),
                 M.RandomPerspective(2, p=0.0, device="cpu", **{k: v for k, v in FULL.items() if k != "p"})):
        rng = random.Random(9)
        p = M.TrainAugment([[32, 32], [64, 64]], [0.5] * 3, [1.0] * 3, 1.5, device="cpu", rng=rng, warp=warp).plan(groups)
        outs.append((p, rng.getstate()))
    for p1, s1 in outs[1:]:
        p0, s0 = outs[0]
        assert s0 == s1 and p0["items"].tobytes() == p1["items"].tobytes() and p0["samples"].tobytes() == p1["samples"].tobytes()
        assert p0["count"] == p1["count"] == 7 and p0["size"] == p1["size"]
        assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(p0["targets"], p1["targets"]))
        assert "warp" not in p0 and p1["warp"]["identity"].all()


def test_train_augment_plan_transforms_the_targets_first(M):
    """The plan of a warped batch is the plan of warp=None fed with the restatement's boxes: same items, same draws."""
    shapes, tg, groups = small_groups()
    mats = [W.matrix(h, w, 15.0 * (i - 3), 0.8 + 0.1 * i, 3.0, -2.0, 0.45 + 0.02 * i, 0.52, 1e-3 / w, -1e-3 / h) for i, (h, w) in enumerate(shapes)]
    mats[1] = np.eye(3)
    moved = [t if i == 1 else W.boxes(t, mats[i], *shapes[i]) for i, t in enumerate(tg)]
    assert any(len(a) != len(b) for a, b in zip(moved, tg)) or any(not np.array_equal(a, b) for a, b in zip(moved, tg))
    want_groups = [[(shapes[0], moved[0])], [(shapes[1], moved[1])], [(s, t) for s, t in zip(shapes[2:6], moved[2:6])], [(shapes[6], moved[6])]]
    r0, r1 = random.Random(4), random.Random(4)
    p1 = M.TrainAugment([[32, 32]], [0.5] * 3, [1.0] * 3, 1.5, device="cpu", rng=r1, warp=M.RandomPerspective.fixed(mats, device="cpu")).plan(groups)
    p0 = M.TrainAugment([[32, 32]], [0.5] * 3, [1.0] * 3, 1.5, device="cpu", rng=r0).plan(want_groups)
    assert r0.getstate() == r1.getstate() and p0["items"].tobytes() == p1["items"].tobytes()
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(p0["targets"], p1["targets"]))
    assert p1["warp"]["identity"].tolist() == [False, True] + [False] * 5


def test_from_config_takes_warp(M):
    cfg = dict(train_img_size=[[32, 32]], normalize=dict(mean=[0.5] * 3, std=[1.0] * 3), expand_scale=1.5)
    w = M.RandomPerspective(0, device="cpu")
    assert M.TrainAugment.from_config(cfg, device="cpu", warp=w).warp is w and M.TrainAugment.from_config(cfg, device="cpu").warp is None


def test_argument_errors_do_not_need_a_gpu(M):
    from mobilenet_yolo_pytorch_amd._lib import MnyError, call, query
    assert query("mny_aug_warp_ws_bytes", 4, 3, 8, 8) >= 4 and query("mny_aug_warp_ws_bytes", 4, 1, 8, 8) >= 4
    assert query("mny_aug_warp_ws_bytes", 0, 3, 8, 8) == 0 and query("mny_aug_warp_ws_bytes", 4097, 3, 8, 8) == 0
    assert query("mny_aug_warp_ws_bytes", 4, 2, 8, 8) == 0 and query("mny_aug_warp_ws_bytes", 4, 3, 0, 8) == 0
    assert query("mny_aug_warp_ws_bytes", 4, 3, 8, 16384) == 0
    buf = (ctypes.c_uint8 * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 8
    p = lambda o=0: ctypes.c_void_p(base + o)
    with pytest.raises(MnyError, match="null pointer"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 3, 8, 8, None, p(256), None)
    with pytest.raises(MnyError, match="dst must not be src"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 3, 8, 8, p(), p(256), None)
    with pytest.raises(MnyError, match="aligned"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 3, 8, 8, p(130), p(256), None)
    with pytest.raises(MnyError, match="channels"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 2, 8, 8, p(128), p(256), None)
    with pytest.raises(MnyError, match="bad sizes"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 0, 3, 8, 8, p(128), p(256), None)


def test_run_device_refuses_a_plan_of_the_wrong_shape(M):
    import torch
    from mobilenet_yolo_pytorch_amd.prep import DESC
    w = M.RandomPerspective(0, device="cpu")
    plan = w.plan([(4, 4), (4, 4)])
    src = torch.zeros(128, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one WARP record per image"):
        w.run_device(src, np.zeros(3, DESC), plan)
    with pytest.raises(ValueError, match="channels"):
        w.run_device(src, np.zeros(2, DESC), plan, channels=2)
