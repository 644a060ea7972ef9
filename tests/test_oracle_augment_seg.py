"""CPU: the seg-map restatement (tests/augment_seg_ref.py) against the REAL reference's id maps (tests/golden/augseg_*.npz,
tools/gen_golden_augment_seg.py), its area resize against an exact fp64 area average, and the host half of
TrainAugment(seg_classes=...): same plan as a plain instance, and the refusals."""
import glob
import json
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as A
import augment_seg_ref as S

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "augseg_*.npz")))


def load(name):
    z = np.load(os.path.join(G, name))
    n = int(z["count"])
    return z, [[(z["img%d" % i], z["tgt%d" % i], z["seg%d" % i])] for i in range(n)]


def test_fixtures_present_and_cover_the_cases():
    assert FIXTURES == ["augseg_a.npz", "augseg_b.npz"]
    seen = set()
    for name in FIXTURES:
        z, groups = load(name)
        for (im, t, sg), in groups:
            assert sg.dtype == np.uint8 and sg.shape == im.shape[:2]
            seen.update(int(v) for v in np.unique(sg))
        samples, _, _ = A.plan(random.Random(int(z["seed"])), [[(im.shape[0], im.shape[1], t)] for (im, t, _), in groups],
                               float(z["expand_scale"]), 1000, z["sizes"].tolist())
        for s in samples:
            m = s["members"][0]
            seen.update(k for k, v in (("expand", m["expand"]), ("crop", m["crop"]), ("flip", m["flip"])) if v)
            seen.update(["nocrop"] if m["crop"] is None else [])
    assert {0, 1, 2, 3, "expand", "crop", "nocrop", "flip"} <= seen, seen
    assert int(np.load(os.path.join(G, "augseg_a.npz"))["seg_classes"]) == 2        # so id 3 lies above its classes


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_geometry_reproduces_reference(name):
    z, groups = load(name)
    rng = random.Random(int(z["seed"]))
    samples, size, count = A.plan(rng, [[(im.shape[0], im.shape[1], t)] for (im, t, _), in groups], float(z["expand_scale"]), 1000, z["sizes"].tolist())
    assert np.array_equal(np.array([rng.random() for _ in range(4)]), z["after"])             # the seg path makes no draw
    assert tuple(size) == tuple(z["size"]) and count == int(z["count"])
    for i, (g, s) in enumerate(zip(groups, samples)):
        m = s["members"][0]
        got = S.geometry(g[0][2], m["expand"], m["crop"], m["flip"])
        assert got.dtype == np.uint8 and got.shape == z["new_seg%d" % i].shape == m["geo"] and np.array_equal(got, z["new_seg%d" % i]), i
        assert np.array_equal(s["target"].numpy(), z["out_tgt%d" % i]), i


@pytest.mark.parametrize("name", FIXTURES)
def test_seg_plan_equals_plain_plan(name):
    from mobilenet_yolo_pytorch_amd import augment
    z, groups = load(name)
    kw = dict(device="cpu")
    r1, r2 = random.Random(int(z["seed"])), random.Random(int(z["seed"]))
    seg = augment.TrainAugment(z["sizes"].tolist(), [0.5] * 3, [1] * 3, float(z["expand_scale"]), rng=r1, seg_classes=int(z["seg_classes"]), **kw)
    plain = augment.TrainAugment(z["sizes"].tolist(), [0.5] * 3, [1] * 3, float(z["expand_scale"]), rng=r2, **kw)
    a, b = seg.plan(groups), plain.plan([[m[:2] for m in g] for g in groups])
    assert a["items"].tobytes() == b["items"].tobytes() and a["samples"].tobytes() == b["samples"].tobytes()
    assert a["size"] == b["size"] == tuple(int(v) for v in z["size"]) and a["count"] == b["count"]
    for i, (s, t) in enumerate(zip(a["targets"], b["targets"])):
        assert torch.equal(s, t) and np.array_equal(s.numpy(), z["out_tgt%d" % i])
    assert r1.getstate() == r2.getstate()
    assert np.array_equal(np.array([r1.random() for _ in range(4)]), z["after"])


# generic shapes (source h, w -> grid h, w), the integer-scale case of the issue, a mixed one (one axis integer), scale 1
AREA_SHAPES = [((52, 78), (26, 26)), ((61, 97), (6, 10)), ((200, 133), (26, 26)), ((26, 200), (2, 26)), ((131, 60), (10, 6)),
               ((97, 26), (13, 26)), ((40, 52), (10, 26)), ((26, 26), (26, 26)), ((57, 143), (26, 10))]


@pytest.mark.parametrize("src,dst", AREA_SHAPES)
def test_restated_area_resize_within_half_a_level_of_exact_average(src, dst):
    r = np.random.RandomState(src[0] * 1000 + src[1])
    fast = S.area_is_fast(src[0], dst[0]) and S.area_is_fast(src[1], dst[1])
    assert fast == (src in ((52, 78), (40, 52), (26, 26)))      # integer on BOTH axes; (26, 200) and (97, 26) are integer on one only
    worst = 0.0
    for k in range(4):
        ids = r.randint(0, 4, size=src).astype(np.uint8)
        if k % 2:                                       # large uniform regions as a real id map has
            ids = np.kron(r.randint(0, 4, size=(4, 4)), np.ones((src[0] // 4 + 1, src[1] // 4 + 1))).astype(np.uint8)[:src[0], :src[1]]
        binary = np.where(ids == 1, 255, 0).astype(np.uint8)
        got = S.resize_area_u8(binary, *dst)
        assert got.dtype == np.uint8 and got.shape == dst
        worst = max(worst, float(np.abs(got.astype(np.float64) - S.exact_area_average(binary, *dst)).max()))
    print("area resize %s -> %s: worst |restated - exact| = %.9f grey levels" % (src, dst, worst))
    assert worst <= 0.5 + 1e-6


def test_area_resize_fast_path_and_scale_one():
    r = np.random.RandomState(2)
    b = (r.randint(0, 2, size=(52, 52)) * 255).astype(np.uint8)
    assert S.area_is_fast(52, 26) and S.area_scale(52, 26) == 2.0
    cnt = (b // 255).reshape(26, 2, 26, 2).sum(axis=(1, 3))
    assert np.array_equal(S.resize_area_u8(b, 26, 26), np.array([0, 64, 128, 191, 255], np.uint8)[cnt])      # 127.5 -> 128 (even)
    assert np.array_equal(S.resize_area_u8(b, 52, 52), b)                                                     # scale 1 is the identity
    with pytest.raises(ValueError, match="scale < 1"):
        S.resize_area_u8(b, 53, 26)
    m = S.seg_maps(np.array([[0, 1, 2, 3]] * 4, np.uint8).repeat(4, 0).repeat(4, 1), 2, (1, 4))
    assert m.shape == (1, 4, 2) and np.array_equal(m[0, :, 0], [0, 1, 0, 0]) and np.array_equal(m[0, :, 1], [0, 0, 1, 0])   # ids 0 and 3: no map


def _bdd_config():
    return json.load(open(os.path.join(G, "state_keys_bdd100k.json")))["config"]


def test_from_config_accepts_the_bdd100k_config():
    from mobilenet_yolo_pytorch_amd import augment
    cfg = _bdd_config()
    assert cfg["seg"]["num_classes"] == 2 and cfg["mosaic_num"] == [1]
    aug = augment.TrainAugment.from_config(cfg, device="cpu")
    assert aug.seg_classes == 2 and aug.sizes == [(416, 416)] and aug.expand_scale == cfg["expand_scale"]
    for bad in ([1, 4], [2], None):                               # the sampler would build mosaic groups, which have no seg maps
        with pytest.raises(ValueError, match="mosaic_num"):
            augment.TrainAugment.from_config(dict(cfg, mosaic_num=bad), device="cpu")
    with pytest.raises(ValueError, match="mosaic_num"):
        augment.TrainAugment.from_config({k: v for k, v in cfg.items() if k != "mosaic_num"}, device="cpu")
    del cfg["seg"]
    assert augment.TrainAugment.from_config(dict(cfg, mosaic_num=[1, 4]), device="cpu").seg_classes is None


def test_seg_refusals_on_the_host():
    from mobilenet_yolo_pytorch_amd import augment
    mk = lambda **kw: augment.TrainAugment([[416, 416]], [0.5] * 3, [1] * 3, 1.3, device="cpu", rng=random.Random(0), **kw)
    with pytest.raises(ValueError, match="seg_classes"):
        mk(seg_classes=9)
    with pytest.raises(ValueError, match="seg_classes"):
        mk(seg_classes=0)
    aug = mk(seg_classes=2)
    im, sg, t = np.zeros((80, 100, 3), np.uint8), np.zeros((80, 100), np.uint8), np.zeros((0, 5), np.float32)
    with pytest.raises(ValueError, match="Mosaic"):
        aug.plan([[(im, t, sg), (im, t, sg)]])
    with pytest.raises(ValueError, match="seg_id"):
        aug.plan([[(im, t, sg[:, :99])]])
    with pytest.raises(ValueError, match="seg_id"):
        aug.plan([[(im, t, sg.astype(np.int32))]])
    small = np.zeros((30, 25, 3), np.uint8)                      # 25 < the 26-wide grid, whatever the crop
    with pytest.raises(ValueError, match="smaller than the 26x26 seg grid"):
        aug.plan([[(small, t, np.zeros((30, 25), np.uint8))]], size=(416, 416))
    plan = aug.plan([[(im, t, sg)]], size=(416, 416))            # 80x100 crops to at least 40x50: fine
    assert plan["size"] == (416, 416) and len(plan["samples"]) == 1
    with pytest.raises(ValueError, match="square"):
        augment.TrainAugment([[416, 352]], [0.5] * 3, [1] * 3, 1.3, device="cpu", seg_classes=2)


def test_library_refuses_bad_arguments_on_the_host():
    """Argument errors are raised before anything is launched, so they need no GPU."""
    import ctypes
    import mobilenet_yolo_pytorch_amd.build as b
    from mobilenet_yolo_pytorch_amd import _lib
    b.build()
    assert _lib.query("mny_aug_seg_ws_bytes", 4, 4, 2, 720, 1280, 26, 26) >= 4
    assert _lib.query("mny_aug_seg_ws_bytes", 4, 4, 9, 720, 1280, 26, 26) == 0
    assert _lib.query("mny_aug_seg_ws_bytes", 4, 4, 0, 720, 1280, 26, 26) == 0
    with pytest.raises(_lib.MnyError, match="null pointer"):
        _lib.call("mny_aug_seg_batch", None, None, None, 1, None, 1, 2, 64, 64, 6, 6, None, None, None)
    host = (ctypes.c_uint64 * 64)()                                # never dereferenced: the checks come first
    q = ctypes.c_void_p(ctypes.addressof(host))
    for C in (0, 9):
        with pytest.raises(_lib.MnyError, match="n_classes"):
            _lib.call("mny_aug_seg_batch", q, q, q, 1, q, 1, C, 64, 64, 6, 6, q, q, None)
    with pytest.raises(_lib.MnyError, match="exceeds"):
        _lib.call("mny_aug_seg_batch", q, q, q, 1, q, 1, 8, 4000, 4000, 600, 600, q, q, None)
