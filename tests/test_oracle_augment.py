"""CPU: the augmentation restatement (tests/augment_ref.py) against the REAL reference's outputs (tests/golden/aug_*.npz,
tools/gen_golden_augment.py) and against live Pillow; TrainAugment.plan (the product's host half) against both."""
import glob
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as A

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "aug_*.npz")))
Image = pytest.importorskip("PIL.Image")
ImageEnhance = pytest.importorskip("PIL.ImageEnhance")


def load(name):
    z = np.load(os.path.join(G, name))
    n = int(z["count"])
    imgs = [z["img%d" % i] for i in range(n)]
    tg = [z["tgt%d" % i] for i in range(n)]
    groups, k = [], 0
    for s in z["groups"]:
        groups.append([(imgs[k + j], tg[k + j]) for j in range(int(s))])
        k += int(s)
    return z, groups


@pytest.fixture(scope="module")
def cube():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_fixtures_present_and_cover_the_cases():
    assert FIXTURES == ["aug_mix.npz", "aug_mosaic.npz", "aug_singles.npz"]
    seen = set()
    for name in FIXTURES:
        z, groups = load(name)
        samples, _, _ = A.plan(random.Random(int(z["seed"])), [[(im.shape[0], im.shape[1], t) for im, t in g] for g in groups],
                               float(z["expand_scale"]), int(z["canvas"]), z["sizes"].tolist())
        for g, s in zip(groups, samples):
            seen.add("mosaic%d" % len(g))
            seen.update(k for m in s["members"] for k, v in (("expand", m["expand"]), ("crop", m["crop"]), ("flip", m["flip"])) if v)
            seen.update("nocrop" for m in s["members"] if m["crop"] is None)
            seen.update("empty" for _, t in g if len(t) == 0)
    assert {"mosaic1", "mosaic2", "mosaic3", "mosaic4", "expand", "crop", "nocrop", "flip", "empty"} <= seen, seen


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_reference(name):
    z, groups = load(name)
    rng = random.Random(int(z["seed"]))
    samples, size, count = A.plan(rng, [[(im.shape[0], im.shape[1], t) for im, t in g] for g in groups], float(z["expand_scale"]),
                                  int(z["canvas"]), z["sizes"].tolist())
    assert np.array_equal(np.array([rng.random() for _ in range(4)]), z["after"])
    assert tuple(size) == tuple(z["size"]) and count == int(z["count"])
    u8 = []
    for i, (g, s) in enumerate(zip(groups, samples)):
        img = A.render_u8([im for im, _ in g], s, int(z["canvas"]))
        assert img.shape == z["u8_%d" % i].shape and np.array_equal(img, z["u8_%d" % i]), i
        t = s["target"].numpy()
        assert t.shape == z["out_tgt%d" % i].shape and np.array_equal(t, z["out_tgt%d" % i]), i
        u8.append(img)
    assert np.array_equal(A.collate(u8, size, z["mean"], z["std"]), z["batch"])


@pytest.mark.parametrize("name", FIXTURES)
def test_train_augment_plan_matches_reference(name):
    from mobilenet_yolo_pytorch_amd import augment
    z, groups = load(name)
    rng = random.Random(int(z["seed"]))
    aug = augment.TrainAugment(z["sizes"].tolist(), z["mean"], z["std"], float(z["expand_scale"]), canvas=int(z["canvas"]), device="cpu", rng=rng)
    plan = aug.plan(groups)
    assert np.array_equal(np.array([rng.random() for _ in range(4)]), z["after"])
    assert plan["size"] == tuple(int(v) for v in z["size"]) and plan["count"] == int(z["count"])
    for i, t in enumerate(plan["targets"]):
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), z["out_tgt%d" % i]), i
    # the descriptors say what the restatement draws
    ref, _, _ = A.plan(random.Random(int(z["seed"])), [[(im.shape[0], im.shape[1], t) for im, t in g] for g in groups],
                       float(z["expand_scale"]), int(z["canvas"]), z["sizes"].tolist())
    items = plan["items"]
    k = 0
    for si, s in enumerate(ref):
        assert tuple(plan["samples"][si])[:2] == (k, len(s["members"]))
        for j, m in enumerate(s["members"]):
            it = items[k]
            assert it["sample"] == si and it["flip"] == int(m["flip"]) and it["n_ops"] == len(m["chain"])
            assert list(it["op"][:it["n_ops"]]) == [op for op, _ in m["chain"]]
            h, w = int(it["h"]), int(it["w"])
            assert tuple(it["exp"]) == (m["expand"] if m["expand"] is not None else (h, w, 0, 0))
            e = tuple(it["exp"])
            assert tuple(it["crop"]) == (m["crop"] if m["crop"] is not None else (0, 0, e[0], e[1]))
            if s["tiles"] is not None:
                assert tuple(it["tile"]) == s["tiles"][j] and tuple(it["mask"]) == s["masks"][j]
            k += 1


def test_train_augment_refuses_seg_config():
    from mobilenet_yolo_pytorch_amd import augment
    cfg = {"train_img_size": [[352, 352]], "expand_scale": 1.5, "normalize": {"mean": [0.5] * 3, "std": [1] * 3}, "seg": {"num_classes": 2}}
    with pytest.raises(ValueError, match="seg"):
        augment.TrainAugment.from_config(cfg, device="cpu")
    del cfg["seg"]
    aug = augment.TrainAugment.from_config(cfg, device="cpu")
    assert aug.sizes == [(352, 352)] and aug.expand_scale == 1.5 and aug.canvas == 1000


def test_host_tables_match_restatement():
    from mobilenet_yolo_pytorch_amd import augment
    for f in (-18 / 255., -5.3 / 255., -0.2 / 255., 0.0, 0.01, 17.99 / 255.):
        assert augment.hue_shift_u8(f) == A.hue_shift_u8(f) == int(np.array(f * 255).astype(np.uint8))
    assert A.hue_shift_u8(-5.3 / 255.) == 251 and A.hue_shift_u8(-17.99 / 255.) == 239 and A.hue_shift_u8(-0.2 / 255.) == 0
    for g in (0.5, 0.77, 1.0, 1.33, 1.5):
        assert np.array_equal(augment.gamma_map(g), A.gamma_map(g))


@pytest.mark.parametrize("f", [0.5, 0.8137, 1.0, 1.2549, 1.5])
def test_blend_ops_match_pillow_on_rgb_cube(cube, f):
    im = Image.fromarray(cube)
    assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), A.brightness(cube, f))
    assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), A.contrast(cube, f))
    assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), A.saturation(cube, f))


def test_contrast_mean_follows_the_chain():
    """Contrast's grey is the mean of the image AS IT IS when contrast runs, not of the source."""
    img = A.brightness(np.full((8, 8, 3), 200, np.uint8), 0.5)
    assert A.l_mean(img) == 100
    assert np.array_equal(np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(1.3)), A.contrast(img, 1.3))


def test_l_and_hsv_match_pillow_on_rgb_cube(cube):
    im = Image.fromarray(cube)
    assert np.array_equal(np.asarray(im.convert("L")), A.to_l(cube))
    hsv = np.asarray(im.convert("HSV"))
    assert np.array_equal(hsv, A.rgb_to_hsv(cube))
    assert np.array_equal(np.asarray(Image.fromarray(hsv, "HSV").convert("RGB")), A.hsv_to_rgb(hsv))


@pytest.mark.parametrize("f", [-18 / 255., -5.3 / 255., 0.0, 0.031, 17.99 / 255.])
def test_hue_matches_pillow_on_rgb_cube(cube, f):
    im = Image.fromarray(cube)
    h, s, v = im.convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    nh += np.array(f * 255).astype(np.uint8)                        # torchvision adjust_hue's PIL path
    ref = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    assert np.array_equal(ref, A.hue(cube, f))


@pytest.mark.parametrize("g", [0.55, 0.9, 1.1, 1.45])
def test_gamma_matches_pillow_on_rgb_cube(cube, g):
    lut = [int((255 + 1 - 1e-3) * 1 * pow(e / 255.0, g)) for e in range(256)] * 3
    assert np.array_equal(np.asarray(Image.fromarray(cube).point(lut)), A.gamma(cube, g))


@pytest.mark.parametrize("out", [(19, 27), (71, 89), (37, 91), (13, 53), (151, 7), (1, 1)])
def test_bicubic_matches_pillow(out):
    from mobilenet_yolo_pytorch_amd import synthetic
    for p in synthetic.photos([(37, 53), (61, 41)], seed=3):
        ref = np.asarray(Image.fromarray(p).resize((out[1], out[0]), Image.BICUBIC))
        assert np.array_equal(ref, A.resize_bicubic_u8(p, *out))
        assert np.array_equal(np.asarray(Image.fromarray(p).resize((out[1], out[0]))), ref)   # Pillow's default for RGB


def test_geometry_and_mosaic_against_pillow():
    """expand / crop / flip through PIL ops, and one mosaic canvas built with Pillow + numpy as Mosaic does."""
    from mobilenet_yolo_pytorch_amd import synthetic
    p, q = synthetic.photos([(30, 44), (25, 20)], seed=5)
    canvas = np.full((50, 60, 3), 127, np.uint8)
    canvas[7:37, 9:53] = p
    ref = np.asarray(Image.fromarray(canvas[4:40, 3:45]).transpose(Image.FLIP_LEFT_RIGHT))
    assert np.array_equal(A.geometry(p, (50, 60, 7, 9), (4, 3, 36, 42), True), ref)
    bg = np.zeros((64, 64, 3))
    tiles = [(p, (0, 3, 30, 20), (0, 0, 30, 64)), (q, (30, 0, 34, 64), (30, 0, 64, 64))]
    for img, (x, y, w, h), m in tiles:
        t = np.array(Image.fromarray(img).resize((w, h)))
        bg[m[1]:m[3], m[0]:m[2]] = np.mean(t, axis=(0, 1))
        bg[y:y + h, x:x + w] = t
    assert np.array_equal(A.mosaic(tiles, 64), bg.astype(np.uint8))
