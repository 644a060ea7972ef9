"""CPU: the specification of the annotation stage.  tests/viz_ref.py restates include/mnyolo.h (mny_viz_boxes, mny_viz_compose) in
numpy; here its box rule is held to Pillow's ImageDraw.rectangle where the two agree by design (both sides at least 2 t), and
the rest, where the header's rule IS the specification, to answers worked by hand."""
import numpy as np
import pytest

import viz_ref as V

PAL = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)


def rec(*boxes):
    out = np.zeros(len(boxes), V.BOX)
    for i, b in enumerate(boxes):
        out[i] = b
    return out


def test_box_rule_equals_pillow_rectangle_on_boxes_of_at_least_2t():
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    from PIL import Image
    rng = np.random.default_rng(0)
    H, W = 40, 56
    checked = {1: 0, 2: 0, 3: 0, 4: 0}
    off_image = 0
    for _ in range(3000):
        t = int(rng.integers(1, 5))
        x0, x1 = sorted(int(v) for v in rng.integers(-12, W + 12, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(-12, H + 12, 2))
        if x1 - x0 < 2 * t or y1 - y0 < 2 * t:
            continue
        img = Image.new("RGB", (W, H), (9, 9, 9))
        ImageDraw.Draw(img).rectangle([x0, y0, x1, y1], outline=(200, 100, 50), width=t)
        mine = V.draw(np.full((H, W, 3), 9, np.uint8), rec((x0, y0, x1, y1, (200, 100, 50), t)))
        assert np.array_equal(np.asarray(img), mine), (x0, y0, x1, y1, t)
        checked[t] += 1
        off_image += x0 < 0 or y0 < 0 or x1 >= W or y1 >= H
    assert min(checked.values()) > 300 and off_image > 500


def test_thinner_boxes_by_hand():
    """A box with a side below 2 t has no interior under the rule: it is filled (Pillow leaves other pixels there)."""
    img = V.draw(np.zeros((6, 8, 3), np.uint8), rec((1, 1, 5, 3, (7, 8, 9), 2)))           # 5 wide, 3 tall, t = 2: 3 - 1 < 4
    want = np.zeros((6, 8), bool)
    want[1:4, 1:6] = True
    assert np.array_equal(img[..., 0] == 7, want) and np.array_equal(img[..., 2] == 9, want)
    img = V.draw(np.zeros((6, 8, 3), np.uint8), rec((2, 2, 2, 2, (7, 8, 9), 1)))           # a point
    assert (img[..., 0] == 7).sum() == 1 and img[2, 2, 0] == 7
    img = V.draw(np.zeros((8, 9, 3), np.uint8), rec((1, 1, 7, 4, (7, 8, 9), 2)))           # 7 x 4: x has an interior, y has not
    want = np.zeros((8, 9), bool)
    want[1:5, 1:8] = True
    assert np.array_equal(img[..., 0] == 7, want)
    img = V.draw(np.zeros((8, 9, 3), np.uint8), rec((1, 1, 7, 6, (7, 8, 9), 2)))           # 7 x 6: interior columns 3..5, rows 3..4
    want[1:7, 1:8] = True
    want[3:5, 3:6] = False
    assert np.array_equal(img[..., 0] == 7, want)
    assert not V.draw(np.zeros((4, 4, 3), np.uint8), rec((0, 0, 3, 3, (7, 8, 9), 0))).any()   # the empty record draws nothing


def test_later_boxes_win():
    a, b = (1, 1, 6, 6, (10, 0, 0), 1), (4, 0, 9, 3, (0, 20, 0), 1)
    ab = V.draw(np.zeros((8, 10, 3), np.uint8), rec(a, b))
    ba = V.draw(np.zeros((8, 10, 3), np.uint8), rec(b, a))
    assert tuple(ab[1, 4]) == (0, 20, 0) and tuple(ba[1, 4]) == (10, 0, 0)             # (4, 1) lies on both outlines
    assert tuple(ab[3, 6]) == (0, 20, 0) and tuple(ba[3, 6]) == (10, 0, 0)
    assert tuple(ab[2, 5]) == (0, 0, 0)                                                 # inside both, on neither outline
    assert tuple(ab[6, 1]) == (10, 0, 0) and tuple(ba[6, 1]) == (10, 0, 0)


def test_score_gate_at_exactly_thr():
    thr = np.float32(0.15)
    conf = np.float32(0.5)
    at = np.float32(0.3)                                                                # 0.5 * 0.3 in fp32
    assert np.float32(conf * at) == thr
    above = np.nextafter(at, np.float32(1))
    rows = np.array([[0.1, 0.1, 0.5, 0.5, conf, at, 1], [0.1, 0.1, 0.5, 0.5, conf, above, 2], [0.1, 0.1, 0.5, 0.5, np.nan, 1, 0],
                     [0.1, 0.1, 0.5, 0.5, 1, 1, np.nan], [0.1, np.nan, 0.5, 0.5, 1, 1, 0], [0.1, 0.1, 0.5, 0.5, 1, 1, -1]], np.float32)
    r = V.records(rows, 0, 20, 40, thr, PAL, 3)
    assert list(r["t"]) == [0, 3, 0, 0, 0, 0]                                           # strict: exactly thr is not drawn
    assert tuple(r[1]["rgb"]) == (0, 0, 255) and (int(r[1]["x0"]), int(r[1]["y0"]), int(r[1]["x1"]), int(r[1]["y1"])) == (4, 2, 20, 10)


def test_corners_round_half_up_and_are_ordered():
    rows = np.array([[0.5, 0.5, 0.0125, 0.025, 1, 1, 4], [0.0374, 0.9, -0.3, 1.4, 1, 1, 5]], np.float32)
    r = V.records(rows, 0, 20, 40, 0.1, PAL, 1)
    # 0.0125 * 40 = 0.5 -> floor(1.0) = 1; 0.025 * 20 = 0.5 -> 1; ordered: x0 = 1, x1 = 20
    assert (int(r[0]["x0"]), int(r[0]["y0"]), int(r[0]["x1"]), int(r[0]["y1"])) == (1, 1, 20, 10)
    assert tuple(r[0]["rgb"]) == (0, 255, 0)                                            # class 4 mod 3 colours
    # 0.0374 * 40 = 1.496 -> floor(1.996) = 1; -0.3 * 40 = -12 -> -12 (fp32: floor(-11.5 + eps) = -12); 1.4 * 20 = 28
    assert (int(r[1]["x0"]), int(r[1]["y0"]), int(r[1]["x1"]), int(r[1]["y1"])) == (-12, 18, 1, 28)
    t = V.records(np.array([[2, 0.5, 0.5, 0.25, 0.5]], np.float32), 1, 20, 40, 0.99, PAL, 2)   # targets ignore the gate
    assert (int(t[0]["x0"]), int(t[0]["y0"]), int(t[0]["x1"]), int(t[0]["y1"]), int(t[0]["t"])) == (15, 5, 25, 15, 2)
    assert tuple(t[0]["rgb"]) == (0, 0, 255)


def test_overlay_by_hand():
    img = np.full((1, 4, 3), 200, np.uint8)
    p = np.zeros((2, 1, 4), np.float32)
    just = np.nextafter(np.float32(0.5), np.float32(1))
    p[0, 0] = [0.5, just, 0.75, 0.75]
    p[1, 0] = [0.0, 0.0, 0.0, 0.875]
    out = V.overlay(img.copy(), p, (1, 0))
    assert tuple(out[0, 0]) == (200, 200, 200)                                          # p = 0.5 is not above 0.5
    assert tuple(out[0, 1]) == (200, 99, 200)                                           # 200 * (1 - 0.50000006) = 99.99999 -> 99
    assert tuple(out[0, 2]) == (200, 50, 200)
    assert tuple(out[0, 3]) == (25, 50, 200)                                            # class 1 on R: 200 * 0.125
    same = V.overlay(img.copy(), p, (1, 1))                                             # two classes on one channel: applied in class order
    assert tuple(same[0, 3]) == (200, 6, 200)                                           # 200 -> 50 -> trunc(50 * 0.125 = 6.25)
    assert np.array_equal(V.overlay(img.copy(), p[:0]), img)                            # C = 0
    odd = V.overlay(img.copy(), np.array([[[1.5, np.nan, 1.0, 0.6]]], np.float32), (2,))
    assert list(odd[0, :, 2]) == [0, 200, 0, 79]                                        # above 1 gives 0; NaN is not above 0.5; 1 - 0.6f = 0.39999998


def test_denormalise_round_trip_every_level():
    """(u8 / 255 - mean) / std in fp32, the normalisation of mny_prep_batch, comes back as u8 for all 256 levels x 3 channels under the
    normalisations of the reference's two configs and the identity the synthetic examples use."""
    lv = np.arange(256, dtype=np.float32)
    for mean, std in (([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]), ([0.5, 0.5, 0.5], [1, 1, 1]), ([0, 0, 0], [1, 1, 1])):
        m, s = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
        x = (np.broadcast_to(lv / np.float32(255), (3, 1, 256)) - m) / s
        assert x.dtype == np.float32
        back = V.denorm(x, mean, std)
        assert back.shape == (1, 256, 3) and np.array_equal(back[0], np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))
    wild = V.denorm(np.array([[[np.nan, -9.0, 9.0, np.inf]]] * 3, np.float32), [0, 0, 0], [1, 1, 1])
    assert wild[0, :, 0].tolist() == [0, 0, 255, 255]


def test_compose_order_source_boxes_overlay():
    x = np.zeros((3, 4, 6), np.float32)
    x[1] = 1.0
    p = np.zeros((1, 4, 6), np.float32)
    p[0, :, :3] = 0.75
    out = V.compose(x, rec((0, 0, 5, 3, (100, 100, 100), 1)), p, (1,), mean=[0, 0, 0], std=[1, 1, 1])
    assert tuple(out[0, 0]) == (100, 25, 100) and tuple(out[1, 1]) == (0, 63, 0) and tuple(out[1, 4]) == (0, 255, 0) and tuple(out[3, 5]) == (100, 100, 100)
