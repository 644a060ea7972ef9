"""CPU: the specification of the text part of the annotation stage.  tests/vizlabel_ref.py restates include/mnyolo.h (mny_viz_labels,
mny_viz_compose_labels) in numpy; here the strips viz.build_atlas renders, the score digits and the label drawing are held to Pillow
(ImageDraw.text with the built-in bitmap font, byte for byte) and the placement to answers worked by hand.  The argument checks of the
two entry points run through the library: they need no GPU."""
import ctypes

import numpy as np
import pytest

import viz_ref as V
import vizlabel_ref as VL

SCORES = [0.005, 0.125, 0.15, 0.3, 0.375, 0.62, 0.87, 0.995, 1.0]
PAL = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)


@pytest.fixture(scope="module")
def viz():
    from mobilenet_yolo_pytorch_amd import viz
    return viz


@pytest.fixture(scope="module")
def names():
    from mobilenet_yolo_pytorch_amd import synthetic
    return synthetic.VOC_NAMES + synthetic.BDD_NAMES + ["Person", "Traffic Light", "TV Monitor", "AEROPLANE", "Yak", "Jeep"]


@pytest.fixture(scope="module")
def builtin(viz, names):
    pytest.importorskip("PIL")
    return viz.build_atlas(names)


def pillow_text(s, font, w, h):
    from PIL import Image, ImageDraw
    im = Image.new("L", (w, h), 0)
    ImageDraw.Draw(im).text((0, 0), s, fill=255, font=font)
    return np.asarray(im)


def one_label(strips, n_names, h, x0, y0, W, cls=0, prod=None, filled=True, bg=(200, 100, 50), fg=(255, 255, 255)):
    """A label record through the restatement, from a box record with the corner (x0, y0)."""
    rec = np.zeros(1, V.BOX)
    rec[0] = (x0, y0, x0 + 30, y0 + 20, bg, 2)
    row = np.array([[0, 0, 0, 0, 1.0 if prod is None else prod, 1.0, cls]], np.float32)
    return VL.labels(row, 0, rec, W, strips, n_names, h, with_score=prod is not None, filled=filled, text_rgb=fg)[0]


def test_the_record_mirrors_the_header(viz):
    assert viz.LABEL == VL.LABEL and viz.LABEL.itemsize == 48 and viz.CHARS == VL.CHARS
    assert viz.LABEL.fields["seq"][1] == 12 and viz.LABEL.fields["n"][1] == 38 and viz.LABEL.fields["fg"][1] == 44
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mnyolo.h")).read()
    assert "} mny_viz_label; /* 48 bytes */" in src and "_LABEL_STRIPS 13" in src
    assert "_MAX_TEXT_H %d\n" % viz.MAX_TEXT_H in src and "_MAX_STRIP_W %d\n" % viz.MAX_STRIP_W in src and "_MAX_NAMES %d\n" % viz.MAX_NAMES in src


def test_composed_strips_equal_pillows_whole_string(viz, names, builtin):
    """The strip of a name, then the strips of ' ', digit, '.', digit, digit side by side = Pillow's rendering of "%s %.2f"."""
    from PIL import ImageFont
    atlas, strips, h = builtin
    font = ImageFont.load_default_imagefont()
    assert h == 11 and len(strips) == len(names) + 12
    cases = 0
    for c, name in enumerate(names):
        assert strips[c, 1] == 6 * len(name)
        for s in SCORES:
            lab = np.zeros(1, VL.LABEL)[0]
            seq = VL.sequence(c, len(names), np.float32(s))
            lab["seq"][:len(seq)], lab["n"], lab["lh"] = seq, len(seq), h
            text = "%s %.2f" % (name, float(np.float32(s)))
            got = VL.text_row(lab, atlas, strips)
            assert got.shape == (11, 6 * len(text)), text
            assert np.array_equal(got, pillow_text(text, font, got.shape[1], h)), text
            cases += 1
    assert cases >= 36 * 8
    assert set(np.unique(atlas)) == {0, 255}                                   # a 1-bit font


def test_single_characters_must_not_be_abutted(builtin, names):
    """Why names are rendered whole: some capitals reach outside their cell, and Pillow pastes glyph after glyph."""
    from PIL import ImageFont
    font = ImageFont.load_default_imagefont()
    differ = 0
    for name in names:
        cells = np.concatenate([pillow_text(ch, font, 6, 11) for ch in name], 1)
        differ += int((cells != pillow_text(name, font, 6 * len(name), 11)).sum())
    assert differ > 0


def test_score_digits_equal_printf():
    rng = np.random.default_rng(0)
    ties = np.array([0.125, 0.375, 0.625, 0.875, 0.005, 0.015, 0.995, 0.985, 0.0, 1.0, 0.15] + [k / 200 for k in range(201)], np.float32)
    vals = np.concatenate([rng.random(120000, dtype=np.float32), ties, np.nextafter(ties, np.float32(2)), np.nextafter(ties, np.float32(-1)).clip(0)])
    assert len(vals) >= 100000
    bad = 0
    for v in vals:
        k = VL.score_digits(v)
        bad += "%d.%d%d" % (k // 100, k // 10 % 10, k % 10) != "%.2f" % float(v)
    assert bad == 0
    assert VL.score_digits(np.float32(0.125)) == 12 and VL.score_digits(np.float32(0.375)) == 38       # ties to even, exact in fp64
    assert VL.score_digits(np.float32(-0.3)) == 0 and VL.score_digits(np.float32(12.0)) == 999 and VL.score_digits(np.float32(np.inf)) == 999
    assert VL.score_digits(np.float32(np.nan)) == 0 and VL.score_digits(np.float32(9.99)) == 999 and VL.score_digits(np.float32(9.98)) == 998


def test_the_class_index_stands_in_for_a_missing_name():
    assert VL.sequence(3.0, 5) == [3] and VL.sequence(4.9, 5) == [4]                                      # (int)cls
    assert VL.sequence(5.0, 5) == [5 + 5] and VL.sequence(120.0, 5) == [5 + 1, 5 + 2, 5 + 0]
    assert VL.sequence(16777215.0, 0) == [1, 6, 7, 7, 7, 2, 1, 5]                                         # eight digits at the most
    assert VL.sequence(7.0, 0, np.float32(0.5)) == [7, VL.SPACE, 0, VL.DOT, 5, 0]
    assert len(VL.sequence(16777215.0, 2, np.float32(1))) == 13


def draw_with_pillow(img, lab, text, font):
    from PIL import Image, ImageDraw
    im = Image.fromarray(img.copy())
    d = ImageDraw.Draw(im)
    lx, ly, lw, lh = int(lab["lx"]), int(lab["ly"]), int(lab["lw"]), int(lab["lh"])
    if int(lab["filled"]):
        d.rectangle([lx, ly, lx + lw - 1, ly + lh - 1], fill=tuple(int(c) for c in lab["bg"]))
    d.text((lx + 2, ly), text, fill=tuple(int(c) for c in lab["fg"]), font=font)
    return np.asarray(im)


@pytest.mark.parametrize("filled", [True, False])
def test_label_drawing_equals_pillow_rectangle_then_text(builtin, names, filled):
    from PIL import ImageFont
    atlas, strips, h = builtin
    font = ImageFont.load_default_imagefont()
    rng = np.random.default_rng(1)
    H, W = 60, 120
    # (x0, y0, class, product): above the box; inside it (box at the top edge, and one row short); clamped at the right edge, at it
    # and one beyond; left of the image; wider than the image
    cases = [(10, 30, 14, 0.87), (10, 0, 6, 0.5), (40, 10, 20, 0.25), (90, 40, 13, 0.62), (W - 52, 25, 6, 0.995), (W - 51, 25, 6, 0.125), (-7, 40, 2, 0.3),
             (5, 11, 32, 0.15), (3, 50, 10, 0.99), (30, 59, 27, 0.45)]
    seen = set()
    for x0, y0, c, prod in cases:
        for width in (W, 40):                                                  # 40: most labels are wider than the image
            img = rng.integers(0, 256, (H, width, 3), dtype=np.uint8)
            lab = one_label(strips, len(names), h, x0, y0, width, c, np.float32(prod), filled, fg=(250, 240, 10))
            text = "%s %.2f" % (names[c], float(np.float32(prod)))
            assert int(lab["lw"]) == 6 * len(text) + 4
            got = VL.draw_label(img.copy(), lab, atlas, strips)
            assert np.array_equal(got, draw_with_pillow(img, lab, text, font)), (x0, y0, c, width)
            assert not np.array_equal(got, img)
            seen |= {"above" if int(lab["ly"]) < y0 else "inside", "wide" if int(lab["lw"]) > width else "fits",
                     "clamped" if 0 < int(lab["lx"]) < x0 else "", "left" if x0 < 0 else ""}
    assert {"above", "inside", "wide", "fits", "clamped", "left"} <= seen
    lab = one_label(strips, len(names), h, 10, 30, W, 14, None, filled)        # label="name": no score
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert int(lab["n"]) == 1 and np.array_equal(VL.draw_label(img.copy(), lab, atlas, strips), draw_with_pillow(img, lab, "person", font))


@pytest.mark.parametrize("filled", [True, False])
def test_antialiased_text_of_the_freetype_font_equals_pillow(viz, filled):
    """Every blend level: the strings as whole strips of ImageFont.load_default(16), blended by the rule, against ImageDraw.text."""
    features = pytest.importorskip("PIL.features")
    if not features.check("freetype2"):
        pytest.skip("Pillow without FreeType")
    from PIL import ImageFont
    font = ImageFont.load_default(16)
    texts = ["person 0.87", "traffic light", "bike", "Bus 1.00", "car"]
    atlas, strips, h = viz.build_atlas(texts, font)
    assert h == sum(font.getmetrics()) and len(np.unique(atlas)) > 20           # antialiased
    rng = np.random.default_rng(2)
    H, W = 50, 110
    for c, text in enumerate(texts[:4]):
        assert font.getbbox(text)[2] <= strips[c, 1]                             # the ink ends within the advance width, the strip's
        for x0, y0 in ((8, 30), (60, 5), (-4, 21)):
            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            lab = one_label(strips, len(texts), h, x0, y0, W, c, None, filled, bg=(30, 60, 200), fg=(255, 250, 5))
            assert np.array_equal(VL.draw_label(img.copy(), lab, atlas, strips), draw_with_pillow(img, lab, text, font)), (text, x0, y0)
    # a strip is as wide as the advance (the header's w_k): the faint column by which this font's "r" overhangs it is cut, nothing else moves
    assert font.getbbox("car")[2] == strips[4, 1] + 1
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = one_label(strips, len(texts), h, 8, 30, W, 4, None, filled, bg=(30, 60, 200), fg=(255, 250, 5))
    differ = (VL.draw_label(img.copy(), lab, atlas, strips) != draw_with_pillow(img, lab, "car", font)).any(2)
    assert differ.any() and set(np.nonzero(differ)[1]) == {8 + 2 + int(strips[4, 1])}


def test_placement_by_hand():
    strips = np.array([[0, 20]] + [[0, 6]] * 12, np.int32)                      # one name of 20 columns: lw = 24 without a score
    h, W = 11, 100
    at = lambda x0, y0, **k: one_label(strips, 1, h, x0, y0, W, 0, **k)
    assert (int(at(5, 11)["ly"]), int(at(5, 10)["ly"]), int(at(5, 12)["ly"])) == (0, 10, 1)        # above exactly from y0 == lh
    assert (int(at(5, 0)["ly"]), int(at(5, -3)["ly"]), int(at(5, -40)["ly"])) == (0, -3, -40)       # never above a box that starts off the image
    assert int(at(5, 40)["lw"]) == 24 and int(at(5, 40, prod=np.float32(0.5))["lw"]) == 20 + 5 * 6 + 4
    assert (int(at(76, 40)["lx"]), int(at(77, 40)["lx"]), int(at(75, 40)["lx"]), int(at(500, 40)["lx"])) == (76, 76, 75, 76)   # x0 = W - lw and beyond
    assert (int(at(-1, 40)["lx"]), int(at(-50, 40)["lx"]), int(at(0, 40)["lx"])) == (0, 0, 0)
    wide = one_label(strips, 1, h, 3, 40, 10, 0)                                # wider than the image: starts at column 0
    assert (int(wide["lx"]), int(wide["lw"])) == (0, 24)
    lab = at(5, 40, prod=np.float32(0.875), filled=False, bg=(1, 2, 3), fg=(4, 5, 6))
    assert list(lab["seq"][:6]) == [0, 1 + 11, 1 + 0, 1 + 10, 1 + 8, 1 + 8] and int(lab["n"]) == 6 and int(lab["filled"]) == 0
    assert tuple(lab["bg"]) == (1, 2, 3) and tuple(lab["fg"]) == (4, 5, 6) and int(lab["lh"]) == 11
    # empty: an empty box record, targets with label_targets off, a class that is no class
    rec = np.zeros(3, V.BOX)
    rec[1] = (1, 20, 9, 30, (9, 9, 9), 2)
    rec[2] = (1, 20, 9, 30, (9, 9, 9), 2)
    tg = np.array([[0, .5, .5, .1, .1], [0, .5, .5, .1, .1], [np.nan, .5, .5, .1, .1]], np.float32)
    on, off = VL.labels(tg, 1, rec, W, strips, 1, h), VL.labels(tg, 1, rec, W, strips, 1, h, label_targets=False)
    assert list(on["n"]) == [0, 1, 0] and on[0].tobytes() == bytes(48) and off.tobytes() == bytes(3 * 48)
    assert VL.labels(tg, 1, rec, W, strips, 1, h, with_score=True)[1]["n"] == 1   # a target has no score


def test_blend_by_hand():
    m = np.array([0, 255, 128, 1, 254], np.uint8)
    under = np.array([37, 37, 100, 0, 255], np.uint8)
    # 128 * 200 + 127 * 100 + 128 = 38428 -> ((38428 >> 8) + 38428) >> 8 = 150; 1 * 200 + 128 = 328 -> 1; 254 * 200 + 255 + 128 = 51183 -> 200
    assert list(VL.blend(m, under, 200)) == [37, 200, 150, 1, 200]


def test_later_labels_draw_over_earlier_ones_and_over_outlines():
    strips = np.array([[0, 8]] * 13, np.int32)
    atlas = np.zeros(8 * 4, np.uint8)
    atlas[::3] = 255
    rec = np.zeros(2, V.BOX)
    rec[0] = (2, 6, 20, 18, (200, 0, 0), 1)
    rec[1] = (4, 8, 22, 19, (0, 200, 0), 1)
    rows = np.array([[0, 0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 1, 1, 0]], np.float32)
    labs = VL.labels(rows, 0, rec, 30, strips, 1, 4, with_score=False)
    assert (int(labs[0]["ly"]), int(labs[1]["ly"])) == (2, 4)
    ab = VL.draw(np.zeros((24, 30, 3), np.uint8), rec, labs, atlas, strips)
    ba = VL.draw(np.zeros((24, 30, 3), np.uint8), rec[::-1], labs[::-1], atlas, strips)
    assert tuple(ab[4, 4]) == (0, 200, 0) and tuple(ba[4, 4]) == (200, 0, 0)    # the padding column of both labels
    assert tuple(ab[6, 5]) == (0, 200, 0) and tuple(ba[6, 5]) == (200, 0, 0)    # label 1 over the outline of box 0, and the outline over the label


def test_names_the_font_cannot_render_and_limits(viz):
    pytest.importorskip("PIL")
    with pytest.raises(ValueError, match="class 1"):
        viz.Annotator(names=["car", "中"])
    with pytest.raises(ValueError, match="wide"):
        viz.Annotator(names=["x" * 200])
    with pytest.raises(ValueError):
        viz.Annotator(names=["a"] * (viz.MAX_NAMES + 1))
    with pytest.raises(ValueError):
        viz.Annotator(names=["a"], label="score")
    from PIL import ImageFont, features
    if features.check("freetype2"):
        with pytest.raises(ValueError, match="line height"):
            viz.Annotator(names=["a"], font=ImageFont.load_default(80))
    ann = viz.Annotator(names=["car", ""])
    assert ann.text_h == 11 and list(ann.strips[:2, 1]) == [18, 0] and len(ann.atlas) == 11 * (18 + 12 * 6)
    plain = viz.Annotator()
    assert plain.names is None and not hasattr(plain, "atlas")


def test_argument_errors_do_not_need_a_gpu(viz):
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd._lib import MnyError, call
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rgb = (ctypes.c_uint8 * 3)(255, 255, 255)
    labels = lambda **k: call("mny_viz_labels", *[k.get(a, d) for a, d in (("rows", p), ("mode", 0), ("begin", p), ("count", p), ("S", 1), ("capacity", 4), ("dims", p),
                                                                            ("boxes", p), ("strips", p), ("n_names", 3), ("h", 11), ("score", 1), ("filled", 1),
                                                                            ("targets", 1), ("rgb", rgb), ("out", p), ("stream", None))])
    for k in ("rows", "begin", "count", "dims", "boxes", "strips", "rgb", "out"):
        with pytest.raises(MnyError, match="mny_viz_labels: null pointer"):
            labels(**{k: None})
    with pytest.raises(MnyError, match="mode 2"):
        labels(mode=2)
    for bad in (dict(n_names=-1), dict(n_names=viz.MAX_NAMES + 1), dict(h=0), dict(h=viz.MAX_TEXT_H + 1), dict(S=-1), dict(capacity=-1)):
        with pytest.raises(MnyError, match="mny_viz_labels"):
            labels(**bad)
    labels(S=0)                                                                 # nothing to do: no launch
    labels(capacity=0, rows=None)
    m3 = (ctypes.c_float * 3)(0, 0, 0)
    compose = lambda **k: call("mny_viz_compose_labels", *[k.get(a, d) for a, d in (
        ("batch", p), ("H", 4), ("W", 4), ("mean", m3), ("std", m3), ("src", None), ("desc", None), ("items", p), ("N", 1), ("boxes", p), ("begin", p),
        ("count", p), ("capacity", 1), ("seg", None), ("C", 0), ("chan", None), ("dst", p), ("ws", p), ("labels", p), ("atlas", p), ("strips", p), ("stream", None))])
    for k in ("items", "dst", "ws", "mean"):
        with pytest.raises(MnyError, match="mny_viz_compose_labels: null pointer"):
            compose(**{k: None})
    for k in ("boxes", "atlas", "strips"):
        with pytest.raises(MnyError, match="labels without"):
            compose(**{k: None})
    with pytest.raises(MnyError, match="exactly one of batch and src"):
        compose(src=p)
    with pytest.raises(MnyError, match="bad batch size"):
        compose(N=0)
    with pytest.raises(MnyError, match="seg classes"):
        compose(C=9)
