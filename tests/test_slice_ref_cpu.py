"""CPU: the sliced-inference specification (include/mnyolo.h) through its numpy restatement (tests/slice_ref.py) and the package's host
half (slicing.tile_grid, slicing.tile_map, the record tables): hand-worked grids, the tile prep against Pillow's crop + resize byte for
byte, and hand-worked rows of the append (the four edge tests, the margin itself, NaN, non-interior sides, the clamp, the map's rounding)."""
import numpy as np
import pytest

import slice_ref
from oracle import prep_ref

f32, f64 = np.float32, np.float64
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _grid(*a):
    from mobilenet_yolo_pytorch_amd.slicing import tile_grid
    got = tile_grid(*a)
    assert got == slice_ref.tile_grid(*a)                                           # the package's rule is the published loop's
    return got


# ---- the grid ------------------------------------------------------------------------------------------------------------
def test_grid_bdd_frame():
    """1280 x 720, tile 416, overlap 0.2: ox = oy = int(83.2) = 83, step 333.  x: 0, 333, 666, then 999 + 416 = 1415 > 1280 -> shifted to
    864..1280 (and 1415 >= 1280 ends the row).  y: 0, then 333 + 416 = 749 > 720 -> 304..720."""
    g = _grid(720, 1280, 416, 416, 0.2, 0.2)
    assert g == [(x, y, x + 416, y + 416) for y in (0, 304) for x in (0, 333, 666, 864)]


def test_grid_exactly_one_tile_smaller_image_and_no_overlap():
    assert _grid(416, 416, 416, 416, 0.2, 0.2) == [(0, 0, 416, 416)]                # end 416 is not below 416: one row, one column
    assert _grid(100, 300, 416, 416, 0.2, 0.2) == [(0, 0, 300, 100)]                # clamped to the image in both axes
    assert _grid(100, 500, 416, 416, 0.2, 0.2) == [(0, 0, 416, 100), (84, 0, 500, 100)]        # one axis smaller: clamped in that axis only
    assert _grid(832, 832, 416, 416, 0.0, 0.0) == [(0, 0, 416, 416), (416, 0, 832, 416), (0, 416, 416, 832), (416, 416, 832, 832)]
    assert _grid(833, 416, 416, 416, 0.0, 0.0) == [(0, 0, 416, 416), (0, 416, 416, 832), (0, 417, 416, 833)]
    # duplicates are not removed: 64-tile, overlap 0.5 on 96 rows: starts 0, 32 (end 96, not below 96: the last)
    assert _grid(96, 64, 64, 64, 0.5, 0.0) == [(0, 0, 64, 64), (0, 32, 64, 96)]
    # two image sizes of the GPU test: 150 x 100 and 64 x 200 at tile 64, overlap 0.25 (step 48)
    assert _grid(150, 100, 64, 64, 0.25, 0.25) == [(x, y, x + 64, y + 64) for y in (0, 48, 86) for x in (0, 36)]
    assert _grid(64, 200, 64, 64, 0.25, 0.25) == [(x, 0, x + 64, 64) for x in (0, 48, 96, 136)]


def test_grid_rectangular_tile_and_overlaps():
    g = _grid(100, 100, 40, 60, 0.5, 0.25)                                          # oy = 20, ox = 15: y 0, 20, 40, 60 (end 100: last); x 0, 45 -> 40
    assert g == [(x, y, x + 60, y + 40) for y in (0, 20, 40, 60) for x in (0, 40)]


@pytest.mark.parametrize("args", [(10, 10, 4, 4, 1.0, 0.0), (10, 10, 4, 4, 0.0, 1.0), (10, 10, 4, 4, -0.1, 0.0), (10, 10, 4, 4, 0.0, 1.5),
                                  (10, 10, 4, 4, float("nan"), 0.0), (0, 10, 4, 4, 0.0, 0.0), (10, 10, 0, 4, 0.0, 0.0), (10, 10, 4, -1, 0.0, 0.0),
                                  (10.5, 10, 4, 4, 0.0, 0.0)])
def test_grid_argument_errors(args):
    from mobilenet_yolo_pytorch_amd.slicing import tile_grid
    with pytest.raises(ValueError):
        tile_grid(*args)


def test_grid_covers_every_pixel_on_200_random_sizes():
    rng = np.random.default_rng(5)
    for _ in range(200):
        h, w = (int(v) for v in rng.integers(1, 400, size=2))
        th, tw = (int(v) for v in rng.integers(1, 130, size=2))
        oh, ow = (float(v) for v in rng.choice([0.0, 0.1, 0.2, 0.25, 0.5, 0.9], size=2))
        g = _grid(h, w, th, tw, oh, ow)
        seen = np.zeros((h, w), bool)
        for x0, y0, x1, y1 in g:
            assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
            assert (x1 - x0, y1 - y0) == (min(tw, w), min(th, h))                   # the tile's size, or clamped to a smaller image
            seen[y0:y1, x0:x1] = True
        assert seen.all(), (h, w, th, tw, oh, ow)


# ---- the tile prep -------------------------------------------------------------------------------------------------------
H, W = 37, 53
# (x0, y0, x1, y1): 1x1, 1x7 (h x w), 13x5 windows at the four corners and inside, and the whole image
WINDOWS = [(0, 0, 1, 1), (W - 1, 0, W, 1), (0, H - 1, 1, H), (W - 1, H - 1, W, H), (20, 11, 21, 12),
           (0, 0, 7, 1), (W - 7, 0, W, 1), (0, H - 1, 7, H), (W - 7, H - 1, W, H), (9, 17, 16, 18),
           (0, 0, 5, 13), (W - 5, 0, W, 13), (0, H - 13, 5, H), (W - 5, H - 13, W, H), (31, 8, 36, 21),
           (0, 0, W, H)]


def _image():
    return np.random.default_rng(7).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("out", [32, 64])
def test_tile_prep_equals_pillow_crop_resize(out):
    """The window is an image of its own: Pillow's crop(box).resize(..., BILINEAR) byte for byte (up-scale, and 37x53 -> 32: down-scale;
    70x90 -> 32 in the GPU test is the down-scale by more than 2).  Image.resize(box=) reads the neighbours and is NOT the model."""
    Image = pytest.importorskip("PIL.Image")
    img = _image()
    pil = Image.fromarray(img)
    differs = 0
    for box in WINDOWS:
        x0, y0, x1, y1 = box
        want_u8 = np.asarray(pil.crop(box).resize((out, out), Image.BILINEAR))
        got = slice_ref.prep_window(img, box, out, out, MEAN, STD)
        assert np.array_equal(got, prep_ref.to_tensor_normalize(want_u8, MEAN, STD)), box
        # the restatement through the flat buffer and the pitch is the same thing
        t = np.array([((y0 * W + x0) * 3, y1 - y0, x1 - x0, 3 * W, 0)], dtype=slice_ref.TILE_DESC)
        flat, status = slice_ref.prep_tiles(img.reshape(-1), t, H, W, out, out, MEAN, STD)
        assert status == 0 and np.array_equal(flat[0], got), box
        differs += int(not np.array_equal(np.asarray(pil.resize((out, out), Image.BILINEAR, box=box)), want_u8))
    assert differs > 0                                                              # (the two Pillow calls do differ: the choice matters)


def test_tile_prep_downscale_by_more_than_two():
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(8).integers(0, 256, size=(80, 100, 3), dtype=np.uint8)
    box = (5, 7, 95, 77)                                                            # 70 x 90 -> 32 x 32
    want = np.asarray(Image.fromarray(img).crop(box).resize((32, 32), Image.BILINEAR))
    assert np.array_equal(slice_ref.prep_window(img, box, 32, 32, MEAN, STD), prep_ref.to_tensor_normalize(want, MEAN, STD))


def test_tile_prep_padding_and_out_of_bound_slots():
    img = _image()
    t = np.array([(0, 5, 5, 3 * W, 0), (0, 5, 5, 3 * W, -1), (0, H, 5, 3 * W, 0), (0, 5, 5, 14, 1), (0, 0, 5, 3 * W, 1)], dtype=slice_ref.TILE_DESC)
    out, status = slice_ref.prep_tiles(img.reshape(-1), t, H - 1, W, 32, 32, MEAN, STD)
    assert status == 3 and out[0].any() and not out[1:].any()                       # slot 2 is the first bad one: 1 + 2
    assert slice_ref.prep_tiles(img.reshape(-1), t[:2], H, W, 32, 32, MEAN, STD)[1] == 0       # a padding slot sets no status


def test_record_tables_match_the_header_structs():
    from mobilenet_yolo_pytorch_amd import slicing
    assert slicing.TILE_DESC == slice_ref.TILE_DESC and slicing.TILE_DESC.itemsize == 24
    assert slicing.TILE_MAP == slice_ref.TILE_MAP and slicing.TILE_MAP.itemsize == 48
    assert [slicing.TILE_MAP.fields[k][1] for k in ("ax", "bx", "ay", "by", "ex", "ey", "image", "interior")] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert [slicing.TILE_DESC.fields[k][1] for k in ("offset", "h", "w", "pitch", "image")] == [0, 8, 12, 16, 20]
    for box in [(0, 0, 64, 64), (36, 48, 100, 112), (36, 86, 100, 150), (0, 0, 100, 150)]:
        a, b = slicing.tile_map(box, 150, 100, 4, 64, 3), slice_ref.make_map(box, 150, 100, 4, 64, 3)
        assert a.tobytes() == b.tobytes()
    m = slicing.tile_map((36, 48, 100, 112), 150, 100, 4, 64, 3)
    assert int(m["interior"]) == slice_ref.LEFT | slice_ref.TOP | slice_ref.BOTTOM and m["ex"] == f32(0.0625) and m["ax"] == 36 / 100
    assert int(slicing.tile_map((0, 0, 100, 150), 150, 100, 4, 64, 0)["interior"]) == 0


# ---- the append ----------------------------------------------------------------------------------------------------------
def _map(interior=0, ex=0.25, ey=0.125, ax=0.0, bx=1.0, ay=0.0, by=1.0, image=0):
    m = np.zeros((), slice_ref.TILE_MAP)
    m["ax"], m["bx"], m["ay"], m["by"], m["ex"], m["ey"], m["image"], m["interior"] = ax, bx, ay, by, ex, ey, image, interior
    return m


def _row(x1, y1, x2, y2, tag=0.0):
    return np.array([x1, y1, x2, y2, 0.5, 0.25, tag], dtype=f32)


below = lambda v: np.nextafter(f32(v), f32(-1))
above = lambda v: np.nextafter(f32(v), f32(2))

# (row, the one interior bit whose test it fails); margins ex = 0.25, ey = 0.125: 1 - ex = 0.75, 1 - ey = 0.875 exactly
EDGE_ROWS = [(_row(below(0.25), 0.5, 0.5, 0.6), slice_ref.LEFT), (_row(0.3, below(0.125), 0.5, 0.6), slice_ref.TOP),
             (_row(0.3, 0.5, above(0.75), 0.6), slice_ref.RIGHT), (_row(0.3, 0.5, 0.5, above(0.875)), slice_ref.BOTTOM)]


def test_each_edge_test_drops_its_row_only_on_its_interior_side():
    for row, bit in EDGE_ROWS:
        for interior in range(16):
            assert slice_ref.cut(row, _map(interior)) == bool(interior & bit), (row, interior)
    assert not slice_ref.cut(_row(0.0, 0.0, 1.0, 1.0), _map(0))                     # non-interior sides are never tested


def test_on_the_margin_and_nan_are_kept():
    assert not slice_ref.cut(_row(0.25, 0.125, 0.75, 0.875), _map(15))              # every value exactly on its margin: all compares strict
    for c in range(4):
        row = _row(0.3, 0.3, 0.6, 0.6)
        row[c] = np.nan
        assert not slice_ref.cut(row, _map(15)), c
    # edge = 0: ex = 0, 1 - ex = 1: only a box that leaves the tile is dropped
    assert not slice_ref.cut(_row(0.0, 0.0, 1.0, 1.0), _map(15, ex=0.0, ey=0.0))
    assert slice_ref.cut(_row(-0.01, 0.0, 1.0, 1.0), _map(15, ex=0.0, ey=0.0)) and not slice_ref.cut(_row(-0.01, 0.0, 1.0, 1.0), _map(14, ex=0.0, ey=0.0))


def test_map_rounding_is_two_fp64_operations_then_one_fp32_rounding():
    rng = np.random.default_rng(9)
    m = slice_ref.make_map((333, 304, 749, 720), 720, 1280, 0, 416, 0)
    assert m["ax"] == f64(333) / f64(1280) and m["bx"] == f64(416) / f64(1280) and m["ay"] == f64(304) / f64(720)
    differs = 0
    for _ in range(2000):
        row = _row(*rng.uniform(-0.1, 1.1, size=4).astype(f32))
        got = slice_ref.map_row(row, m)
        for c, (a, b) in enumerate((("ax", "bx"), ("ay", "by"), ("ax", "bx"), ("ay", "by"))):
            assert got[c] == f32(f64(m[a]) + f64(m[b]) * f64(row[c]))
            differs += int(got[c] != f32(m[a]) + f32(m[b]) * row[c])                # an fp32 evaluation rounds differently somewhere
        assert np.array_equal(got[4:], row[4:])
    assert differs > 0
    ident = _map()
    for _ in range(100):
        row = _row(*rng.uniform(-0.1, 1.1, size=4).astype(f32))
        assert slice_ref.map_row(row, ident).tobytes() == row.tobytes()             # ax = 0, bx = 1: bit-identical copies
    big = slice_ref.map_row(_row(-0.5, 0.0, 1.5, 1.0), _map(ax=0.5, bx=0.5))
    assert big[0] == f32(0.25) and big[2] == f32(1.25)                              # nothing is clipped to [0, 1]


def test_append_order_clamp_and_dropped():
    """Three slots: 0 and 2 go to image 1, slot 1 to image 0; image 1's segment (stride 4, base 1) fills up in the middle of slot 2."""
    src = np.zeros((4, 3, 7), f32)
    for b in range(4):
        for r in range(3):
            src[b, r] = _row(0.3, 0.3, 0.6, 0.6, tag=10 * b + r)
    src[0, 1] = _row(0.1, 0.3, 0.6, 0.6, tag=1)                                     # cut on the left in slot 0 (interior = LEFT)
    maps = np.array([_map(slice_ref.LEFT, image=1), _map(image=0), _map(ax=0.5, bx=0.5, image=1), _map(image=-1)])
    counts_src = np.array([3, 2, 5, 3], np.int32)                                   # slot 2: above the stride of 3 -> 3 rows
    dst = np.full((2, 4, 7), -7.0, f32)
    counts, dropped = np.array([0, 1], np.int32), np.zeros(2, np.int32)
    slice_ref.det_append_tiles(src, counts_src, maps, dst, counts, dropped)
    assert counts.tolist() == [2, 4] and dropped.tolist() == [0, 2]                 # image 1: 2 + 3 survivors offered, 3 fit behind base 1
    assert dst[0, :2, 6].tolist() == [10.0, 11.0] and (dst[0, 2:] == -7.0).all()
    assert (dst[1, 0] == -7.0).all() and dst[1, 1:, 6].tolist() == [0.0, 2.0, 20.0]  # slot 0's survivors, then slot 2's first row
    assert dst[1, 3, 0] == f32(0.5 + 0.5 * f64(f32(0.3))) and dst[1, 1, 0] == f32(0.3)
    # a count outside its segment: nothing is appended, every survivor is counted as dropped
    counts2, dropped2 = np.array([9, -1], np.int32), np.zeros(2, np.int32)
    before = dst.copy()
    slice_ref.det_append_tiles(src, counts_src, maps, dst, counts2, dropped2)
    assert counts2.tolist() == [9, -1] and dropped2.tolist() == [2, 5] and np.array_equal(dst, before)
