"""Sliced inference on the MI355X: mny_prep_tiles and mny_det_append_tiles against the numpy restatement (tests/slice_ref.py) and against
mny_prep_batch bit for bit, the one-tile identity of slicing.Sliced against model(x), the whole call against the oracle pipeline on the
same heads (the chunk plans' decoded rows through the numpy append and the existing NMS), a `seg:` config and the errors.  Every
comparison is exact (array_equal)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import slice_ref
from oracle import procedural

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
f32, f64 = np.float32, np.float64
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
C3 = lambda v: (ctypes.c_float * 3)(*v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _table(a):
    return _dev(a.view(np.uint8).reshape(-1))


# ---- mny_prep_tiles ----------------------------------------------------------------------------------------------------
def _pack(imgs):
    """the images back to back in one flat uint8 buffer (16-byte aligned starts) -> (buffer, offsets)"""
    offs, off = [], 0
    for im in imgs:
        offs.append(off)
        off += (im.size + 15) // 16 * 16
    buf = np.zeros(off, np.uint8)
    for o, im in zip(offs, imgs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, offs


def _tiles_case():
    """Two images (37x53 and 80x100).  Slots: 1x1, 1x7 and 13x5 windows at the four corners of image 0 and inside it (pitch > 3*w), the
    whole 37x53 image (pitch == 3*w), a 70x90 window of image 1, two overlapping windows of image 0, and a padding slot in the middle."""
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((37, 53), (80, 100))]
    buf, offs = _pack(imgs)
    H, W = 37, 53
    boxes = []
    for hh, ww in ((1, 1), (1, 7), (13, 5)):
        boxes += [(0, 0, 0, ww, hh), (0, W - ww, 0, W, hh), (0, 0, H - hh, ww, H), (0, W - ww, H - hh, W, H), (0, 20, 11, 20 + ww, 11 + hh)]
    boxes += [(0, 0, 0, W, H), (1, 5, 7, 95, 77), (0, 10, 5, 40, 30), (0, 25, 15, 45, 35)]
    tiles = []
    for i, x0, y0, x1, y1 in boxes:
        w = imgs[i].shape[1]
        tiles.append((offs[i] + (y0 * w + x0) * 3, y1 - y0, x1 - x0, 3 * w, i))
    tiles.insert(9, (0, 5, 5, 15, -1))                                              # a padding slot between live ones
    return buf, np.array(tiles, dtype=slice_ref.TILE_DESC)


@pytest.mark.parametrize("out", [32, 64])
def test_prep_tiles_equals_restatement(out):
    from mobilenet_yolo_pytorch_amd import ops
    buf, tiles = _tiles_case()
    want, status = slice_ref.prep_tiles(buf, tiles, 80, 100, out, out, MEAN, STD)
    got, ws = ops.prep_tiles(_dev(buf), _table(tiles), len(tiles), 80, 100, out, out, C3(MEAN), C3(STD))
    assert status == 0 and int(ws[:4].view(torch.int32).item()) == 0
    got = got.cpu().numpy()
    for b in range(len(tiles)):
        assert np.array_equal(got[b], want[b]), (b, tiles[b])
    assert not got[9].any() and all(got[b].any() for b in range(len(tiles)) if b != 9)
    live = tiles[tiles["image"] >= 0]
    assert (live["pitch"] == 3 * live["w"]).sum() == 1 and (live["pitch"] > 3 * live["w"]).sum() == len(live) - 1           # both kinds of pitch


def test_prep_tiles_out_of_bound_window_is_flagged_and_written_as_zeros():
    from mobilenet_yolo_pytorch_amd import ops
    buf, tiles = _tiles_case()
    sel = tiles[[0, 9, 17, 16, 12]]                                                 # 1x1, padding, 70x90 (larger than max_h = 64), 37x53, 13x5
    want, status = slice_ref.prep_tiles(buf, sel, 64, 100, 32, 32, MEAN, STD)
    got, ws = ops.prep_tiles(_dev(buf), _table(sel), len(sel), 64, 100, 32, 32, C3(MEAN), C3(STD))
    assert status == 3 and int(ws[:4].view(torch.int32).item()) == 3                # 1 + b of the window that is too large; the padding slot sets nothing
    got = got.cpu().numpy()
    assert np.array_equal(got, want) and not got[1].any() and not got[2].any() and got[3].any()
    sel = sel.copy()
    sel["pitch"][3] = 3 * 53 - 1                                                    # a pitch below 3 * w
    sel["h"][2] = 60
    got, ws = ops.prep_tiles(_dev(buf), _table(sel), len(sel), 64, 100, 32, 32, C3(MEAN), C3(STD))
    assert int(ws[:4].view(torch.int32).item()) == 4 and not got[3].any() and bool(got[2].any())


def test_prep_tiles_whole_images_equal_prep_batch():
    """Whole-image windows with pitch == 3 * w: mny_prep_batch on the same images, bit for bit (one set of kernels behind both)."""
    from mobilenet_yolo_pytorch_amd import ops, prep, synthetic
    imgs = synthetic.photos([(150, 200), (220, 130), (64, 64), (33, 47)], seed=4)
    bp = prep.BatchPrep([(64, 64)], MEAN, STD)
    want = bp(imgs).cpu().numpy()
    stage, desc, mh, mw = bp.pack(imgs)
    tiles = np.array([(int(d["offset"]), int(d["h"]), int(d["w"]), 3 * int(d["w"]), i) for i, d in enumerate(desc)], dtype=slice_ref.TILE_DESC)
    got, ws = ops.prep_tiles(stage.cuda(), _table(tiles), len(tiles), mh, mw, 64, 64, bp.mean, bp.std)
    assert int(ws[:4].view(torch.int32).item()) == 0
    assert np.array_equal(got.cpu().numpy(), want)
    ident = (imgs[2].astype(f32).transpose(2, 0, 1) / f32(255) - np.asarray(MEAN, f32)[:, None, None]) / np.asarray(STD, f32)[:, None, None]
    assert np.array_equal(want[2], ident)                                           # a window of the output's size: copy + normalisation


# ---- mny_det_append_tiles ----------------------------------------------------------------------------------------------
SENTINEL = -7.0
SRC_STRIDE, DST_STRIDE = 300, 400
#           slot:  0  1   2   3   4    5    6    7    8    9   10  11
SLOT_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 300, 400, 50, 20]                   # round the wave scan and the 256-row trip; 400 > src_stride
SLOT_IMAGE = [0, 0, 1, 0, 1, 2, 0, 1, 2, 0, -1, 2]                                  # image 0: slots 0, 1, 3 with slot 2 (image 1) between them
SLOT_INTERIOR = [1, 2, 4, 8, 15, 0, 1, 2, 4, 8, 15, 0]                              # every single bit, all four, none
BASE = [2, 1, 3]


def _append_case():
    rng = np.random.default_rng(31)
    B = len(SLOT_COUNTS)
    src = np.zeros((B, SRC_STRIDE, 7), f32)
    xy = rng.uniform(-0.05, 0.9, size=(B, SRC_STRIDE, 2)).astype(f32)
    wh = rng.uniform(0.01, 0.3, size=(B, SRC_STRIDE, 2)).astype(f32)
    src[:, :, 0:2], src[:, :, 2:4] = xy, xy + wh
    src[:, :, 4:6] = rng.uniform(0.0, 1.0, size=(B, SRC_STRIDE, 2)).astype(f32)
    src[:, :, 6] = (np.arange(B)[:, None] * 1000 + np.arange(SRC_STRIDE)[None, :]).astype(f32)       # (slot, row): the order is visible
    src[5, 7, 0] = src[5, 9, 3] = np.nan                                            # slot 5 has the identity map
    src[6, 3, 0] = np.nan                                                           # a NaN x1 on a tested side: kept
    maps = np.zeros(B, slice_ref.TILE_MAP)
    for b in range(B):
        maps[b] = slice_ref.make_map((36, 48, 100, 112), 150, 100, 6.4, 64, SLOT_IMAGE[b])           # ex = ey = 0.1
        maps[b]["interior"] = SLOT_INTERIOR[b]
    maps[5]["ax"], maps[5]["bx"], maps[5]["ay"], maps[5]["by"] = 0.0, 1.0, 0.0, 1.0
    dst = np.full((4, DST_STRIDE, 7), SENTINEL, f32)                                # one more block behind the last image: a guard
    return src, np.array(SLOT_COUNTS, np.int32), maps, dst, np.array(BASE, np.int32), np.zeros(3, np.int32)


def test_append_tiles_equals_restatement():
    """Image 0 (slots 0, 1, 3, 6, 9) and image 2 (slots 5, 8, 11) fill up in the middle of a slot: `dropped` is exact, and the rows behind
    every segment (the next image's base rows, the guard block behind the last) keep the sentinel.  Image 1 has room to spare."""
    from mobilenet_yolo_pytorch_amd import ops
    src, src_counts, maps, dst, counts, dropped = _append_case()
    d_dst, d_counts, d_dropped = _dev(dst), _dev(counts), _dev(dropped)
    ops.det_append_tiles(_dev(src), _dev(src_counts), _table(maps), d_dst[:3], d_counts, d_dropped)
    slice_ref.det_append_tiles(src, src_counts, maps, dst[:3], counts, dropped)
    got = d_dst.cpu().numpy()
    assert np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(d_dropped.cpu().numpy(), dropped)
    assert np.array_equal(got, dst, equal_nan=True)
    assert counts.tolist()[0] == DST_STRIDE and counts.tolist()[2] == DST_STRIDE and counts[1] < DST_STRIDE
    assert dropped[0] > 0 and dropped[2] > 0 and dropped[1] == 0
    for n in range(3):                                                              # the canaries: base rows and the guard block
        assert (got[n, :BASE[n]] == SENTINEL).all()
    assert (got[3] == SENTINEL).all() and (got[1, counts[1]:] == SENTINEL).all()
    tags = got[0, BASE[0]:, 6]
    assert (np.diff(tags) > 0).all() and {int(t) // 1000 for t in tags} >= {3, 6, 9}                  # slot order, source order
    assert {int(t) // 1000 for t in got[1, BASE[1]:counts[1], 6]} == {2, 4, 7}
    # every interior bit dropped something, the untested slot (5, the identity map) dropped nothing and is a bit-identical copy
    for b in (2, 4, 7):
        kept = [r for r in range(SLOT_COUNTS[b]) if not slice_ref.cut(src[b, r], maps[b])]
        assert 0 < len(kept) < SLOT_COUNTS[b]
    seg2 = got[2, BASE[2]:BASE[2] + 255]
    ok = ~np.isnan(src[5, :255])
    assert np.array_equal(ok, ~np.isnan(seg2)) and seg2[ok].tobytes() == src[5, :255][ok].tobytes() and (~ok).sum() == 2
    assert np.isnan(got[0]).sum() == 1                                              # slot 6's NaN row survived the left-edge test
    assert src_counts[9] > SRC_STRIDE and int(got[0, :, 6].max()) // 1000 <= 9


def test_append_tiles_no_slots_no_images_and_padding_only():
    from mobilenet_yolo_pytorch_amd import _lib, ops
    _lib.call("mny_det_append_tiles", None, 0, None, None, 0, None, 0, None, None, 0, None)          # B == 0, N == 0
    dst, counts, dropped = torch.full((2, 4, 7), SENTINEL, device="cuda"), torch.zeros(2, device="cuda", dtype=torch.int32), torch.zeros(
        2, device="cuda", dtype=torch.int32)
    _lib.call("mny_det_append_tiles", None, 0, None, None, 0, ops._p(dst), 4, ops._p(counts), ops._p(dropped), 2, None)      # B == 0
    src = torch.rand(2, 3, 7, device="cuda")
    maps = np.zeros(2, slice_ref.TILE_MAP)
    maps["image"], maps["bx"], maps["by"] = [-1, 5], 1.0, 1.0                       # a padding slot and an image outside 0..N-1
    ops.det_append_tiles(src, _dev(np.array([3, 3], np.int32)), _table(maps), dst, counts, dropped)
    assert counts.tolist() == [0, 0] and dropped.tolist() == [0, 0] and bool((dst == SENTINEL).all())


# ---- slicing.Sliced ----------------------------------------------------------------------------------------------------
VAL_CONF = 0.3


@pytest.fixture(scope="module")
def model():
    from mobilenet_yolo_pytorch_amd import yolo
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG, sync_metrics=True)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = VAL_CONF
    return m


@pytest.mark.parametrize("with_post", [False, True], ids=["plain", "post_defaults"])
def test_one_tile_without_full_view_equals_model(model, with_post):
    from mobilenet_yolo_pytorch_amd import prep, synthetic
    from mobilenet_yolo_pytorch_amd.postprocess import PostProcess
    from mobilenet_yolo_pytorch_amd.slicing import Sliced
    imgs = synthetic.photos([(64, 64), (64, 64)], seed=6)
    want = [d.cpu().numpy() for d in model(prep.BatchPrep([(64, 64)], MEAN, STD)(imgs, size=(64, 64)))]
    sl = Sliced(model, size=64, tile=(64, 64), overlap=0, full_view=False, edge=0, batch=2, mean=MEAN, std=STD,
                post=PostProcess() if with_post else None)
    got = sl(imgs)
    assert isinstance(got, list) and len(got) == 2 and all(d.is_cuda and d.shape[1] == 7 for d in got)
    assert sum(len(d) for d in want) > 0
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.cpu().numpy(), b)


def _records(imgs, offs, edge):
    """the records of a call, restated: per image the full view, then the grid's tiles; -> (TILE_DESC [R], TILE_MAP [R])"""
    tiles, maps = [], []
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        for box in [(0, 0, w, h)] + slice_ref.tile_grid(h, w, 64, 64, 0.25, 0.25):
            x0, y0, x1, y1 = box
            tiles.append((offs[i] + (y0 * w + x0) * 3, y1 - y0, x1 - x0, 3 * w, i))
            maps.append(slice_ref.make_map(box, h, w, edge, 64, i))
    out = np.zeros(len(maps), slice_ref.TILE_MAP)
    for r, m in enumerate(maps):
        out[r] = m
    return np.array(tiles, dtype=slice_ref.TILE_DESC), out


SLICED_CASES = {
    # batch = 4: the 7 + 5 records fill three chunks exactly; batch = 5: the last chunk holds two records and three padding slots
    "plain_batch4": dict(batch=4, edge=0, merge=False, post=False),
    "plain_padded": dict(batch=5, edge=0, merge=False, post=False),
    "edge4_padded": dict(batch=5, edge=4, merge=False, post=False),
    "merge_padded": dict(batch=5, edge=4, merge=True, post=False),
    "agnostic_max_det20_batch4": dict(batch=4, edge=4, merge=False, post=True),
    "agnostic_max_det20_padded": dict(batch=5, edge=4, merge=True, post=True),
}


@pytest.mark.parametrize("case", list(SLICED_CASES))
def test_sliced_equals_oracle_pipeline_on_same_heads(model, case):
    """Images of 150x100 and 64x200, tile 64, overlap 0.25 (6 and 4 tiles), full view.  The oracle: the records restated, every chunk's
    input from the restated tile prep, the chunk plan's own forward and decode on it, the numpy append into the joint buffer, then the
    existing NMS (and top-k, merge) entry points.  val_conf = 0.3, photos seed 3: with the CPU oracle network the two images give 174 / 124
    candidates of which the edge rule drops 128 / 87 at edge 0 (the procedural weights decode boxes larger than a 64-pixel tile) and every
    tile keeps some; the asserts below hold the non-vacuity on the GPU's own heads."""
    from mobilenet_yolo_pytorch_amd import ops, postprocess, synthetic
    from mobilenet_yolo_pytorch_amd.postprocess import PostProcess
    from mobilenet_yolo_pytorch_amd.slicing import Sliced
    cfg = SLICED_CASES[case]
    post = PostProcess(agnostic=True, max_det=20) if cfg["post"] else None
    imgs = synthetic.photos([(150, 100), (64, 200)], seed=3)
    sl = Sliced(model, size=64, tile=(64, 64), overlap=0.25, full_view=True, edge=cfg["edge"], batch=cfg["batch"], mean=MEAN, std=STD,
                merge=cfg["merge"], post=post)
    got = [d.cpu().numpy() for d in sl(imgs)]

    buf, offs = _pack(imgs)
    tiles, maps = _records(imgs, offs, cfg["edge"])
    R, Bc = len(tiles), cfg["batch"]
    assert R == 12 and np.bincount(tiles["image"]).tolist() == [7, 5]
    chunks = -(-R // Bc)
    pad = chunks * Bc - R
    assert pad == (3 if Bc == 5 else 0)
    tiles = np.concatenate([tiles, np.zeros(pad, slice_ref.TILE_DESC)])
    maps = np.concatenate([maps, np.zeros(pad, slice_ref.TILE_MAP)])
    tiles["image"][R:] = maps["image"][R:] = -1
    x_all, status = slice_ref.prep_tiles(buf, tiles, 150, 200, 64, 64, MEAN, STD)
    assert status == 0
    plan = model._plans[(Bc, 64, 64, False)]
    C = model.num_classes
    stride = plan.cap if post is None else post.stride(plan.cap, C)
    cap = 7 * stride
    joint, counts, dropped = np.zeros((2, cap, 7), f32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    cut_rows, alive_tiles = 0, set()
    for k in range(chunks):
        x = _dev(x_all[k * Bc:(k + 1) * Bc])
        if post is None:
            plan.forward_eval(x, [VAL_CONF, VAL_CONF], nms=False)
            rows, cnt = plan.rows.cpu().numpy(), plan.cnt1.cpu().numpy()
        else:
            plan.forward_eval(x, [VAL_CONF, VAL_CONF], decode=False)
            d_rows = torch.zeros(Bc, stride, 7, device="cuda")
            z = [torch.zeros(Bc, device="cuda", dtype=torch.int32) for _ in range(4)]
            postprocess.decode_plan(plan, post, model, d_rows, z[0], z[1], z[2], z[3], None)
            rows, cnt = d_rows.cpu().numpy(), z[1].cpu().numpy()
            assert not z[2].any() and not z[3].any()
        for b in range(Bc):
            m = maps[k * Bc + b]
            if m["image"] >= 0:
                kept = sum(not slice_ref.cut(r, m) for r in rows[b, :cnt[b]])
                cut_rows += int(cnt[b]) - kept
                if kept and m["interior"]:
                    alive_tiles.add((int(m["image"]), k * Bc + b))
        slice_ref.det_append_tiles(rows, cnt, maps[k * Bc:(k + 1) * Bc], joint, counts, dropped)
    assert cut_rows > 0, "no candidate was dropped by the edge rule: the case is vacuous"
    assert max(sum(1 for i, _ in alive_tiles if i == n) for n in range(2)) >= 3, "no image keeps candidates from three tiles"
    assert not dropped.any() and counts.min() >= 20
    assert np.array_equal(next(iter(sl._bufs.values()))["counts"].cpu().numpy(), counts)
    assert np.array_equal(next(iter(sl._bufs.values()))["rows"].cpu().numpy()[0, :counts[0]], joint[0, :counts[0]])

    d_rows, begin, count = _dev(joint.reshape(-1, 7)), _dev(np.arange(2, dtype=np.int32) * cap), _dev(counts)
    if post is None:
        out_idx, out_counts, out_rows, prefix, st = ops.nms_per_class(d_rows, begin, count, C, thr=0.45, max_seg_rows=cap)
        thr = 0.45
    else:
        out_idx, out_counts, out_rows, prefix, st = ops.nms_agnostic(d_rows, begin, count, thr=post.iou_thres, max_seg_rows=cap)
        prefix = ops.det_topk(d_rows, begin, out_idx, out_counts, out_rows, 20)
        thr = post.iou_thres
    if cfg["merge"]:
        ops.nms_merge(d_rows, begin, count, out_idx, out_counts, prefix, out_rows, thr=thr)
    assert int(st.item()) == 0
    pre = prefix.cpu().numpy()
    want = out_rows.cpu().numpy()
    for n in range(2):
        w = want[pre[n]:pre[n + 1]]
        assert len(w) > 0 and (post is None or len(w) <= 20)
        assert got[n].shape == w.shape and np.array_equal(got[n], w), (case, n)


def _bdd():
    from mobilenet_yolo_pytorch_amd import yolo
    man = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))
    torch.manual_seed(0)
    m = yolo(man["config"], sync_metrics=True)
    procedural.fill_state_dict_(m)
    return man["config"]["seg"]["num_classes"], m.cuda().eval()


def test_seg_config_returns_the_full_views_seg():
    """Two images smaller than the 128-pixel tile: each gives a full view and one tile, both the whole image, four records in one chunk
    of four: slots 0 and 2 are the full views.  model(x) on the same four inputs is the reference."""
    from mobilenet_yolo_pytorch_amd import MnyError, prep, synthetic
    from mobilenet_yolo_pytorch_amd.slicing import Sliced
    C, m = _bdd()
    imgs = synthetic.photos([(100, 80), (64, 64)], seed=8)
    x = prep.BatchPrep([(64, 64)], MEAN, STD)([imgs[0], imgs[0], imgs[1], imgs[1]], size=(64, 64))
    _, seg_plain = m(x)
    z_plain = m.seg_logits()
    sl = Sliced(m, size=64, tile=(128, 128), overlap=0.0, full_view=True, batch=4, mean=MEAN, std=STD)
    with pytest.raises(MnyError, match="no Sliced call"):
        sl.seg_logits()
    det, seg = sl(imgs)
    assert isinstance(det, list) and len(det) == 2 and all(d.shape[1] == 7 and d.is_cuda for d in det)
    assert isinstance(seg, np.ndarray) and seg.shape == (C, 4, 4) and np.array_equal(seg, seg_plain)
    z = sl.seg_logits()
    assert z.shape == (2, 4, 4, C) and z.dtype == torch.float32 and torch.equal(z, z_plain[[0, 2]])
    assert not torch.equal(z[0], z[1])
    off = Sliced(m, size=64, tile=(128, 128), overlap=0.0, full_view=False, batch=4, mean=MEAN, std=STD)
    det = off(imgs)                                                                 # detections only
    assert isinstance(det, list) and len(det) == 2 and all(isinstance(d, torch.Tensor) for d in det)
    with pytest.raises(MnyError, match="full_view"):
        off.seg_logits()


def test_errors(model):
    from mobilenet_yolo_pytorch_amd import MnyError, synthetic
    from mobilenet_yolo_pytorch_amd.slicing import Sliced
    kw = dict(mean=MEAN, std=STD)
    for bad in (dict(size=100), dict(size=0), dict(size=64, overlap=1.0), dict(size=64, overlap=-0.1), dict(size=64, edge=32),
                dict(size=64, edge=-1), dict(size=64, batch=0), dict(size=64, max_candidates=0), dict(size=64, tile=(0, 64))):
        with pytest.raises(ValueError):
            Sliced(model, **dict(kw, **bad))
    with pytest.raises(ValueError, match="mean and std"):
        Sliced(model, size=64)
    imgs = synthetic.photos([(150, 100), (64, 200)], seed=3)
    sl = Sliced(model, size=64, tile=(64, 64), overlap=0.25, batch=4, max_candidates=5, **kw)
    with pytest.raises(MnyError, match="image 0 has"):
        sl(imgs)
    with pytest.raises(ValueError, match="empty batch"):
        sl([])
    model.train()
    try:
        with pytest.raises(MnyError, match="model.eval"):
            Sliced(model, size=64, tile=(64, 64), **kw)(imgs)
    finally:
        model.eval()
