"""Annotation on the device (mny_viz_boxes, mny_viz_compose behind viz.Annotator) against the numpy restatement of
include/mnyolo.h (tests/viz_ref.py, which tests/test_viz_ref_cpu.py holds to Pillow and to hand-worked answers).  Exact equality
everywhere: the draw records byte for byte, the images pixel for pixel."""
import numpy as np
import pytest
import torch

import viz_ref as V

pytestmark = pytest.mark.gpu
LIST = 256                                                                       # kList of csrc/viz.hip: draw records per pass of the LDS list
WAVE = 64                                                                        # the scan appends wave by wave
TILE_W, TILE_H = 64, 16                                                          # the pixel tile of a workgroup
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PAL = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255]], np.uint8)


@pytest.fixture(scope="module")
def viz():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import viz
    return viz


def det_rows(rng, k, off_image=True):
    """[k,7] detection rows: boxes of every size, some partly outside the image, some below the score gate."""
    lo, hi = (-0.2, 1.2) if off_image else (0.0, 1.0)
    a, b = rng.uniform(lo, hi, (k, 2)), rng.uniform(lo, hi, (k, 2))
    rows = np.concatenate([np.minimum(a, b), np.maximum(a, b), rng.uniform(0.3, 1.0, (k, 2)), rng.integers(0, 20, (k, 1))], 1).astype(np.float32)
    return rows


def batch(rng, n, h, w):
    """A normalised fp32 batch whose pixels cover 0..255 and go a little beyond (the clamp)."""
    u = rng.integers(-3, 259, (n, 3, h, w)).astype(np.float32) / np.float32(255)
    return ((u - np.asarray(MEAN, np.float32).reshape(1, 3, 1, 1)) / np.asarray(STD, np.float32).reshape(1, 3, 1, 1)).astype(np.float32)


def cut(buf, desc):
    b = buf.cpu().numpy()
    return [b[int(d["offset"]):int(d["offset"]) + 3 * int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"]), 3) for d in desc]


def test_records_equal_the_restatement(viz):
    rng = np.random.default_rng(0)
    sizes = [(33, 17), (352, 352), (1, 1)]
    counts = [70, 300, 5]
    rows = [det_rows(rng, k) for k in counts]
    rows[0][3, 4] = np.nan                                                      # a NaN score, a NaN corner, classes no colour stands for
    rows[0][4, 1] = np.nan
    rows[0][5, 6] = -1
    rows[0][6, 6] = np.nan
    rows[0][7, 6] = 3e7
    rows[0][8, :4] = [0.9, 0.8, 0.1, 0.2]                                       # corners in the wrong order
    rows[0][9, :4] = [3e9, -3e9, 1e30, -1e30]                                   # clamped
    rows[1][0, 4:6] = [0.5, 0.3]                                                # the product is exactly the gate
    ann = viz.Annotator(palette=PAL, thickness=3, score_thres=0.15)
    dev = torch.device("cuda:0")
    out, begin, count, K = ann.boxes([torch.from_numpy(r) for r in rows], 0, sizes, dev)
    got = out.cpu().numpy().view(V.BOX)
    assert K == sum(counts) and list(count.cpu().numpy()) == counts
    want = np.concatenate([V.records(r, 0, h, w, np.float32(0.15), PAL, 3) for r, (h, w) in zip(rows, sizes)])
    assert got.tobytes() == want.tobytes()
    assert list(want["t"][3:8]) == [0] * 5 and want["t"][8] == 3 and want["t"][9] == 3 and want["t"][70] == 0
    assert (want["t"] == 0).sum() > 20 and (want["t"] == 3).sum() > 200
    tg = [np.concatenate([rng.integers(0, 20, (k, 1)), rng.uniform(0, 1, (k, 4))], 1).astype(np.float32) for k in (4, 0, 9)]
    out, _, _, K = ann.boxes([torch.from_numpy(t) for t in tg], 1, sizes, dev)
    want = np.concatenate([V.records(t, 1, h, w, 0, PAL, 3) for t, (h, w) in zip(tg, sizes)])
    assert K == 13 and out.cpu().numpy().view(V.BOX)[:13].tobytes() == want.tobytes() and (want["t"] == 3).all()
    # the segment form: rows that no segment covers keep what the record buffer held
    r = torch.from_numpy(np.concatenate(rows)).to(dev)
    b2, c2 = torch.tensor([0, 80, 370], dtype=torch.int32, device=dev), torch.tensor([60, 100, 5000], dtype=torch.int32, device=dev)
    out, _, _, K = ann.boxes((r, b2, c2), 0, sizes, dev)                        # the last segment is clipped to the capacity
    assert K == 375 and out.numel() == 375 * 20
    flat = np.concatenate(rows)
    want = np.zeros(375, V.BOX)
    for (b, c), (h, w) in zip(((0, 60), (80, 100), (370, 5)), sizes):
        want[b:b + c] = V.records(flat[b:b + c], 0, h, w, np.float32(0.15), PAL, 3)
    assert out.cpu().numpy().view(V.BOX).tobytes() == want.tobytes()


@pytest.mark.parametrize("k", [0, 1, WAVE - 1, WAVE, WAVE + 1, LIST - 1, LIST, LIST + 1, 300])
def test_box_counts_round_the_list_size(viz, k):
    """One image of 5 x 3 tiles (ragged on both sides), k boxes: the filter's wave boundary (64) and its pass size (the LDS list of 256
    records: 257 and 300 need a second pass, whose records must still win over the first's)."""
    rng = np.random.default_rng(k)
    h, w = 70, 150
    x = batch(rng, 1, h, w)
    rows = det_rows(rng, k)
    ann = viz.Annotator(palette=PAL, thickness=2, score_thres=0.15)
    buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(rows)], mean=MEAN, std=STD)
    ann.check()
    want = V.compose(x[0], V.records(rows, 0, h, w, np.float32(0.15), PAL, 2), mean=MEAN, std=STD)
    assert np.array_equal(cut(buf, desc)[0], want)


@pytest.mark.parametrize("t", [1, 2, 8])
def test_boxes_on_tile_and_image_borders(viz, t):
    h, w = 40, 140
    px = lambda x0, y0, x1, y1, c: [(x0 - 0.25) / w, (y0 - 0.25) / h, (x1 + 0.25) / w, (y1 + 0.25) / h, 0.9, 0.9, c]    # rounds to these pixels
    rows = np.array([px(TILE_W - 1, TILE_H - 1, 2 * TILE_W, 2 * TILE_H, 0), px(TILE_W, TILE_H, 2 * TILE_W - 1, 2 * TILE_H - 1, 1),
                     px(0, 0, w - 1, h - 1, 2), px(-5, -5, w + 4, h + 4, 3), px(w - 1, 0, w - 1, h - 1, 4), px(0, h - 1, w - 1, h - 1, 0),
                     px(TILE_W - t, 3, TILE_W + t - 1, 30, 1), px(10, TILE_H - t, 120, TILE_H + t, 2), px(-20, 5, 0, 9, 3), px(70, -9, 75, 0, 4)], np.float32)
    rng = np.random.default_rng(t)
    x = batch(rng, 1, h, w)
    ann = viz.Annotator(palette=PAL, thickness=t)
    recs = V.records(rows, 0, h, w, np.float32(0.15), PAL, t)
    assert (int(recs[0]["x0"]), int(recs[0]["y0"]), int(recs[0]["x1"]), int(recs[0]["y1"])) == (TILE_W - 1, TILE_H - 1, 2 * TILE_W, 2 * TILE_H)
    assert (recs["t"] == t).all()
    for order in (np.arange(len(rows)), np.arange(len(rows))[::-1].copy()):
        buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(rows[order])], mean=MEAN, std=STD)
        assert np.array_equal(cut(buf, desc)[0], V.compose(x[0], recs[order], mean=MEAN, std=STD))


def test_a_sheet_of_five_tiles_in_two_columns(viz):
    """The sixth cell and the gutters keep the background the sheet was filled with: the kernel writes its tiles' pixels only."""
    rng = np.random.default_rng(5)
    h, w = 21, 70
    x = batch(rng, 5, h, w)
    rows = [det_rows(rng, k) for k in (3, 0, 70, 1, 9)]
    ann = viz.Annotator(palette=PAL, thickness=1)
    ann.background, ann.gutter = 0xA5, 3
    buf, desc = ann.sheet(torch.from_numpy(x).cuda(), cols=2, dets=[torch.from_numpy(r) for r in rows], mean=MEAN, std=STD)
    ann.check()
    H, W = 3 * h + 4 * 3, 2 * w + 3 * 3
    assert (int(desc[0]["h"]), int(desc[0]["w"])) == (H, W) and buf.numel() == 3 * H * W
    want = np.full((H, W, 3), 0xA5, np.uint8)
    for i in range(5):
        y0, x0 = 3 + (i // 2) * (h + 3), 3 + (i % 2) * (w + 3)
        want[y0:y0 + h, x0:x0 + w] = V.compose(x[i], V.records(rows[i], 0, h, w, np.float32(0.15), PAL, 1), mean=MEAN, std=STD)
    got = cut(buf, desc)[0]
    assert np.array_equal(got, want)
    assert (got[3 + 2 * (h + 3):3 + 2 * (h + 3) + h, 3 + w + 3:3 + 2 * w + 3] == 0xA5).all()          # the untouched cell


@pytest.mark.parametrize("C", [0, 1, 2])
def test_uint8_originals_of_three_sizes_with_overlay(viz, C):
    rng = np.random.default_rng(10 + C)
    sizes = [(1, 1), (17, 33), (352, 352)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(3, DESC)
    off = 0
    for i, a in enumerate(imgs):
        desc[i] = (off, a.shape[0], a.shape[1])
        off += (a.size + 15) // 16 * 16
    src = np.zeros(off, np.uint8)
    for d, a in zip(desc, imgs):
        src[int(d["offset"]):int(d["offset"]) + a.size] = a.reshape(-1)
    rows = [det_rows(rng, k) for k in (2, 40, 300)]
    probs = [rng.uniform(0.3, 0.9, (C, h, w)).astype(np.float32) for h, w in sizes]
    for p in probs:
        p.reshape(-1)[::7] = 0.5                                               # exactly the threshold: untouched
    ann = viz.Annotator(palette=PAL, thickness=2, seg_channel=(1, 0))
    seg = None if C == 0 else [torch.from_numpy(p).cuda() for p in probs]
    buf, d2 = ann.annotate((torch.from_numpy(src).cuda(), desc), dets=[torch.from_numpy(r) for r in rows], seg_probs=seg)
    ann.check()
    assert (d2["offset"] % 16 == 0).all()
    for a, r, p, got in zip(imgs, rows, probs, cut(buf, d2)):
        h, w = a.shape[:2]
        assert np.array_equal(got, V.compose(a, V.records(r, 0, h, w, np.float32(0.15), PAL, 2), p, (1, 0))), (h, w)
    if C == 2:                                                                  # the planes as views of one buffer, as segeval.upsample returns them
        flat = torch.cat([torch.from_numpy(p).reshape(-1) for p in probs]).cuda()
        views, o = [], 0
        for h, w in sizes:
            views.append(flat[o:o + C * h * w].view(C, h, w))
            o += C * h * w
        buf2, d3 = ann.annotate((torch.from_numpy(src).cuda(), desc), dets=[torch.from_numpy(r) for r in rows], seg_probs=views)
        assert all(np.array_equal(a, b) for a, b in zip(cut(buf, d2), cut(buf2, d3)))   # the images: the bytes between them belong to nobody


def test_targets_alone_and_under_detections(viz):
    rng = np.random.default_rng(3)
    h, w = 48, 80
    x = batch(rng, 2, h, w)
    tg = [np.concatenate([rng.integers(1, 21, (k, 1)), rng.uniform(0.1, 0.9, (k, 2)), rng.uniform(0.05, 0.6, (k, 2))], 1).astype(np.float32) for k in (3, 0)]
    rows = [det_rows(rng, k) for k in (0, 6)]
    ann = viz.Annotator(palette=PAL, thickness=2)
    xd = torch.from_numpy(x).cuda()
    buf, desc = ann.annotate(xd, targets=[torch.from_numpy(t) for t in tg], mean=MEAN, std=STD)
    for i, got in enumerate(cut(buf, desc)):
        assert np.array_equal(got, V.compose(x[i], V.records(tg[i], 1, h, w, 0, PAL, 2), mean=MEAN, std=STD))
    tg[1] = tg[0].copy()
    rows[0] = det_rows(rng, 4)
    buf, desc = ann.annotate(xd, dets=[torch.from_numpy(r) for r in rows], targets=[torch.from_numpy(t) for t in tg], mean=MEAN, std=STD)
    for i, got in enumerate(cut(buf, desc)):
        recs = np.concatenate([V.records(tg[i], 1, h, w, 0, PAL, 2), V.records(rows[i], 0, h, w, np.float32(0.15), PAL, 2)])
        assert np.array_equal(got, V.compose(x[i], recs, mean=MEAN, std=STD))


def test_an_item_that_contradicts_its_source_is_reported_and_left_alone(viz):
    import ctypes
    from mobilenet_yolo_pytorch_amd._lib import call, query
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8)
    x = batch(rng, 3, 9, 20)
    items = np.zeros(3, viz.ITEM)
    for i in range(3):
        items[i] = (i * 640, 60, 0, 9, 20)
    items[1]["w"] = 19                                                          # not the batch's width
    dst = torch.full((3 * 640,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.zeros(query("mny_viz_ws_bytes", 3), dtype=torch.uint8, device=dev)
    xd, i_dev = torch.from_numpy(x).to(dev), torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    call("mny_viz_compose", p(xd), 9, 20, m, s, None, None, p(i_dev), 3, None, None, None, 0, None, 0, None, p(dst), p(ws),
         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    out = dst.cpu().numpy()
    assert int(ws[:4].cpu().numpy().view(np.int32)[0]) == 2
    assert (out[640:1280] == 0xA5).all() and (out[540:640] == 0xA5).all()
    for i in (0, 2):
        assert np.array_equal(out[i * 640:i * 640 + 540].reshape(9, 20, 3), V.denorm(x[i], MEAN, STD))


def test_the_complete_case_model_rows_to_annotated_images(viz):
    """Annotator on model.eval()(x) of the synthetic config equals the restatement on the same rows."""
    from mobilenet_yolo_pytorch_amd import synthetic, yolo
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = yolo(synthetic.VOC_CONFIG).to(dev).eval()
    x = synthetic.images(2, 352, 352, seed=3).to(dev)
    dets = model(x)
    assert len(dets) == 2 and all(d.shape[1] == 7 for d in dets)
    ann = viz.Annotator(thickness=2, score_thres=0.15)
    buf, desc = ann.annotate(x, dets=dets, mean=MEAN, std=STD)
    ann.check()
    drawn = 0
    for i, got in enumerate(cut(buf, desc)):
        recs = V.records(dets[i].cpu().numpy(), 0, 352, 352, np.float32(0.15), ann.palette, 2)
        drawn += int((recs["t"] > 0).sum())
        assert np.array_equal(got, V.compose(x[i].cpu().numpy(), recs, mean=MEAN, std=STD)), i
    assert drawn > 0
