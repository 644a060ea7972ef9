"""Class-name labels on the device (mny_viz_labels, mny_viz_compose_labels behind viz.Annotator(names=)) against the numpy restatement
of include/mnyolo.h (tests/vizlabel_ref.py, which tests/test_vizlabel_ref_cpu.py holds to Pillow and to hand-worked answers).  Exact
equality everywhere: the label records byte for byte, the images pixel for pixel.  The kernels take the strip atlas as data, so most
cases use random uint8 strips: every blend level, no font."""
import ctypes
import io

import numpy as np
import pytest
import torch

import viz_ref as V
import vizlabel_ref as VL

pytestmark = pytest.mark.gpu
LIST, WAVE = 256, 64                                                             # csrc/viz.hip: records per pass of the LDS list; the scan's wave
TILE_W, TILE_H = 64, 16                                                          # the pixel tile of a workgroup
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PAL = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255]], np.uint8)
THR = np.float32(0.15)
FG = (250, 240, 10)


@pytest.fixture(scope="module")
def viz():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import viz
    return viz


def annotator(viz, atlas, strips, h, **kw):
    """An Annotator whose strips are the given ones, not a font's."""
    ann = viz.Annotator(palette=PAL, names=[""] * (len(strips) - 12), text_rgb=FG, **kw)
    ann.atlas, ann.strips, ann.text_h = atlas, np.ascontiguousarray(strips, np.int32), h
    return ann


def det_rows(rng, k, n_cls=20, lo=-0.2, hi=1.2):
    a, b = rng.uniform(lo, hi, (k, 2)), rng.uniform(lo, hi, (k, 2))
    return np.concatenate([np.minimum(a, b), np.maximum(a, b), rng.uniform(0.3, 1.0, (k, 2)), rng.integers(0, n_cls, (k, 1))], 1).astype(np.float32)


def px_rows(boxes, h, w):
    """(x0, y0, x1, y1, cls) in pixels -> detection rows whose corners round to exactly these pixels."""
    return np.array([[(x0 - 0.25) / w, (y0 - 0.25) / h, (x1 + 0.25) / w, (y1 + 0.25) / h, 0.9, 0.9, c] for x0, y0, x1, y1, c in boxes], np.float32)


def batch(rng, n, h, w):
    u = rng.integers(-3, 259, (n, 3, h, w)).astype(np.float32) / np.float32(255)
    return ((u - np.asarray(MEAN, np.float32).reshape(1, 3, 1, 1)) / np.asarray(STD, np.float32).reshape(1, 3, 1, 1)).astype(np.float32)


def cut(buf, desc):
    b = buf.cpu().numpy()
    return [b[int(d["offset"]):int(d["offset"]) + 3 * int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"]), 3) for d in desc]


def want_image(ann, x, rows, mode=0, probs=None):
    """The restatement for one image: x fp32 [3,H,W] (normalised) or uint8 [H,W,3]."""
    h, w = x.shape[-2:] if x.dtype != np.uint8 else x.shape[:2]
    recs = V.records(rows, mode, h, w, np.float32(ann.score_thres), ann.palette, ann.thickness)
    labs = VL.labels(rows, mode, recs, w, ann.strips, len(ann.names), ann.text_h, ann.with_score, ann.label_bg, ann.label_targets, ann.text_rgb)
    return VL.compose(x, recs, labs, ann.atlas, ann.strips, probs, ann.seg_channel, MEAN, STD), recs, labs


def test_label_records_equal_the_restatement(viz):
    rng = np.random.default_rng(0)
    n_names, h = 7, 9
    atlas, strips = VL.random_atlas(rng, n_names, h, empty=(2,))                # class 2 has the empty name
    sizes = [(33, 17), (352, 352), (1, 1)]
    counts = [70, 300, 5]
    rows = [det_rows(rng, k, n_cls=12) for k in counts]                         # classes 7..11 have no name: their index in decimal
    rows[0][3, 4] = np.nan                                                      # a NaN score
    rows[0][4, 1] = np.nan
    rows[0][5, 6] = -1
    rows[0][6, 6] = np.nan
    rows[0][7, 6] = 3e7
    rows[0][8, 6] = n_names                                                     # the first class without a name
    rows[0][9, 6] = 16777215                                                    # eight digits
    rows[0][10, 6] = 2                                                          # the empty name
    rows[0][11, 6] = 6.75                                                       # (int)cls
    rows[0][12, 4:6] = [0.5, 0.009]                                             # 0.0045 -> "0.00"
    rows[0][13, 4:6] = [1.0, 1.0]                                               # "1.00"
    rows[0][14, 4:6] = [4.0, 3.0]                                               # clamped: "9.99"
    rows[0][15, 4:6] = [0.5, 0.25]                                              # 0.125: the tie goes to the even digit, "0.12"
    rows[1][0, 4:6] = [0.5, 0.008]                                              # the product is exactly the gate
    thr = np.float32(np.float32(0.5) * np.float32(0.008))
    dev = torch.device("cuda:0")
    for score, filled in ((True, True), (False, False)):
        ann = annotator(viz, atlas, strips, h, thickness=3, score_thres=float(thr), label="name_score" if score else "name", label_bg=filled)
        box, lab, begin, count, K = ann.records([torch.from_numpy(r) for r in rows], 0, sizes, dev)
        assert K == sum(counts) and lab.numel() == K * 48
        got = lab.cpu().numpy().view(VL.LABEL)
        recs = [V.records(r, 0, hh, ww, thr, PAL, 3) for r, (hh, ww) in zip(rows, sizes)]
        assert box.cpu().numpy().tobytes() == np.concatenate(recs).tobytes()
        want = np.concatenate([VL.labels(r, 0, b, ww, strips, n_names, h, score, filled, True, FG) for r, b, (hh, ww) in zip(rows, recs, sizes)])
        assert got.tobytes() == want.tobytes()
        assert list(want["n"][3:8]) == [0] * 5 and want["n"][70] == 0 and (want["n"] > 0).sum() > 300
        extra = 5 if score else 0
        assert list(want["n"][8:12]) == [1 + extra, 8 + extra, 1 + extra, 1 + extra] and want["seq"][11][0] == 6
        assert score or want["lw"][10] == 4                                      # the empty name: padding alone
        if score:
            digits = lambda i: [int(s) - n_names for s in want["seq"][i][int(want["n"][i]) - 5:int(want["n"][i])]]
            assert digits(12) == [VL.SPACE, 0, VL.DOT, 0, 0] and digits(13) == [VL.SPACE, 1, VL.DOT, 0, 0]
            assert digits(14) == [VL.SPACE, 9, VL.DOT, 9, 9] and digits(15) == [VL.SPACE, 0, VL.DOT, 1, 2]
    # targets: labelled with the name alone, or not at all
    tg = [np.concatenate([rng.integers(0, 12, (k, 1)), rng.uniform(0, 1, (k, 4))], 1).astype(np.float32) for k in (4, 0, 9)]
    for on in (True, False):
        ann = annotator(viz, atlas, strips, h, thickness=3, label_targets=on)
        box, lab, _, _, K = ann.records([torch.from_numpy(t) for t in tg], 1, sizes, dev)
        recs = [V.records(t, 1, hh, ww, 0, PAL, 3) for t, (hh, ww) in zip(tg, sizes)]
        want = np.concatenate([VL.labels(t, 1, b, ww, strips, n_names, h, True, True, on, FG) for t, b, (hh, ww) in zip(tg, recs, sizes)])
        assert K == 13 and lab.cpu().numpy()[:13 * 48].tobytes() == want.tobytes()
        assert (want["n"] > 0).all() == on and (want["n"] <= 2).all()
    # the segment form: rows that no segment covers keep the empty record
    ann = annotator(viz, atlas, strips, h, thickness=3, score_thres=float(thr))
    r = torch.from_numpy(np.concatenate(rows)).to(dev)
    b2, c2 = torch.tensor([0, 80, 370], dtype=torch.int32, device=dev), torch.tensor([60, 100, 5000], dtype=torch.int32, device=dev)
    box, lab, _, _, K = ann.records((r, b2, c2), 0, sizes, dev)
    flat = np.concatenate(rows)
    want = np.zeros(375, VL.LABEL)
    for (b, c), (hh, ww) in zip(((0, 60), (80, 100), (370, 5)), sizes):
        rc = V.records(flat[b:b + c], 0, hh, ww, thr, PAL, 3)
        want[b:b + c] = VL.labels(flat[b:b + c], 0, rc, ww, strips, n_names, h, True, True, True, FG)
    assert K == 375 and lab.cpu().numpy().tobytes() == want.tobytes() and (want["n"][60:80] == 0).all() and (want["n"][:60] > 0).any()


@pytest.mark.parametrize("k", [0, 1, WAVE - 1, WAVE, WAVE + 1, LIST - 1, LIST, LIST + 1, 300])
def test_record_counts_round_the_list_size(viz, k):
    """One image of 5 x 3 tiles (ragged on both sides), k labelled boxes: the filter's wave boundary and its pass size; labels of a second
    pass must still blend over what the first left.  Unfilled labels on odd k: every label depends on what lies beneath it."""
    rng = np.random.default_rng(k)
    h, w = 70, 150
    x = batch(rng, 1, h, w)
    rows = det_rows(rng, k)
    atlas, strips = VL.random_atlas(rng, 20, 7, max_w=24)
    ann = annotator(viz, atlas, strips, 7, thickness=2, label_bg=k % 2 == 0)
    buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(rows)], mean=MEAN, std=STD)
    ann.check()
    want, recs, labs = want_image(ann, x[0], rows)
    assert np.array_equal(cut(buf, desc)[0], want)
    if k:
        assert not np.array_equal(want, V.compose(x[0], recs, mean=MEAN, std=STD))   # the labels are there


@pytest.mark.parametrize("size", [(1, 1), (6, 11), (33, 17), (40, 130), (130, 40), (352, 352)])
@pytest.mark.parametrize("filled", [True, False])
def test_image_sizes_from_one_pixel_to_many_tiles(viz, size, filled):
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    k = 300 if h == 352 else 40
    x = batch(rng, 1, h, w)
    rows = det_rows(rng, k)
    atlas, strips = VL.random_atlas(rng, 20, 20 if h == 352 else 5)
    ann = annotator(viz, atlas, strips, 20 if h == 352 else 5, thickness=1, label_bg=filled)
    buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(rows)], mean=MEAN, std=STD)
    ann.check()
    assert np.array_equal(cut(buf, desc)[0], want_image(ann, x[0], rows)[0])


@pytest.mark.parametrize("filled", [True, False])
@pytest.mark.parametrize("t", [1, 3])
def test_labels_in_tiles_their_outlines_miss(viz, filled, t):
    """Boxes whose top edges lie on rows 16 k and left edges on columns 64 k: the label sits in the tile above, which the outline never
    touches.  A box that swallows whole tiles with its label (hung inside: the box starts above the image) in one of them.  Labels
    clipped at every edge of the image.  Overlapping labels, in both orders."""
    H, W = 80, 200
    hh = 6
    boxes = [(TILE_W, TILE_H, TILE_W + 30, TILE_H + 9, 0), (2 * TILE_W, 3 * TILE_H, 2 * TILE_W + 5, 3 * TILE_H + 20, 1), (10, 2 * TILE_H, 50, 2 * TILE_H + 3, 2),
              (3 * TILE_W - 1, 4 * TILE_H, 3 * TILE_W + 3, 4 * TILE_H + 9, 3), (TILE_W - 3, TILE_H + hh, TILE_W + 9, TILE_H + hh + 4, 4),
              (-20, -4, W + 20, H + 20, 5), (-30, -30, W + 30, H + 30, 6), (1, 1, W - 2, H - 2, 7), (0, hh - 1, 198, 70, 8),
              (W - 6, 30, W - 1, 40, 9), (W - 1, 50, W + 30, 60, 10), (-40, 60, -1, 70, 11), (-40, 20, 3, 28, 12), (60, H - 1, 90, H + 9, 13),
              (70, H + 3, 90, H + 9, 14), (100, -9, 120, 0, 15), (20, 40, 60, 60, 16), (24, 42, 64, 62, 17), (22, 41, 62, 61, 18), (128, 40, 140, 50, 19)]
    rows = px_rows(boxes, H, W)
    rng = np.random.default_rng(7 + t)
    x = batch(rng, 1, H, W)
    atlas, strips = VL.random_atlas(rng, 20, hh, max_w=30)
    ann = annotator(viz, atlas, strips, hh, thickness=t, label_bg=filled)
    recs = V.records(rows, 0, H, W, THR, PAL, t)
    assert (int(recs[0]["x0"]), int(recs[0]["y0"])) == (TILE_W, TILE_H) and (recs["t"] == t).all()
    labs = VL.labels(rows, 0, recs, W, strips, 20, hh, True, filled, True, FG)
    assert int(labs[0]["ly"]) == TILE_H - hh and int(labs[5]["ly"]) == -4 and int(labs[6]["ly"]) == -30 and int(labs[9]["lx"]) < W - 6 and int(labs[11]["lx"]) == 0
    for order in (np.arange(len(rows)), np.arange(len(rows))[::-1].copy()):
        buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(rows[order])], mean=MEAN, std=STD)
        assert np.array_equal(cut(buf, desc)[0], want_image(ann, x[0], rows[order])[0])
    one = px_rows([boxes[0]], H, W)                                             # alone: nothing else lists the record in the tile above
    buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(one)], mean=MEAN, std=STD)
    want = want_image(ann, x[0], one)[0]
    assert np.array_equal(cut(buf, desc)[0], want)
    assert not np.array_equal(want[TILE_H - hh:TILE_H, TILE_W:TILE_W + 8], V.denorm(x[0], MEAN, STD)[TILE_H - hh:TILE_H, TILE_W:TILE_W + 8])
    inner = px_rows([boxes[5]], H, W)                                           # alone: its label lies in a tile wholly inside the box
    buf, desc = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(inner)], mean=MEAN, std=STD)
    assert np.array_equal(cut(buf, desc)[0], want_image(ann, x[0], inner)[0])


def originals(rng, sizes):
    from mobilenet_yolo_pytorch_amd.prep import DESC
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    desc = np.zeros(len(sizes), DESC)
    off = 0
    for i, a in enumerate(imgs):
        desc[i] = (off, a.shape[0], a.shape[1])
        off += (a.size + 15) // 16 * 16
    src = np.zeros(off, np.uint8)
    for d, a in zip(desc, imgs):
        src[int(d["offset"]):int(d["offset"]) + a.size] = a.reshape(-1)
    return imgs, src, desc


def test_a_sheet_of_five_unequal_tiles(viz):
    """Each label clips to its tile; the gutters and the rest of every cell keep the background the sheet was filled with."""
    rng = np.random.default_rng(5)
    sizes = [(21, 70), (9, 30), (30, 66), (1, 1), (17, 90)]
    imgs, src, desc = originals(rng, sizes)
    rows = [det_rows(rng, k) for k in (6, 3, 70, 2, 9)]
    rows[1][:, :4] = [0.5, 0.1, 1.3, 0.8]                                      # labels that would run over the right edge of a small tile
    atlas, strips = VL.random_atlas(rng, 20, 8)
    ann = annotator(viz, atlas, strips, 8, thickness=1)
    ann.background, ann.gutter = 0xA5, 3
    buf, d1 = ann.sheet((torch.from_numpy(src).cuda(), desc), cols=2, dets=[torch.from_numpy(r) for r in rows])
    ann.check()
    ch, cw = 30, 90
    H, W = 3 * ch + 4 * 3, 2 * cw + 3 * 3
    assert (int(d1[0]["h"]), int(d1[0]["w"])) == (H, W)
    want = np.full((H, W, 3), 0xA5, np.uint8)
    for i, (h, w) in enumerate(sizes):
        y0, x0 = 3 + (i // 2) * (ch + 3), 3 + (i % 2) * (cw + 3)
        want[y0:y0 + h, x0:x0 + w] = want_image(ann, imgs[i], rows[i])[0]
    assert np.array_equal(cut(buf, d1)[0], want)


@pytest.mark.parametrize("C", [1, 2])
def test_batch_and_originals_under_the_seg_overlay(viz, C):
    """The overlay comes after the labels and dims their pixels too."""
    rng = np.random.default_rng(20 + C)
    atlas, strips = VL.random_atlas(rng, 20, 10)
    ann = annotator(viz, atlas, strips, 10, thickness=2, seg_channel=(1, 0))
    sizes = [(17, 33), (48, 80), (1, 1)]
    imgs, src, desc = originals(rng, sizes)
    rows = [det_rows(rng, k, lo=0.0, hi=1.0) for k in (5, 30, 2)]
    probs = [rng.uniform(0.3, 0.9, (C, h, w)).astype(np.float32) for h, w in sizes]
    buf, d2 = ann.annotate((torch.from_numpy(src).cuda(), desc), dets=[torch.from_numpy(r) for r in rows], seg_probs=[torch.from_numpy(p).cuda() for p in probs])
    ann.check()
    for a, r, p, got in zip(imgs, rows, probs, cut(buf, d2)):
        want, recs, labs = want_image(ann, a, r, probs=p)
        assert np.array_equal(got, want), a.shape
    recs = V.records(rows[1], 0, 48, 80, THR, PAL, 2)
    labs = VL.labels(rows[1], 0, recs, 80, strips, 20, 10, True, True, True, FG)
    plain = VL.compose(imgs[1], recs, labs, atlas, strips)
    inside = np.zeros((48, 80), bool)
    for l in labs:
        inside[max(int(l["ly"]), 0):int(l["ly"]) + 10, int(l["lx"]):int(l["lx"]) + int(l["lw"])] = True
    assert (cut(buf, d2)[1][inside] != plain[inside]).any()                    # dimmed label pixels
    x = batch(rng, 2, 48, 80)
    tg = [np.concatenate([rng.integers(0, 20, (k, 1)), rng.uniform(0.1, 0.9, (k, 2)), rng.uniform(0.05, 0.6, (k, 2))], 1).astype(np.float32) for k in (3, 1)]
    dr = [det_rows(rng, k) for k in (4, 6)]
    pb = [rng.uniform(0.3, 0.9, (C, 48, 80)).astype(np.float32) for _ in range(2)]
    buf, d3 = ann.annotate(torch.from_numpy(x).cuda(), dets=[torch.from_numpy(r) for r in dr], targets=[torch.from_numpy(t) for t in tg],
                           seg_probs=[torch.from_numpy(p).cuda() for p in pb], mean=MEAN, std=STD)
    for i, got in enumerate(cut(buf, d3)):                                      # targets first, detections over them, the same order for the labels
        rt, rd = V.records(tg[i], 1, 48, 80, 0, PAL, 2), V.records(dr[i], 0, 48, 80, THR, PAL, 2)
        lt = VL.labels(tg[i], 1, rt, 80, strips, 20, 10, True, True, True, FG)
        ld = VL.labels(dr[i], 0, rd, 80, strips, 20, 10, True, True, True, FG)
        want = VL.compose(x[i], np.concatenate([rt, rd]), np.concatenate([lt, ld]), atlas, strips, pb[i], (1, 0), MEAN, STD)
        assert np.array_equal(got, want), i


def test_null_labels_and_no_names_are_the_annotator_of_before(viz):
    """mny_viz_compose_labels with labels = NULL equals mny_viz_compose byte for byte, and Annotator() without names equals the
    restatement of the stage without text (tests/viz_ref.py), as before."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    h, w, n = 70, 150, 3
    x = batch(rng, n, h, w)
    rows = [det_rows(rng, k) for k in (300, 0, 65)]
    plain = viz.Annotator(palette=PAL, thickness=2)
    assert plain.names is None
    xd = torch.from_numpy(x).to(dev)
    buf, desc = plain.annotate(xd, dets=[torch.from_numpy(r) for r in rows], mean=MEAN, std=STD)
    plain.check()
    imgs = cut(buf, desc)
    for i in range(n):
        assert np.array_equal(imgs[i], V.compose(x[i], V.records(rows[i], 0, h, w, THR, PAL, 2), mean=MEAN, std=STD))
    rec, begin, count, K = plain.boxes([torch.from_numpy(r) for r in rows], 0, [(h, w)] * n, dev)
    items = np.zeros(n, viz.ITEM)
    for i in range(n):
        items[i] = (int(desc[i]["offset"]), 3 * w, 0, h, w)
    i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    outs = []
    for entry, more in (("mny_viz_compose", ()), ("mny_viz_compose_labels", (None, None, None))):
        dst = torch.full((buf.numel(),), 0x5A, dtype=torch.uint8, device=dev)
        ws = torch.zeros(query("mny_viz_ws_bytes", n), dtype=torch.uint8, device=dev)
        call(entry, p(xd), h, w, m, s, None, None, p(i_dev), n, p(rec), p(begin), p(count), K, None, 0, None, p(dst), p(ws), *more, st)
        assert int(ws[:4].cpu().numpy().view(np.int32)[0]) == 0
        outs.append(dst.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(cut(torch.from_numpy(outs[0]), desc), imgs))


def test_end_to_end_model_rows_to_labelled_files(viz):
    """Annotator(names=VOC) with Pillow's built-in font on model.eval()(x) equals the restatement on the same rows, and the JPEG
    files of those images equal Pillow's files of the restated images."""
    Image = pytest.importorskip("PIL.Image")
    from mobilenet_yolo_pytorch_amd import jpeg, synthetic, yolo
    from oracle import procedural
    dev = torch.device("cuda:0")
    model = yolo(synthetic.VOC_CONFIG)
    procedural.fill_state_dict_(model)
    model = model.to(dev).eval()
    for hs in model.yolo_losses:
        hs.val_conf = 0.01
    x = synthetic.images(2, 64, 64, seed=3).to(dev)
    dets = model(x)
    assert len(dets) == 2 and all(d.shape[1] == 7 for d in dets)
    ann = viz.Annotator(thickness=1, score_thres=0.01, names=synthetic.VOC_NAMES)
    assert ann.text_h == 11 and set(np.unique(ann.atlas)) == {0, 255}
    buf, desc = ann.annotate(x, dets=dets, mean=MEAN, std=STD)
    ann.check()
    files = jpeg.JpegEncoder(quality=75, subsampling="4:2:0", device=dev)(buf, desc)
    labelled = 0
    for i, got in enumerate(cut(buf, desc)):
        want, recs, labs = want_image(ann, x[i].cpu().numpy(), dets[i].cpu().numpy())
        labelled += int((labs["n"] == 6).sum())
        print("image %d: %d rows, %d labels" % (i, len(recs), int((labs["n"] > 0).sum())))
        assert np.array_equal(got, want), i
        b = io.BytesIO()
        Image.fromarray(want).save(b, "JPEG", quality=75, subsampling="4:2:0")
        assert files[i] == b.getvalue(), i
    assert labelled > 0
