"""Device-side random perspective (mny_aug_warp_batch, augment.RandomPerspective, TrainAugment(warp=...)) against the numpy fp64
restatement (tests/warp_ref.py), which tests/test_warp_ref_cpu.py pins to Pillow's Image.transform(PERSPECTIVE): every comparison is
BYTE FOR BYTE, nothing takes a tolerance.  Kernel calls go through ctypes with src, dst and ws sized exactly inside larger allocations
of sentinel bytes."""
import ctypes
import random

import numpy as np
import pytest
import torch

import augment_ref as A
import augment_seg_ref as S
import seq_ref
import warp_ref as W

pytestmark = pytest.mark.gpu
GUARD = 4096
SENT = 0xA5
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 33), (65, 67), (375, 500)]       # 3 * 33 and 3 * 67 are no multiples of 4
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import augment
    return augment


def kinds(h, w):
    """name -> (c[0..7], identity flag): every record kind of the issue for an image of size (h, w)."""
    return {
        "identity_flag": ((1, 0, 2.0, 0, 1, -1.0, 0, 0), 1),                               # the flag wins over the coefficients: a copy
        "identity_coeffs": (W.IDENTITY_C, 0),
        "integer_shift": ((1, 0, 1.0, 0, 1, -1.0, 0, 0), 0),
        "half_pixel_shift": ((1, 0, 0.5, 0, 1, -0.5, 0, 0), 0),
        "quarter_turn": (W.coeffs(W.matrix(h, w, degrees=90.0)), 0),
        "rotation": (W.coeffs(W.matrix(h, w, degrees=33.7)), 0),
        "scale_half": (W.coeffs(W.matrix(h, w, scale=0.5)), 0),
        "scale_two": (W.coeffs(W.matrix(h, w, scale=2.0)), 0),
        "shear": (W.coeffs(W.matrix(h, w, shear_x=10.0, shear_y=-7.0)), 0),
        "perspective": (W.coeffs(W.matrix(h, w, degrees=-12.0, scale=0.9, px=0.3 / w, py=-0.2 / h)), 0),
        "perspective_steep": (W.coeffs(W.matrix(h, w, scale=1.2, px=-0.6 / w, py=0.3 / h, tx=0.55)), 0),
        "all_outside": ((1, 0, 10.0 * w + 5, 0, 1, 0, 0, 0), 0),
    }


@pytest.fixture(scope="module")
def batch(M):
    """Every (size, kind) pair in one batch: images, id maps, records, and the restatement's answers, computed once."""
    imgs, segs, rec, names = [], [], [], []
    for si, (h, w) in enumerate(SIZES):
        for ki, (name, (c, ident)) in enumerate(kinds(h, w).items()):
            imgs.append(W.image(h, w, 100 * si + ki))
            segs.append(W.image(h, w, 100 * si + ki + 50, channels=1) + (ki % 2))        # ids 0..5; half the maps hold no background
            r = np.zeros((), M.WARP)
            r["c"], r["identity"] = c, ident
            rec.append(r)
            names.append("%s %dx%d" % (name, h, w))
    rec = np.array(rec, M.WARP)
    rec_rgb, rec_id = rec.copy(), rec.copy()
    rec_rgb["fill"] = W.FILL
    want_rgb = [a if r["identity"] else W.warp_rgb(a, r["c"]) for a, r in zip(imgs, rec)]
    want_id = [a if r["identity"] else W.warp_id(a, r["c"]) for a, r in zip(segs, rec)]
    return dict(imgs=imgs, segs=segs, rec_rgb=rec_rgb, rec_id=rec_id, want_rgb=want_rgb, want_id=want_id, names=names)


def layout(arrs, shift=None):
    """16-byte-rounded offsets (+ shift[i] bytes) -> (desc, src bytes with SENT in the gaps, covered mask)."""
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(len(arrs), DESC)
    off = 0
    for i, a in enumerate(arrs):
        desc[i] = (off + (shift[i] if shift else 0), a.shape[0], a.shape[1])
        off += (a.size + 15 + (16 if shift and shift[i] else 0)) // 16 * 16
    total = int(desc["offset"][-1]) + arrs[-1].size                   # src ends with the last image, nothing after it
    buf = np.full(total, SENT, np.uint8)
    cover = np.zeros(total, bool)
    for d, a in zip(desc, arrs):
        buf[d["offset"]:d["offset"] + a.size] = a.reshape(-1)
        cover[d["offset"]:d["offset"] + a.size] = True
    return desc, buf, cover


def run(arrs, rec, channels, shift=None, max_hw=None):
    """-> (per-image device results, status).  Asserts that no byte outside the images changed and that src is intact."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    desc, buf, cover = layout(arrs, shift)
    n, total = len(desc), len(buf)
    mh, mw = max_hw or (int(desc["h"].max()), int(desc["w"].max()))
    wsb = query("mny_aug_warp_ws_bytes", n, channels, mh, mw)
    assert wsb >= 4
    dev = torch.device("cuda:0")
    big_src = torch.full((GUARD + total + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_dst = torch.full((GUARD + total + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_ws = torch.full((GUARD + wsb + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_src[GUARD:GUARD + total] = torch.from_numpy(buf).to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    w_dev = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).to(dev)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    call("mny_aug_warp_batch", p(big_src, GUARD), p(d_dev), p(w_dev), n, channels, mh, mw, p(big_dst, GUARD), p(big_ws, GUARD),
         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    dst, ws, src_after = big_dst.cpu().numpy(), big_ws.cpu().numpy(), big_src.cpu().numpy()
    assert np.all(dst[:GUARD] == SENT) and np.all(dst[GUARD + total:] == SENT), "dst: bytes outside the buffer were written"
    assert np.all(ws[:GUARD] == SENT) and np.all(ws[GUARD + wsb:] == SENT), "ws: bytes outside the buffer were written"
    assert np.array_equal(src_after[GUARD:GUARD + total], buf) and np.all(src_after[:GUARD] == SENT) and np.all(src_after[GUARD + total:] == SENT)
    body = dst[GUARD:GUARD + total]
    assert np.all(body[~cover] == SENT), "dst: bytes between the images were written"
    status = int(ws[GUARD:GUARD + 4].view(np.int32)[0])
    return [body[d["offset"]:d["offset"] + a.size].reshape(a.shape) for d, a in zip(desc, arrs)], status


def test_kernel_rgb_bilinear_every_size_and_kind(batch):
    out, status = run(batch["imgs"], batch["rec_rgb"], 3)
    assert status == 0
    for o, want, name in zip(out, batch["want_rgb"], batch["names"]):
        assert np.array_equal(o, want), (name, int(np.count_nonzero(o != want)))
    whole = {n: o for n, o in zip(batch["names"], out)}
    assert np.all(whole["all_outside 375x500"] == 127) and np.all(whole["all_outside 1x1"] == 127)
    assert np.any(whole["perspective 375x500"] == 127) and np.any(whole["perspective 375x500"] != 127)
    again, status = run(batch["imgs"], batch["rec_rgb"], 3)                                 # launch to launch
    assert status == 0 and all(np.array_equal(a, b) for a, b in zip(out, again))


def test_kernel_id_map_nearest_every_size_and_kind(batch):
    out, status = run(batch["segs"], batch["rec_id"], 1)
    assert status == 0
    for o, want, name in zip(out, batch["want_id"], batch["names"]):
        assert np.array_equal(o, want), (name, int(np.count_nonzero(o != want)))
    whole = {n: o for n, o in zip(batch["names"], out)}
    assert not whole["all_outside 375x500"].any() and whole["identity_flag 375x500"].any()
    again, status = run(batch["segs"], batch["rec_id"], 1)
    assert status == 0 and all(np.array_equal(a, b) for a, b in zip(out, again))


def test_the_batch_exercises_both_paths_and_the_tails(batch):
    c = batch["rec_rgb"]["c"]
    div = (c[:, 6] != 0) | (c[:, 7] != 0)
    assert 8 <= div.sum() <= len(c) - 8                                # the division path next to affine items
    assert any(a.size % 4 for a in batch["imgs"]) and any(a.size % 4 for a in batch["segs"]) and any(a.shape[0] * a.shape[1] > 1024 for a in batch["imgs"])


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("case", ["misaligned", "too_high", "too_wide", "nan_coefficient", "inf_coefficient"])
def test_status_word(M, case, channels):
    """Items 1 and 3 are malformed: the word names the lower one, both are written as zeros, the neighbours are right."""
    shapes = [(17, 33), (20, 30) if case == "too_high" else (12, 70) if case == "too_wide" else (17, 33), (10, 67), (9, 9), (16, 64)]
    arrs = [W.image(h, w, 7 + i, channels=channels) + (channels == 1) for i, (h, w) in enumerate(shapes)]
    rec = np.zeros(len(arrs), M.WARP)
    for r, (h, w) in zip(rec, shapes):
        r["c"], r["fill"] = W.coeffs(W.matrix(h, w, degrees=20.0, scale=0.9, px=0.2 / w)), (W.FILL if channels == 3 else 0)
    shift = [0, 2 if case == "misaligned" else 0, 0, 0, 0]
    if case == "nan_coefficient":
        rec["c"][1][4] = np.nan
    elif case == "inf_coefficient":
        rec["c"][1][7] = -np.inf
    rec["c"][3][0] = np.nan
    out, status = run(arrs, rec, channels, shift=shift, max_hw=(17, 67))
    assert status == 2
    assert not out[1].any() and not out[3].any()                       # sentinels around them are checked in run()
    ref = W.warp_rgb if channels == 3 else W.warp_id
    for i in (0, 2, 4):
        assert np.array_equal(out[i], ref(arrs[i], rec["c"][i])), (case, i)


def test_status_word_of_an_item_that_names_no_bytes(M):
    """A side of zero or a negative offset: reported, nothing written for it."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    from mobilenet_yolo_pytorch_amd.prep import DESC
    dev = torch.device("cuda:0")
    img = W.image(9, 9, 1)
    for field, value in (("h", 0), ("offset", -16), ("w", 16384)):
        desc = np.zeros(2, DESC)
        desc[0], desc[1] = (0, 9, 9), (256, 9, 9)
        desc[field][0] = value
        rec = np.zeros(2, M.WARP)
        rec["c"], rec["fill"] = W.coeffs(W.matrix(9, 9, degrees=45.0)), W.FILL
        src = torch.full((1024,), SENT, dtype=torch.uint8, device=dev)
        src[256:256 + img.size] = torch.from_numpy(img.reshape(-1)).to(dev)
        dst = torch.full((1024,), SENT, dtype=torch.uint8, device=dev)
        ws = torch.zeros(query("mny_aug_warp_ws_bytes", 2, 3, 9, 9), dtype=torch.uint8, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        d_dev, w_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev), torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        call("mny_aug_warp_batch", p(src), p(d_dev), p(w_dev), 2, 3, 9, 9, p(dst), p(ws), None)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert int(ws[:4].view(torch.int32).item()) == 1, field
        assert np.array_equal(got[256:256 + img.size].reshape(img.shape), W.warp_rgb(img, rec["c"][1])), field
        assert np.all(got[:256] == SENT) and np.all(got[256 + img.size:] == SENT), field


def test_bad_arguments(M):
    from mobilenet_yolo_pytorch_amd._lib import MnyError, call
    t = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    p = lambda o=0: ctypes.c_void_p(t.data_ptr() + o)
    with pytest.raises(MnyError, match="dst must not be src"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 3, 8, 8, p(), p(256), None)
    with pytest.raises(MnyError, match="null pointer"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 3, 8, 8, None, p(256), None)
    with pytest.raises(MnyError, match="channels"):
        call("mny_aug_warp_batch", p(), p(512), p(640), 1, 4, 8, 8, p(128), p(256), None)


# ---- through the public interface -----------------------------------------------------------------------------------
FULL = dict(degrees=25.0, translate=0.1, scale=0.5, shear=8.0, perspective=3e-4, p=0.85)


def test_run_device_on_a_drawn_plan(M):
    from mobilenet_yolo_pytorch_amd.prep import DESC
    r = np.random.RandomState(2)
    shapes = [(int(r.randint(1, 200)), int(r.randint(1, 200))) for _ in range(14)] + [(1, 1), (200, 3)]
    imgs = [W.image(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    warp = M.RandomPerspective(12, **FULL)
    plan = warp.plan(shapes)
    assert 0 < plan["identity"].sum() < 16 and np.all(plan["records"]["c"][~plan["identity"]][:, 6:] != 0)
    desc, buf, _ = layout(imgs)
    dst = warp.run_device(torch.from_numpy(buf).to("cuda:0"), desc, plan, channels=3)
    warp.check()
    got = dst.cpu().numpy()
    for d, a, rec in zip(desc, imgs, plan["records"]):
        want = a if rec["identity"] else W.warp_rgb(a, rec["c"])
        assert np.array_equal(got[d["offset"]:d["offset"] + a.size].reshape(a.shape), want), a.shape
    segs = [W.image(h, w, 90 + i, channels=1) + 1 for i, (h, w) in enumerate(shapes)]
    sdesc, sbuf, _ = layout(segs)
    sdst = warp.run_device(torch.from_numpy(sbuf).to("cuda:0"), sdesc, plan["records"], channels=1).cpu().numpy()
    warp.check()
    for d, a, rec in zip(sdesc, segs, plan["records"]):
        want = a if rec["identity"] else W.warp_id(a, rec["c"])
        assert np.array_equal(sdst[d["offset"]:d["offset"] + a.size].reshape(a.shape), want), a.shape
    assert np.all(plan["records"]["fill"] == 127)                      # run_device(channels=1) worked on a copy


def voc_groups():
    """Three single images and one 4-image mosaic, VOC-shaped."""
    from mobilenet_yolo_pytorch_amd import synthetic
    shapes = [(375, 500), (500, 375), (375, 500), (375, 500), (500, 375), (375, 500), (333, 500)]
    photos = synthetic.photos(shapes, seed=5)
    tg = [t.numpy() for t in synthetic.targets(len(shapes), seed=6, boxes_per_image=4)]
    m = list(zip(photos, tg))
    return [[m[0]], m[1:5], [m[5]], [m[6]]]


def regroup(groups, flat):
    it = iter(flat)
    return [[next(it) for _ in g] for g in groups]


@pytest.fixture(scope="module")
def voc(M):
    """The batch, its drawn warp plan, and the restatement's warped images and boxes."""
    groups = voc_groups()
    flat = [m for g in groups for m in g]
    plan = M.RandomPerspective(31, **FULL).plan([im.shape[:2] for im, _ in flat])
    assert not plan["identity"].all()
    warped = []
    for (im, t), rec, mat in zip(flat, plan["records"], plan["matrices"]):
        warped.append((im, t) if rec["identity"] else (W.warp_rgb(im, rec["c"]), W.boxes(t, mat, im.shape[0], im.shape[1])))
    return groups, plan, regroup(groups, warped)


SCALE = 2.1610954191879452


def test_train_augment_with_warp_equals_the_restated_chain(M, voc):
    groups, wplan, warped = voc
    size = (352, 352)
    aug = M.TrainAugment([list(size)], MEAN, STD, SCALE, rng=random.Random(3), warp=M.RandomPerspective(31, **FULL))
    images, targets, count = aug(groups)
    aug.check()
    samples, drawn, n = A.plan(random.Random(3), [[(im.shape[0], im.shape[1], t) for im, t in g] for g in warped], SCALE, 1000, [list(size)])
    assert count == n == 7 and drawn == size
    got = images.cpu().numpy()
    for i, (g, s) in enumerate(zip(warped, samples)):
        ref = A.collate([A.render_u8([im for im, _ in g], s, 1000)], size, MEAN, STD)[0]
        assert np.array_equal(got[i], ref), i
        assert np.array_equal(targets[i].numpy(), s["target"].numpy()), i
    plain = M.TrainAugment([list(size)], MEAN, STD, SCALE, rng=random.Random(3))(groups)
    assert not torch.equal(plain[0], images)                             # and the stage did something


def test_all_identity_warp_is_bit_equal_to_none(M, voc):
    groups = voc[0]
    mk = lambda **kw: M.TrainAugment([[320, 320]], MEAN, STD, SCALE, rng=random.Random(8), **kw)
    a = mk(warp=M.RandomPerspective(1, degrees=0, translate=0, scale=0, shear=0, perspective=0))
    ia, ta, ca = a(groups)
    a.check()
    ib, tb, cb = mk()(groups)
    assert torch.equal(ia, ib) and ca == cb and len(ta) == len(tb) and all(torch.equal(x, y) for x, y in zip(ta, tb))
    gated = mk(warp=M.RandomPerspective(1, p=0.0, **{k: v for k, v in FULL.items() if k != "p"}))
    ic, tc, _ = gated(groups)
    assert torch.equal(ic, ib) and all(torch.equal(x, y) for x, y in zip(tc, tb))


def test_seq_runs_before_warp(M, voc):
    """With a fixed median stage (exact) in front: the batch is the plain chain on warp(median(image))."""
    groups, wplan, _ = voc
    flat = [m for g in groups for m in g]
    ks = [3, 5, 3, 5, 5, 3, 5]
    both = []
    for (im, t), k, rec, mat in zip(flat, ks, wplan["records"], wplan["matrices"]):
        b = seq_ref.median(im, k)[0]
        both.append((b, t) if rec["identity"] else (W.warp_rgb(b, rec["c"]), W.boxes(t, mat, im.shape[0], im.shape[1])))
    mk = lambda **kw: M.TrainAugment([[288, 288]], MEAN, STD, SCALE, rng=random.Random(13), **kw)
    aug = mk(seq=M.SeqAugment.fixed([[(M.SEQ_MEDIAN, k)] for k in ks]), warp=M.RandomPerspective(31, **FULL))
    images, targets, _ = aug(groups)
    aug.check()
    w_images, w_targets, _ = mk()(regroup(groups, both))
    assert torch.equal(images, w_images) and all(torch.equal(a, b) for a, b in zip(targets, w_targets))
    other = [(seq_ref.median(W.warp_rgb(im, rec["c"]), k)[0], t) for (im, t), k, rec in zip(flat, ks, wplan["records"])]
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(both, other))      # the two orders differ on this batch


def test_decoder_path_warps_what_the_decoder_wrote(M):
    """Encoded streams through decoder= and warp=: the batch of the array path on the same decoded pixels (tests/golden/jpeg_cases.npz)."""
    import os
    from mobilenet_yolo_pytorch_amd import jpeg
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
    names = ["ok_420_37x53", "ok_422_37x53", "ok_444_37x53", "ok_gray_37x53", "ok_qtables", "ok_420_17x33"]
    tg = lambda k: np.array([[k % 3, 0.5, 0.5, 0.4 + 0.05 * (k % 4), 0.5], [1, 0.3, 0.6, 0.2, 0.3]], np.float32)
    shape = [[0, 1, 2, 3], [4], [5]]
    arrays = [[(z["p_" + names[k]], tg(k)) for k in g] for g in shape]
    streams = [[(z["s_" + names[k]].tobytes(), tg(k)) for k in g] for g in shape]
    r0, r1 = random.Random(4), random.Random(4)
    mk = lambda rng, **kw: M.TrainAugment([[64, 64]], MEAN, STD, 2.0, canvas=200, rng=rng, warp=M.RandomPerspective(5, **FULL), **kw)
    a, b = mk(r0), mk(r1, decoder=jpeg.JpegDecoder(threads=2))
    xa, ta, ca = a(arrays)
    xb, tb, cb = b(streams)
    a.check(), b.check(), b.decoder.check()
    assert torch.equal(xa, xb) and ca == cb == 6 and all(torch.equal(x, y) for x, y in zip(ta, tb)) and r0.getstate() == r1.getstate()
    plain = M.TrainAugment([[64, 64]], MEAN, STD, 2.0, canvas=200, rng=random.Random(4))(arrays)
    assert not torch.equal(plain[0], xa)


def test_check_reports_the_warp_status(M, voc):
    groups = voc[0]
    aug = M.TrainAugment([[96, 96]], MEAN, STD, SCALE, rng=random.Random(1), warp=M.RandomPerspective(31, **FULL))
    plan = aug.plan(groups)
    stage, offsets = aug.pack(groups)
    plan["items"]["offset"] = offsets
    plan["warp"]["records"]["c"][2][3] = np.nan
    aug.warp.run_device(stage.to("cuda:0"), plan["items"], plan["warp"])
    with pytest.raises(RuntimeError, match="warp augment: image 2"):
        aug.check()


def test_seg_config_warps_the_id_maps_with_the_images_coefficients(M):
    from mobilenet_yolo_pytorch_amd import synthetic
    from mobilenet_yolo_pytorch_amd.prep import DESC
    r = np.random.RandomState(4)
    n, C, size = 6, 3, 96
    shapes = [(int(r.randint(120, 300)), int(r.randint(120, 300))) for _ in range(n)]
    photos = synthetic.photos(shapes, seed=4)
    tg = [t.numpy() for t in synthetic.targets(n, seed=5, boxes_per_image=3)]
    ids = [np.kron(r.randint(0, C + 2, size=(6, 5)), np.ones((h // 6 + 1, w // 5 + 1))).astype(np.uint8)[:h, :w] for h, w in shapes]
    groups = [[(p, t, s)] for p, t, s in zip(photos, tg, ids)]
    seg_full = dict(FULL, scale=0.2)                                    # keeps the cropped geometry above the 6x6 grid
    wplan = M.RandomPerspective(9, **seg_full).plan(shapes)
    assert not plan_all_identity(wplan)
    w_ids = [s if rec["identity"] else W.warp_id(s, rec["c"]) for s, rec in zip(ids, wplan["records"])]
    w_img = [p if rec["identity"] else W.warp_rgb(p, rec["c"]) for p, rec in zip(photos, wplan["records"])]
    w_tg = [t if rec["identity"] else W.boxes(t, m, *hw) for t, rec, m, hw in zip(tg, wplan["records"], wplan["matrices"], shapes)]
    assert any(not np.array_equal(a, b) for a, b in zip(w_ids, ids))
    # the id maps alone, through run_device on the packed maps
    aug = M.TrainAugment([[size, size]], [0.5] * 3, [1, 1, 1], 1.3, rng=random.Random(5), seg_classes=C, warp=M.RandomPerspective(9, **seg_full))
    stage, offsets = aug.pack_seg(groups)
    desc = np.zeros(n, DESC)
    desc["offset"], desc["h"], desc["w"] = offsets, [s[0] for s in shapes], [s[1] for s in shapes]
    got = aug.warp.run_device(stage.to("cuda:0"), desc, wplan, channels=1).cpu().numpy()
    for o, s, want in zip(offsets, ids, w_ids):
        assert np.array_equal(got[o:o + s.size].reshape(s.shape), want)
    # end to end
    images, targets, count, maps = aug(groups)
    aug.check()
    samples, drawn, _ = A.plan(random.Random(5), [[(h, w, t)] for (h, w), t in zip(shapes, w_tg)], 1.3, 1000, [[size, size]])
    ref = S.batch_maps(w_ids, [s["members"][0] for s in samples], C, drawn)
    assert np.array_equal(maps.cpu().numpy(), ref)
    assert all(np.array_equal(t.numpy(), s["target"].numpy()) for t, s in zip(targets, samples))
    plain = M.TrainAugment([[size, size]], [0.5] * 3, [1, 1, 1], 1.3, rng=random.Random(5))([[(p, t)] for p, t in zip(w_img, w_tg)])
    assert torch.equal(plain[0], images)
    # the all-identity instance leaves the seg maps those of warp=None
    mk = lambda **kw: M.TrainAugment([[size, size]], [0.5] * 3, [1, 1, 1], 1.3, rng=random.Random(6), seg_classes=C, **kw)
    a = mk(warp=M.RandomPerspective(1, degrees=0, translate=0, scale=0, shear=0, perspective=0))(groups)
    b = mk()(groups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def plan_all_identity(wplan):
    return bool(wplan["identity"].all())
