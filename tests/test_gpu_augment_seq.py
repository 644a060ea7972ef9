"""Device-side blur / sharpen / noise stage (mny_aug_seq_batch, augment.SeqAugment, TrainAugment(seq=...)) against the numpy /
scipy restatement (tests/seq_ref.py).  imgaug and cv2 are not available: the stage is parity-unpinned against them and the header's
arithmetic is the specification.  Median, copies and the identities are compared byte for byte.  The fp32 ops are compared with the
fp64 value v of the restatement: wherever v is farther than 1e-3 from a half-integer the device byte is the rounded, clamped v,
inside that band it may differ by one, and the band may hold at most 2 % of the pixels (one pixel of an image under 100 pixels);
the inputs were chosen so that this holds on the restatement alone (tests/test_seq_cpu.py).
Every call goes through ctypes with src, dst and ws sized exactly inside larger allocations of sentinel bytes."""
import ctypes
import itertools
import random

import numpy as np
import pytest
import torch

import seq_ref as R

pytestmark = pytest.mark.gpu
GUARD = 4096
SENT = 0xA5


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import augment
    return augment


@pytest.fixture(scope="module")
def IMS():
    return [a for _, _, a in R.images(0)]


def layout(imgs, shift=None):
    """16-byte-rounded offsets (+ shift[i] bytes) -> (desc, src bytes with SENT in the gaps, covered mask)."""
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(len(imgs), DESC)
    off = 0
    for i, a in enumerate(imgs):
        desc[i] = (off + (shift[i] if shift else 0), a.shape[0], a.shape[1])
        off += (a.size + 15 + (16 if shift and shift[i] else 0)) // 16 * 16
    total = int(desc["offset"][-1]) + imgs[-1].size                   # src ends with the last image, nothing after it
    buf = np.full(total, SENT, np.uint8)
    cover = np.zeros(total, bool)
    for d, a in zip(desc, imgs):
        buf[d["offset"]:d["offset"] + a.size] = a.reshape(-1)
        cover[d["offset"]:d["offset"] + a.size] = True
    return desc, buf, cover


def run(M, imgs, rec, desc=None, buf=None, cover=None, max_hw=None):
    """-> (per-image device results, status, per-image op-0 intermediates of ws).  Asserts that no byte outside the images changed."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    if desc is None:
        desc, buf, cover = layout(imgs)
    n, total = len(desc), len(buf)
    mh, mw = max_hw or (int(desc["h"].max()), int(desc["w"].max()))
    wsb = query("mny_aug_seq_ws_bytes", n, total, mh, mw)
    assert wsb >= 256 + total
    dev = torch.device("cuda:0")
    big_src = torch.full((GUARD + total + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_dst = torch.full((GUARD + total + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_ws = torch.full((GUARD + wsb + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_src[GUARD:GUARD + total] = torch.from_numpy(buf).to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    s_dev = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).to(dev)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    call("mny_aug_seq_batch", p(big_src, GUARD), p(d_dev), p(s_dev), n, mh, mw, p(big_dst, GUARD), p(big_ws, GUARD),
         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    dst, ws, src_after = big_dst.cpu().numpy(), big_ws.cpu().numpy(), big_src.cpu().numpy()
    assert np.all(dst[:GUARD] == SENT) and np.all(dst[GUARD + total:] == SENT), "dst: bytes outside the buffer were written"
    assert np.all(ws[:GUARD] == SENT) and np.all(ws[GUARD + wsb:] == SENT), "ws: bytes outside the buffer were written"
    assert np.array_equal(src_after[GUARD:GUARD + total], buf) and np.all(src_after[:GUARD] == SENT) and np.all(src_after[GUARD + total:] == SENT)
    body = dst[GUARD:GUARD + total]
    assert np.all(body[~cover] == SENT), "dst: bytes between the images were written"
    status = int(ws[GUARD:GUARD + 4].view(np.int32)[0])
    mid = ws[GUARD + 256:GUARD + 256 + total]
    cut = lambda b: [b[d["offset"]:d["offset"] + 3 * d["h"] * d["w"]].reshape(d["h"], d["w"], 3) if d["offset"] >= 0 and d["h"] > 0 else None
                     for d in desc]
    return cut(body), status, cut(mid)


def rounded_ok(dev, ref, v, what):
    """The comparison rule of the fp32 ops on one image."""
    bad, _ = R.mismatch(dev, ref, v)
    assert bad == 0, "%s: %d values break the rule (max difference %d)" % (what, bad, int(np.abs(dev.astype(int) - ref.astype(int)).max()))


def same_for_all(M, imgs, ops):
    return M.seq_records([ops(i) for i in range(len(imgs))])


@pytest.mark.parametrize("k", [3, 5])
def test_median_exact(M, IMS, k):
    out, status, _ = run(M, IMS, same_for_all(M, IMS, lambda i: [(M.SEQ_MEDIAN, k)]))
    assert status == 0
    for i, a in enumerate(IMS):
        assert np.array_equal(out[i], R.median(a, k)[0]), (i, a.shape)


@pytest.mark.parametrize("name", ["no_op", "gauss_delta", "sharpen_alpha0", "noise_scale0"])
def test_identities_exact(M, IMS, name):
    ops = {"no_op": lambda i: [], "gauss_delta": lambda i: [(M.SEQ_GAUSS, 0.05)], "sharpen_alpha0": lambda i: [(M.SEQ_SHARPEN, 0.0, 1.1)],
           "noise_scale0": lambda i: [(M.SEQ_NOISE, 0.0, i % 2, 99 + i)]}[name]
    rec = same_for_all(M, IMS, ops)
    assert np.all(rec["n_ops"] == (0 if name == "no_op" else 1))
    out, status, _ = run(M, IMS, rec)
    assert status == 0
    for i, a in enumerate(IMS):
        assert np.array_equal(out[i], a), (i, a.shape)


@pytest.mark.parametrize("sigma", R.GAUSS_SIGMAS)
def test_gaussian_rounded(M, IMS, sigma):
    refs = [R.gaussian(a, R.taps(sigma)) for a in IMS]
    assert R.band_ok([v for _, v in refs])
    out, status, _ = run(M, IMS, same_for_all(M, IMS, lambda i: [(M.SEQ_GAUSS, sigma)]))
    assert status == 0
    for i, (ref, v) in enumerate(refs):
        rounded_ok(out[i], ref, v, "gauss %g image %d %s" % (sigma, i, IMS[i].shape))


@pytest.mark.parametrize("alpha,lightness", R.SHARPEN_PARAMS)
def test_sharpen_rounded(M, IMS, alpha, lightness):
    refs = [R.sharpen(a, *R.sharpen_coeffs(alpha, lightness)) for a in IMS]
    assert R.band_ok([v for _, v in refs])
    assert any((ref == 255).any() and (ref == 0).any() for ref, _ in refs)             # the clamps are reached
    out, status, _ = run(M, IMS, same_for_all(M, IMS, lambda i: [(M.SEQ_SHARPEN, alpha, lightness)]))
    assert status == 0
    for i, (ref, v) in enumerate(refs):
        rounded_ok(out[i], ref, v, "sharpen %g %g image %d %s" % (alpha, lightness, i, IMS[i].shape))


@pytest.mark.parametrize("scale,per", list(itertools.product(R.NOISE_SCALES, [False, True])))
def test_noise_rounded(M, IMS, scale, per):
    key = lambda i: R.noise_key(i)[0] | (R.noise_key(i)[1] << 32)
    refs = [R.noise(a, scale, per, R.noise_key(i)) for i, a in enumerate(IMS)]
    assert R.band_ok([v for _, v in refs])
    out, status, _ = run(M, IMS, same_for_all(M, IMS, lambda i: [(M.SEQ_NOISE, scale, per, key(i))]))
    assert status == 0
    for i, (ref, v) in enumerate(refs):
        rounded_ok(out[i], ref, v, "noise %g %s image %d %s" % (scale, per, i, IMS[i].shape))
    if scale > 1:
        assert any(not np.array_equal(o, a) for o, a in zip(out, IMS))


def test_noise_semantics(M):
    a = np.full((64, 67, 3), 128, np.uint8)
    imgs = [a, a, a, a]
    rec = M.seq_records([[(M.SEQ_NOISE, 7.65, False, 5)], [(M.SEQ_NOISE, 7.65, True, 5)], [(M.SEQ_NOISE, 7.65, False, 5)],
                         [(M.SEQ_NOISE, 7.65, False, 5 + (1 << 40))]])
    out, status, _ = run(M, imgs, rec)
    assert status == 0
    d = [o.astype(int) - 128 for o in out]
    assert all(0 < o.min() and o.max() < 255 for o in out)                              # nothing clips
    assert np.array_equal(d[0][..., 0], d[0][..., 1]) and np.array_equal(d[0][..., 0], d[0][..., 2]) and d[0].any()
    assert not np.array_equal(d[1][..., 0], d[1][..., 1]) and not np.array_equal(d[1][..., 0], d[1][..., 2])
    assert np.array_equal(d[1][..., 0], d[0][..., 0])                                   # channel 0 takes z0 in both modes
    assert np.array_equal(d[0], d[2])                                                   # same key, same size: same field
    assert not np.array_equal(d[0], d[3])
    assert 6.5 < d[1].std() < 8.8                                                       # 7.65 up to rounding and 12864 samples


def one_op(M, kind, i):
    return {M.SEQ_GAUSS: (M.SEQ_GAUSS, 0.8), M.SEQ_MEDIAN: (M.SEQ_MEDIAN, 5 if i % 2 else 3), M.SEQ_SHARPEN: (M.SEQ_SHARPEN, 0.037, 1.0),
            M.SEQ_NOISE: (M.SEQ_NOISE, 3.0, bool(i % 2), 4242 + i)}[kind]


def test_chains(M):
    """Every ordered pair of distinct kinds on a one-tile and a many-tile image.  Op 0's uint8 result stays in ws (ws + 256 + offset): it
    is held to op 0's rule, and dst to op 1's rule on that intermediate; where the intermediate equals the restatement's, which it must
    for an exact op 0, this is the restatement applied twice."""
    r = np.random.RandomState(7)
    kinds = (M.SEQ_GAUSS, M.SEQ_MEDIAN, M.SEQ_SHARPEN, M.SEQ_NOISE)
    pairs = [(a, b) for a in kinds for b in kinds if a != b]
    assert len(pairs) == 12
    imgs, ops = [], []
    for shape in ((17, 33), (130, 257)):
        for a, b in pairs:
            imgs.append(r.randint(0, 256, size=shape + (3,)).astype(np.uint8))
            ops.append([one_op(M, a, len(ops)), one_op(M, b, len(ops))])
    rec = M.seq_records(ops)
    assert np.all(rec["n_ops"] == 2)
    out, status, mid = run(M, imgs, rec)
    assert status == 0
    for i, a in enumerate(imgs):
        ref0, v0 = R.apply_op(a, rec[i], int(rec[i]["op"][0]))
        rounded_ok(mid[i], ref0, v0, "chain %s image %d, op 0" % (ops[i], i))
        if rec[i]["op"][0] == M.SEQ_MEDIAN:
            assert np.array_equal(mid[i], ref0)
        ref1, v1 = R.apply_op(mid[i], rec[i], int(rec[i]["op"][1]))
        rounded_ok(out[i], ref1, v1, "chain %s image %d, op 1" % (ops[i], i))
        if np.array_equal(mid[i], ref0):
            twice, v = R.apply(a, rec[i])
            rounded_ok(out[i], twice, v, "chain %s image %d, applied twice" % (ops[i], i))


def test_launch_to_launch(M, IMS):
    rec = M.SeqAugment(seed=4, p=0.9, device="cuda:0").plan(len(IMS))
    assert {0, 1, 2} <= set(rec["n_ops"].tolist())
    a, sa, _ = run(M, IMS, rec)
    b, sb, _ = run(M, IMS, rec)
    assert sa == sb == 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for i, im in enumerate(IMS):                                                        # and the mixed batch is right
        ref, v = R.apply(im, rec[i])
        if rec[i]["n_ops"] == 0:
            assert np.array_equal(a[i], im)
        elif rec[i]["n_ops"] == 1:
            rounded_ok(a[i], ref, v, "mixed image %d" % i)


def _bad(M, case):
    """-> (record of the malformed image, its shape, byte shift, declared-maximum override)."""
    rec = M.seq_records([[(M.SEQ_MEDIAN, 3)]])[0]
    shape, shift = (17, 33), 0
    if case == "too_high":
        shape = (20, 30)
    elif case == "too_wide":
        shape = (12, 70)
    elif case == "misaligned":
        shift = 2
    elif case == "three_ops":
        rec["n_ops"] = 3
    elif case == "negative_ops":
        rec["n_ops"] = -1
    elif case == "unknown_op":
        rec["op"][0] = 4
    elif case == "repeated_op":
        rec["n_ops"], rec["op"] = 2, (M.SEQ_MEDIAN, M.SEQ_MEDIAN)
    elif case == "median_4":
        rec["median_k"] = 4
    elif case == "nan_tap":
        rec["op"][0], rec["taps"] = M.SEQ_GAUSS, (0, 0.25, np.nan, 0.25, 0)
    elif case == "inf_sharpen":
        rec["op"][0], rec["sharpen_c"], rec["sharpen_s"] = M.SEQ_SHARPEN, np.inf, -0.1
    elif case == "nan_noise":
        rec["op"][0], rec["noise_scale"] = M.SEQ_NOISE, np.nan
    else:
        raise KeyError(case)
    return rec, shape, shift


@pytest.mark.parametrize("case", ["too_high", "too_wide", "misaligned", "three_ops", "negative_ops", "unknown_op", "repeated_op", "median_4",
                                  "nan_tap", "inf_sharpen", "nan_noise"])
def test_status_word(M, case):
    r = np.random.RandomState(3)
    bad_rec, shape, shift = _bad(M, case)
    imgs = [r.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in ((17, 33), shape, (10, 67), (16, 64))]
    rec = M.seq_records([[(M.SEQ_MEDIAN, 5)], [], [(M.SEQ_GAUSS, 0.7), (M.SEQ_MEDIAN, 3)], [(M.SEQ_SHARPEN, 0.05, 1.0)]])
    rec[1] = bad_rec
    desc, buf, cover = layout(imgs, shift=[0, shift, 0, 0])
    out, status, _ = run(M, imgs, rec, desc, buf, cover, max_hw=(17, 67))
    assert status == 2
    assert not out[1].any()                                                             # written as zeros, sentinels checked in run()
    for i in (0, 2, 3):
        ref, v = R.apply(imgs[i], rec[i])
        if i == 0:
            assert np.array_equal(out[i], ref)
        else:
            rounded_ok(out[i], ref, v, "%s: neighbour %d" % (case, i))


@pytest.mark.parametrize("case", ["zero_height", "negative_offset"])
def test_status_word_of_an_item_that_names_no_bytes(M, case):
    """Such an item is reported and nothing is written for it; its slot in dst keeps the sentinel."""
    r = np.random.RandomState(5)
    imgs = [r.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in ((17, 33), (9, 9), (10, 67))]
    rec = M.seq_records([[(M.SEQ_MEDIAN, 5)], [(M.SEQ_MEDIAN, 3)], [(M.SEQ_NOISE, 2.0, True, 8)]])
    desc, buf, cover = layout(imgs)
    slot = slice(int(desc["offset"][1]), int(desc["offset"][1]) + imgs[1].size)
    cover[slot] = False
    if case == "zero_height":
        desc["h"][1] = 0
    else:
        desc["offset"][1] = -16
    out, status, _ = run(M, imgs, rec, desc, buf, cover)
    assert status == 2
    assert np.array_equal(out[0], R.apply(imgs[0], rec[0])[0])
    rounded_ok(out[2], *R.apply(imgs[2], rec[2]), "%s: neighbour 2" % case)


def test_status_reports_the_lowest_index(M):
    r = np.random.RandomState(6)
    imgs = [r.randint(0, 256, size=(8, 9, 3)).astype(np.uint8) for _ in range(5)]
    rec = M.seq_records([[(M.SEQ_MEDIAN, 3)]] * 5)
    rec["median_k"][[2, 4]] = 7
    out, status, _ = run(M, imgs, rec)
    assert status == 3 and not out[2].any() and not out[4].any()
    assert all(np.array_equal(out[i], R.median(imgs[i], 3)[0]) for i in (0, 1, 3))


def test_bad_arguments(M):
    from mobilenet_yolo_pytorch_amd._lib import MnyError, call, query
    assert query("mny_aug_seq_ws_bytes", 0, 100, 8, 8) == 0 and query("mny_aug_seq_ws_bytes", 4, 0, 8, 8) == 0
    assert query("mny_aug_seq_ws_bytes", 4, 100, 0, 8) == 0 and query("mny_aug_seq_ws_bytes", 4, 100, 8, 8) >= 356
    t = torch.zeros(1024, dtype=torch.uint8, device="cuda:0")
    p = lambda o=0: ctypes.c_void_p(t.data_ptr() + o)
    with pytest.raises(MnyError, match="dst must not be src"):
        call("mny_aug_seq_batch", p(), p(512), p(512), 1, 8, 8, p(), p(256), None)
    with pytest.raises(MnyError, match="null pointer"):
        call("mny_aug_seq_batch", p(), p(512), p(512), 1, 8, 8, None, p(256), None)
    with pytest.raises(MnyError, match="aligned"):
        call("mny_aug_seq_batch", p(), p(512), p(512), 1, 8, 8, p(130), p(256), None)


# ---- through the public interface -----------------------------------------------------------------------------------
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def small_groups():
    from mobilenet_yolo_pytorch_amd import synthetic
    shapes = [(64, 67), (48, 60), (57, 41), (64, 64), (50, 67), (61, 45), (40, 52)]
    photos = synthetic.photos(shapes, seed=2)
    tg = [t.numpy() for t in synthetic.targets(len(shapes), seed=3, boxes_per_image=2)]
    m = list(zip(photos, tg))
    return [[m[0]], [m[1]], m[2:6], [m[6]]]                             # three single images and one 4-image mosaic


def test_train_augment_with_a_fixed_median_stage(M):
    groups = small_groups()
    ks = [3, 5, 3, 5, 5, 3, 5]
    mk = lambda **kw: M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=random.Random(21), **kw)
    aug = mk(seq=M.SeqAugment.fixed([[(M.SEQ_MEDIAN, k)] for k in ks]))
    images, targets, count = aug(groups)
    aug.check()
    flat = [m for g in groups for m in g]
    blurred = [(R.median(im, k)[0], t) for (im, t), k in zip(flat, ks)]
    assert any(not np.array_equal(b[0], f[0]) for b, f in zip(blurred, flat))
    want_groups = [[blurred[0]], [blurred[1]], blurred[2:6], [blurred[6]]]
    plain = mk()
    w_images, w_targets, w_count = plain(want_groups)
    plain.check()
    assert tuple(images.shape) == (4, 3, 32, 32) and count == w_count == 7
    assert torch.equal(images, w_images)                                                # bit for bit
    assert len(targets) == len(w_targets) == 4 and all(torch.equal(a, b) for a, b in zip(targets, w_targets))
    untouched = mk()(groups)
    assert not torch.equal(untouched[0], images)                                        # and the stage did something


def test_train_augment_without_seq_is_unchanged(M):
    groups = small_groups()
    a = M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=random.Random(21), seq=None)(groups)
    b = M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=random.Random(21))(groups)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]


def test_train_augment_with_drawn_seq_keeps_targets_and_random_state(M):
    groups = small_groups()
    r0, r1 = random.Random(33), random.Random(33)
    with_seq = M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=r0, seq=M.SeqAugment(seed=1, p=1.0))
    a = with_seq(groups)
    with_seq.check()
    b = M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=r1)(groups)
    assert r0.getstate() == r1.getstate() and a[2] == b[2] and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[0].shape == b[0].shape and not torch.equal(a[0], b[0]) and torch.isfinite(a[0]).all()


def test_check_raises_on_a_malformed_record(M):
    rec = M.seq_records([[(M.SEQ_MEDIAN, 3)]] * 7)
    rec["median_k"][3] = 9
    aug = M.TrainAugment([[32, 32]], MEAN, STD, 1.5, rng=random.Random(1), seq=M.SeqAugment.fixed(rec))
    aug(small_groups())
    with pytest.raises(RuntimeError, match="image 3"):
        aug.check()
