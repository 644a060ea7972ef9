"""Baseline JPEG decode on the device (mny_jpeg_pixels_batch behind jpeg.JpegDecoder, and the decoder= path of BatchPrep and
TrainAugment) against Pillow's pixels as stored in tests/golden/jpeg_cases.npz (tools/gen_golden_jpeg.py).  All of the pixel
arithmetic is integer work, so every comparison is byte for byte.  Direct calls go through ctypes with dst and ws sized exactly
inside larger allocations of sentinel bytes."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 4096
SENT = 0xA5
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def CASES():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    hashes = {n: str(z["h_" + n]) for n in names if "h_" + n in z.files}       # cases pinned by the SHA-256 of Pillow's RGB
    return {n: (z["s_" + n].tobytes(), z["p_" + n] if "p_" + n in z.files else None) for n in names}, str(z["voc_like_sha256"]), hashes


def same(img, n, CASES):
    if n in CASES[2]:
        return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == CASES[2][n]
    return np.array_equal(img, CASES[0][n][1])


def ok_names(CASES):
    return sorted(n for n in CASES[0] if n.startswith("ok_"))


def cut(buf, desc):
    return [buf[int(d["offset"]):int(d["offset"]) + 3 * int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"]), 3) for d in desc]


def pixels_direct(J, streams, desc=None, max_hw=None, shift=None):
    """Host stage into numpy buffers, then mny_jpeg_pixels_batch on sentinel-filled device buffers.
    -> (dst bytes, desc, status, covered mask); asserts that nothing outside dst and ws was written."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    from mobilenet_yolo_pytorch_amd.prep import DESC
    coef, items = J.decode_host(streams, threads=4)
    n = len(streams)
    if desc is None:
        desc = np.zeros(n, DESC)
        off = 0
        for i, it in enumerate(items):
            desc[i] = (off + (shift[i] if shift else 0), it["h"], it["w"])
            off += (3 * int(it["h"]) * int(it["w"]) + 15 + (16 if shift and shift[i] else 0)) // 16 * 16
    total = int(desc["offset"][-1]) + 3 * int(desc["h"][-1]) * int(desc["w"][-1])     # dst ends with the last image
    cover = np.zeros(total, bool)
    for d in desc:
        cover[int(d["offset"]):int(d["offset"]) + 3 * int(d["h"]) * int(d["w"])] = True
    mh, mw = max_hw or (int(desc["h"].max()), int(desc["w"].max()))
    wsb = query("mny_jpeg_ws_bytes", n, coef.size)
    assert wsb >= 256 + coef.size
    dev = torch.device("cuda:0")
    big_dst = torch.full((GUARD + total + GUARD,), SENT, dtype=torch.uint8, device=dev)
    big_ws = torch.full((GUARD + wsb + GUARD,), SENT, dtype=torch.uint8, device=dev)
    c_dev = torch.from_numpy(coef).to(dev)
    i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    call("mny_jpeg_pixels_batch", p(c_dev), p(i_dev), n, p(big_dst, GUARD), p(d_dev), mh, mw, p(big_ws, GUARD),
         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    dst, ws = big_dst.cpu().numpy(), big_ws.cpu().numpy()
    assert np.all(dst[:GUARD] == SENT) and np.all(dst[GUARD + total:] == SENT), "dst: bytes outside the buffer were written"
    assert np.all(ws[:GUARD] == SENT) and np.all(ws[GUARD + wsb:] == SENT), "ws: bytes outside the buffer were written"
    body = dst[GUARD:GUARD + total]
    assert np.all(body[~cover] == SENT), "dst: bytes between the images were written"
    return body, desc, int(ws[GUARD:GUARD + 4].view(np.int32)[0]), items


def test_pixel_parity_direct_call_with_guards(J, CASES):
    names = ok_names(CASES)
    assert len(names) == 39
    body, desc, status, items = pixels_direct(J, [CASES[0][n][0] for n in names])
    assert status == 0
    for n, img in zip(names, cut(body, desc)):
        assert same(img, n, CASES), n


def test_pixel_parity_through_the_decoder(J, CASES):
    names = ok_names(CASES)
    dec = J.JpegDecoder(threads=4, fallback=lambda b: pytest.fail("no stream of this batch needs the fallback"))
    src, desc, mh, mw = dec([CASES[0][n][0] for n in names])
    dec.check()
    assert (desc["offset"] % 16 == 0).all() and mh == int(desc["h"].max()) and mw == int(desc["w"].max())
    assert src.device.type == "cuda" and src.dtype == torch.uint8
    assert (dec.statuses == 0).all()
    for n, img in zip(names, cut(src.cpu().numpy(), desc)):
        assert same(img, n, CASES), n
    for k, n in enumerate(names):                                               # one by one: bytearray, memoryview and array members
        s = CASES[0][n][0]
        member = [s, bytearray(s), memoryview(s), np.frombuffer(s, np.uint8)][k % 4]
        src1, desc1, _, _ = dec([member])
        assert same(cut(src1.cpu().numpy(), desc1)[0], n, CASES), n
    assert dec.sizes([CASES[0][n][0] for n in names]) == [(int(d["h"]), int(d["w"])) for d in desc]


def test_voc_like_by_hash(J, CASES):
    s = open(os.path.join(GOLDEN, "voc_like.jpg"), "rb").read()
    dec = J.JpegDecoder(threads=2)
    src, desc, mh, mw = dec([s, s])
    dec.check()
    assert (mh, mw) == (375, 500)
    for img in cut(src.cpu().numpy(), desc):
        assert hashlib.sha256(img.tobytes()).hexdigest() == CASES[1]


def test_fallback_fills_what_the_decoder_does_not_take(J, CASES):
    from mobilenet_yolo_pytorch_amd import MnyError
    names = ["ok_420_37x53", "route_progressive", "ok_gray_9x7", "route_cmyk", "ok_444_17x33"]
    by_stream = {CASES[0][n][0]: CASES[0][n][1] for n in names}
    asked = []

    def stub(b):
        asked.append(b)
        return by_stream[b]

    dec = J.JpegDecoder(threads=3, fallback=stub)
    src, desc, mh, mw = dec([CASES[0][n][0] for n in names])
    assert asked == [CASES[0]["route_progressive"][0], CASES[0]["route_cmyk"][0]]
    assert list(dec.statuses) == [J.OK, J.PROGRESSIVE, J.OK, J.COLORSPACE, J.OK]
    assert int(dec._status.item()) == 2                                         # 1 + the lowest index the kernels left alone
    dec.check()                                                                 # ... which the fallback filled: not an error
    for n, img in zip(names, cut(src.cpu().numpy(), desc)):
        assert np.array_equal(img, CASES[0][n][1]), n

    def absent(b):                                                              # what fallback=None does where Pillow is not installed
        raise MnyError("image needs the fallback decoder and Pillow is not installed")

    with pytest.raises(MnyError, match="Pillow is not installed"):
        J.JpegDecoder(fallback=absent)([CASES[0][n][0] for n in names])
    # a hostile stream: either it decodes (pixels defined) or it is routed; never a crash
    hostile = [n for n in sorted(CASES[0]) if n.startswith("hostile_")]
    dec2 = J.JpegDecoder(fallback=lambda b: np.zeros((53, 37, 3), np.uint8))
    src2, desc2, _, _ = dec2([CASES[0][n][0] for n in hostile])
    dec2.check()
    assert len(hostile) == 4 and int((dec2.statuses != 0).sum()) >= 2
    assert all(img.shape == (53, 37, 3) for img in cut(src2.cpu().numpy(), desc2))


def test_bad_descriptors_leave_the_buffer_untouched(J, CASES):
    names = ["ok_420_16x16", "ok_422_17x33", "ok_444_9x7", "ok_gray_37x53"]
    streams = [CASES[0][n][0] for n in names]
    body, desc, status, _ = pixels_direct(J, streams, shift=[0, 4, 0, 0])      # image 1 at an offset that is no multiple of 16
    assert status == 2
    imgs = cut(body, desc)
    assert np.all(imgs[1] == SENT)
    for k in (0, 2, 3):
        assert np.array_equal(imgs[k], CASES[0][names[k]][1])
    body, desc, status, _ = pixels_direct(J, streams, max_hw=(33, 17))         # images 0 (16 wide fits) .. 3 (53x37 does not)
    assert status == 4
    imgs = cut(body, desc)
    assert np.all(imgs[3] == SENT)
    for k in (0, 1, 2):
        assert np.array_equal(imgs[k], CASES[0][names[k]][1])
    _, good, _, _ = pixels_direct(J, streams)
    wrong = good.copy()
    wrong["h"][2] += 1                                                          # a size that is not the stream's
    wrong["offset"][3] += 48
    body, desc, status, _ = pixels_direct(J, streams, desc=wrong)
    assert status == 3 and np.all(cut(body, desc)[2] == SENT)
    neg = good.copy()
    neg["offset"][0] = -16
    body, _, status, _ = pixels_direct(J, streams, desc=neg)
    assert status == 1 and np.all(body[:3 * 16 * 16] == SENT)


def _members(CASES):
    names = ["ok_420_37x53", "ok_422_37x53", "ok_444_37x53", "ok_gray_37x53", "ok_qtables", "ok_checker_q5", "ok_noise_q50", "ok_420_17x33"]
    tg = lambda k: np.array([[k % 3, 0.5, 0.5, 0.4 + 0.05 * (k % 4), 0.5], [1, 0.3, 0.6, 0.2, 0.3]], np.float32)
    return [(CASES[0][n][0], CASES[0][n][1], tg(k)) for k, n in enumerate(names)]


def test_batch_prep_on_streams_equals_batch_prep_on_arrays(J, CASES):
    from mobilenet_yolo_pytorch_amd import prep
    mem = _members(CASES)
    sizes = [(64, 64), (96, 80)]
    r0, r1 = random.Random(3), random.Random(3)
    a = prep.BatchPrep(sizes, MEAN, STD, rng=r0)
    b = prep.BatchPrep(sizes, MEAN, STD, rng=r1, decoder=J.JpegDecoder(threads=2))
    for _ in range(2):
        xa, xb = a([m[1] for m in mem]), b([m[0] for m in mem])
        a.check(), b.check(), b.decoder.check()
        assert xa.shape == xb.shape and torch.equal(xa, xb)
    assert r0.getstate() == r1.getstate()
    assert torch.equal(b([m[1] for m in mem], size=(64, 64)), a([m[1] for m in mem], size=(64, 64)))   # arrays still take the old path
    with pytest.raises(ValueError, match="not both"):
        b([mem[0][0], mem[1][1]])


def test_train_augment_on_streams_equals_train_augment_on_arrays(J, CASES):
    from mobilenet_yolo_pytorch_amd import augment
    mem = _members(CASES)
    cfg = dict(train_img_size=[[96, 96], [64, 64]], normalize=dict(mean=MEAN, std=STD), expand_scale=2.0)
    shape = [[0, 1, 2, 3], [4], [5, 6], [7]]                                    # a four-image Mosaic, a two-image one, two singles
    arrays = [[(mem[k][1], mem[k][2]) for k in g] for g in shape]
    streams = [[(mem[k][0], mem[k][2]) for k in g] for g in shape]
    r0, r1 = random.Random(4), random.Random(4)
    a = augment.TrainAugment.from_config(cfg, rng=r0, canvas=200)
    b = augment.TrainAugment.from_config(cfg, rng=r1, canvas=200, decoder=J.JpegDecoder(threads=2))
    for _ in range(2):
        xa, ta, ca = a(arrays)
        xb, tb, cb = b(streams)
        a.check(), b.check(), b.decoder.check()
        assert xa.shape == xb.shape and torch.equal(xa, xb)
        assert ca == cb == 8 and len(ta) == len(tb) == 4 and all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert r0.getstate() == r1.getstate()
    seq = augment.SeqAugment.fixed([[(augment.SEQ_MEDIAN, 3)]] * 8)
    c = augment.TrainAugment.from_config(cfg, rng=random.Random(4), canvas=200, seq=seq)
    d = augment.TrainAugment.from_config(cfg, rng=random.Random(4), canvas=200, seq=seq, decoder=J.JpegDecoder())
    assert torch.equal(c(arrays)[0], d(streams)[0])
    with pytest.raises(ValueError, match="not both"):
        b([[(mem[0][0], mem[0][2])], [(mem[1][1], mem[1][2])]])


def test_two_runs_give_identical_buffers(J, CASES):
    names = ok_names(CASES)
    streams = [CASES[0][n][0] for n in names]
    a = pixels_direct(J, streams)[0]
    b = pixels_direct(J, streams)[0]
    assert np.array_equal(a, b)
    dec = J.JpegDecoder(threads=8)
    s1 = dec(streams)[0].clone()
    s2 = dec(streams)[0]
    d = dec(streams)[1]
    cover = np.zeros(s1.numel(), bool)
    for r in d:
        cover[int(r["offset"]):int(r["offset"]) + 3 * int(r["h"]) * int(r["w"])] = True
    assert np.array_equal(s1.cpu().numpy()[cover], s2.cpu().numpy()[cover])
