"""Baseline JPEG encode on the device (mny_jpeg_coef_batch behind jpeg.JpegEncoder) against the numpy restatement of
include/mnyolo.h (tests/jpegenc_ref.py, which tests/test_jpegenc_ref_cpu.py holds to the file Pillow writes) and, where Pillow
imports, against Pillow itself.  All of the arithmetic is integer work, so every comparison is exact.  Direct calls go through
ctypes with coef sized exactly inside a larger allocation of canary words."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpegenc_ref as R

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (3, 5), (6, 6), (8, 8), (9, 7), (16, 16), (17, 33), (24, 8), (37, 53), (40, 8)]    # h x w
GUARD = 2048                                                                     # int16 words in front of and behind coef
CANARY = 0x5A5A


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available()
    from mobilenet_yolo_pytorch_amd import jpeg
    return jpeg


def images(seed):
    return [R.pattern(h, w, "noise" if (k + seed) % 2 else "smooth", seed) for k, (h, w) in enumerate(SIZES)]


def pack(imgs, shift=None):
    """-> (device buffer, desc): the images at offsets that are multiples of 16 (+ shift[i])."""
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(len(imgs), DESC)
    off = 0
    for i, a in enumerate(imgs):
        desc[i] = (off + (shift[i] if shift else 0), a.shape[0], a.shape[1])
        off += (a.size + 15 + 16) // 16 * 16
    buf = np.full(off, 0xEE, np.uint8)
    for d, a in zip(desc, imgs):
        buf[int(d["offset"]):int(d["offset"]) + a.size] = a.reshape(-1)
    return torch.from_numpy(buf).cuda(), desc


def coef_direct(J, buf, desc, q, s, max_hw=None):
    """mny_jpeg_coef_batch on a canary-filled coefficient buffer -> (coef, items, status word); nothing outside coef is written."""
    from mobilenet_yolo_pytorch_amd._lib import call, query
    items, total = J.enc_layout(desc, q, s)
    dev = buf.device
    big = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.int16, device=dev)
    ws = torch.full((query("mny_jpeg_enc_ws_bytes", len(desc)),), 0xA5, dtype=torch.uint8, device=dev)
    i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    mh, mw = max_hw or (int(desc["h"].max()), int(desc["w"].max()))
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    call("mny_jpeg_coef_batch", p(buf), p(d_dev), p(i_dev), len(desc), mh, mw, p(big, 2 * GUARD), p(ws), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    out = big.cpu().numpy()
    assert (out[:GUARD] == CANARY).all() and (out[GUARD + total:] == CANARY).all(), "coef: words outside the buffer were written"
    return out[GUARD:GUARD + total], items, int(ws[:4].cpu().numpy().view(np.int32)[0])


@pytest.mark.parametrize("s", sorted(R.SAMPLING))
@pytest.mark.parametrize("q", [5, 75, 100])
def test_coefficients_equal_the_restatement_own_grid_blocks_only(J, q, s):
    """Every size at this sampling and quality in one batch.  The restatement leaves the canary in the blocks of the padded grid
    outside a component's own grid, and so must the kernel."""
    hs, vs = R.SAMPLING[s]
    imgs = images(q)
    buf, desc = pack(imgs)
    coef, items, status = coef_direct(J, buf, desc, q, s)
    assert status == 0
    untouched = 0
    for x, it in zip(imgs, items):
        want = R.coefficients(x, q, hs, vs, fill=CANARY)
        got = coef[int(it["coef_off"]):int(it["coef_off"]) + int(it["n_coef"])]
        assert np.array_equal(got, want), (x.shape, q, s)
        L = R.layout(x.shape[0], x.shape[1], hs, vs)
        untouched += sum(L["bw"][c] * L["bh"][c] - L["obw"][c] * L["obh"][c] for c in range(3))
    assert (untouched > 0) == (s != "4:4:4")                                    # padded grids really exceed the own grids


def test_a_wrong_descriptor_is_reported_and_left_alone(J):
    imgs = images(1)
    hs, vs = R.SAMPLING["4:2:0"]
    shift = [0] * len(imgs)
    shift[4] = 4                                                                # image 4 at an offset that is no multiple of 16
    buf, desc = pack(imgs, shift)
    coef, items, status = coef_direct(J, buf, desc, 75, "4:2:0")
    assert status == 5
    for k, (x, it) in enumerate(zip(imgs, items)):
        got = coef[int(it["coef_off"]):int(it["coef_off"]) + int(it["n_coef"])]
        if k == 4:
            assert (got == CANARY).all()
        else:
            assert np.array_equal(got, R.coefficients(x, 75, hs, vs, fill=CANARY)), k
    buf, desc = pack(imgs)
    coef, items, status = coef_direct(J, buf, desc, 75, "4:2:0", max_hw=(40, 33))    # only 37x53 (index 8) is wider
    assert status == 9
    got = coef[int(items[8]["coef_off"]):int(items[8]["coef_off"]) + int(items[8]["n_coef"])]
    assert (got == CANARY).all()
    last = coef[int(items[9]["coef_off"]):]
    assert np.array_equal(last, R.coefficients(imgs[9], 75, hs, vs, fill=CANARY))
    wrong = desc.copy()
    wrong["h"][0] = 0                                                           # the layout refuses it, so does the kernel
    c2, items2, status = coef_direct(J, buf, wrong, 75, "4:2:0")
    assert status == 1 and int(items2[0]["status"]) == J.HEADER
    enc = J.JpegEncoder(75, "4:2:0")
    with pytest.raises(ValueError, match="outside buf"):
        bad = desc.copy()
        bad["offset"][9] = buf.numel() - 16
        enc(buf, bad)


@pytest.mark.parametrize("s,q", [("4:2:0", 75), ("4:2:2", 5), ("4:4:4", 100)])
def test_encoder_output_equals_the_restatement_and_pillow(J, s, q):
    imgs = images(q + 1)
    buf, desc = pack(imgs)
    enc = J.JpegEncoder(quality=q, subsampling=s, threads=4)
    files = enc(buf, desc)
    assert len(files) == len(imgs) and all(isinstance(f, bytes) for f in files) and (enc.statuses == 0).all()
    for x, f in zip(imgs, files):
        assert f == R.encode(x, q, s), (x.shape, q, s)
    try:
        from PIL import Image
    except ImportError:
        return
    for x, f in zip(imgs, files):
        b = io.BytesIO()
        Image.fromarray(x).save(b, "JPEG", quality=q, subsampling=s)
        assert f == b.getvalue(), (x.shape, q, s)
    assert enc(buf, desc) == files                                              # and again: the same bytes


def test_a_voc_sized_batch_through_the_encoder(J):
    """375x500 at 4:2:0: 144 jobs per image, odd height, a width that is no multiple of 16; a small image behind the large ones."""
    imgs = [R.pattern(375, 500, "smooth", 2), R.pattern(375, 500, "noise", 3), R.pattern(16, 16, "noise", 4)]
    buf, desc = pack(imgs)
    files = J.JpegEncoder(threads=3)(buf, desc)
    for x, f in zip(imgs, files):
        assert f == R.encode(x, 75, "4:2:0"), x.shape


def test_round_trip_through_the_decoder(J):
    """JpegDecoder on the encoder's output equals Pillow's decode of Pillow's encode of the same pixels."""
    Image = pytest.importorskip("PIL.Image")
    imgs = images(9)
    buf, desc = pack(imgs)
    for s in sorted(R.SAMPLING):
        files = J.JpegEncoder(quality=90, subsampling=s)(buf, desc)
        dec = J.JpegDecoder(threads=2, fallback=lambda b: pytest.fail("the decoder takes every stream the encoder writes"))
        src, d2, mh, mw = dec(files)
        dec.check()
        got = src.cpu().numpy()
        for x, d in zip(imgs, d2):
            b = io.BytesIO()
            Image.fromarray(x).save(b, "JPEG", quality=90, subsampling=s)
            want = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
            h, w = int(d["h"]), int(d["w"])
            assert (h, w) == x.shape[:2]
            assert np.array_equal(got[int(d["offset"]):int(d["offset"]) + 3 * h * w].reshape(h, w, 3), want), (x.shape, s)
        src3 = J.JpegEncoder(quality=90, subsampling=s)(src, d2)                # the decoder's buffer feeds the encoder as it is
        assert len(src3) == len(files)
