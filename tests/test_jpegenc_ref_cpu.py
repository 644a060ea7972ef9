"""CPU: the specification of the JPEG encoder and its host half.  tests/jpegenc_ref.py restates include/mnyolo.h ("baseline JPEG
encode") in numpy, pixels -> coefficients -> bytes, and must give the FILE Pillow writes, byte for byte: live where Pillow
imports, and always against the streams stored in tests/golden/jpegenc_cases.npz (tools/gen_golden_jpegenc.py).  The library's
host stage (mny_jpeg_enc_layout, mny_jpeg_huffman_batch; csrc/jpegenc_host.h) is fed the restatement's coefficients and must
give the same bytes; the decoder's host stage on those bytes must return those coefficients.  No tolerance anywhere."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpegenc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 8), (6, 6), (7, 8), (8, 1), (8, 8), (8, 17), (9, 7), (16, 16), (17, 33), (24, 8), (37, 53), (40, 8),
         (64, 48), (8, 375), (375, 8)]                                           # h x w
QUALITIES = (5, 50, 75, 90, 95, 100)
CANARY = 0x5A5A


@pytest.fixture(scope="module")
def jpeg():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def stored():
    z = np.load(os.path.join(GOLDEN, "jpegenc_cases.npz"))
    out = {}
    for n in (str(n) for n in z["names"]):
        key, size, q, _ = n.split("_")
        out[n] = (z["x_" + n], z["s_" + n].tobytes(), int(q[1:]), key[0] + ":" + key[1] + ":" + key[2])
    return out


def pillow_file(x, q, s):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(x).save(b, "JPEG", quality=q, subsampling=s)
    return b.getvalue()


def library_files(jpeg, images, q, s, threads=3, fill=CANARY):
    """The library's host stage on the restatement's coefficients; blocks outside a component's own grid hold `fill`."""
    from mobilenet_yolo_pytorch_amd.prep import DESC
    hs, vs = R.SAMPLING[s]
    desc = np.zeros(len(images), DESC)
    for i, x in enumerate(images):
        desc[i] = (0, x.shape[0], x.shape[1])
    items, total = jpeg.enc_layout(desc, q, s)
    coef = np.full(max(total, 64), fill, np.int16)
    for x, it in zip(images, items):
        c = R.coefficients(x, q, hs, vs, fill=fill)
        assert len(c) == int(it["n_coef"])
        coef[int(it["coef_off"]):int(it["coef_off"]) + len(c)] = c
    files, status = jpeg.encode_host(coef, items, threads)
    assert (status == jpeg.OK).all()
    return files, coef, items


def test_fixture_holds_what_the_issue_lists(stored):
    assert len(stored) == 12
    shapes = {(n.split("_")[0], x.shape[:2]) for n, (x, _, _, _) in stored.items()}
    assert {("420", (6, 6)), ("420", (8, 8)), ("420", (24, 8)), ("420", (40, 8)), ("420", (37, 53))} <= shapes
    assert {n.split("_")[0] for n in stored} == {"420", "422", "444"}
    assert max(max(x.shape[:2]) for x, _, _, _ in stored.values()) == 53
    assert os.path.getsize(os.path.join(GOLDEN, "jpegenc_cases.npz")) < 40000


def test_restatement_equals_the_stored_pillow_files(stored):
    for n, (x, s, q, sub) in stored.items():
        assert R.encode(x, q, sub) == s, n


def test_restatement_equals_pillow_live_on_the_whole_grid():
    pytest.importorskip("PIL.Image")
    assert {(6, 6), (8, 8), (24, 8), (40, 8), (8, 375)} <= set(SIZES)
    checked = 0
    for h, w in SIZES:
        for kind in ("noise", "smooth"):
            x = R.pattern(h, w, kind)
            for q in QUALITIES:
                for s in R.SAMPLING:
                    assert R.encode(x, q, s) == pillow_file(x, q, s), (h, w, kind, q, s)
                    checked += 1
    assert checked == len(SIZES) * 2 * 6 * 3
    x = R.pattern(375, 500, "noise")
    assert R.encode(x, 75, "4:2:0") == pillow_file(x, 75, "4:2:0")


def test_even_heights_repeat_the_down_sampled_row_not_the_input_row():
    """At 4:2:0 the rows below the last down-sampled one repeat IT; repeating input rows first would give other coefficients at
    heights 2, 4, 6, 8, 24, 40 ... (the fixture must really depend on the difference)."""
    for h in (6, 24, 40):
        x = R.pattern(h, 8, "noise", seed=3)
        want = R.coefficients(x, 90, 2, 2)
        padded = np.concatenate([x, np.repeat(x[-1:], 16 - h % 16, axis=0)]) if h % 16 else x
        L, Lp = R.layout(h, 8, 2, 2), R.layout(padded.shape[0], 8, 2, 2)
        other = R.coefficients(padded, 90, 2, 2)
        a = want[L["plane_off"][1]:L["plane_off"][2]].reshape(L["bh"][1], L["bw"][1], 64)
        b = other[Lp["plane_off"][1]:Lp["plane_off"][2]].reshape(Lp["bh"][1], Lp["bw"][1], 64)
        assert not np.array_equal(a[:L["obh"][1]], b[:L["obh"][1]]), h


def test_quantisation_tables(jpeg):
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(1, DESC)
    desc[0] = (0, 9, 7)
    for q in (1, 5, 49, 50, 51, 75, 99, 100):
        items, _ = jpeg.enc_layout(desc, q, "4:2:0")
        ql, qc = R.qtables(q)
        assert np.array_equal(items[0]["q"][0], ql) and np.array_equal(items[0]["q"][1], qc) and np.array_equal(items[0]["q"][2], qc), q
    assert (R.qtables(100)[0] == 1).all() and R.qtables(1)[0].max() == 255 and R.qtables(50)[0][0] == 16


def test_layout_records(jpeg):
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(len(SIZES), DESC)
    for i, (h, w) in enumerate(SIZES):
        desc[i] = (16 * i, h, w)
    for s, (hs, vs) in R.SAMPLING.items():
        items, total = jpeg.enc_layout(desc, 75, s)
        off = 0
        for it, (h, w) in zip(items, SIZES):
            L = R.layout(h, w, hs, vs)
            assert (int(it["status"]), int(it["h"]), int(it["w"]), int(it["ncomp"]), int(it["hs"]), int(it["vs"])) == (0, h, w, 3, hs, vs)
            assert list(it["bw"]) == L["bw"] and list(it["bh"]) == L["bh"] and list(it["plane_off"]) == L["plane_off"]
            assert int(it["n_coef"]) == L["n_coef"] and int(it["coef_off"]) == off and off % 64 == 0
            off += L["n_coef"]
        assert total == off


def test_library_host_stage_equals_the_restatement_and_pillow(jpeg, stored):
    for q in (5, 75, 100):
        for s in R.SAMPLING:
            images = [R.pattern(h, w, "noise" if (h + w + q) % 2 else "smooth", seed=q) for h, w in SIZES]
            files, _, _ = library_files(jpeg, images, q, s)
            for x, f in zip(images, files):
                assert f == R.encode(x, q, s), (x.shape, q, s)
    names = sorted(stored)
    for sub in R.SAMPLING:
        for q in sorted({stored[n][2] for n in names}):
            group = [n for n in names if stored[n][3] == sub and stored[n][2] == q]
            if group:
                files, _, _ = library_files(jpeg, [stored[n][0] for n in group], q, sub)
                for n, f in zip(group, files):
                    assert f == stored[n][1], n                                 # Pillow's stored file


def test_decoder_host_stage_returns_the_coefficients(jpeg):
    """Round trip on the host: mny_jpeg_entropy_batch on the encoder's bytes gives the encoder's coefficients, a padding block
    being (the DC of the block before it in the MCU, no AC)."""
    for s, (hs, vs) in R.SAMPLING.items():
        images = [R.pattern(h, w, "noise", seed=7) for h, w in SIZES[:16]]
        files, coef, items = library_files(jpeg, images, 90, s, fill=0)
        back, items2 = jpeg.decode_host(files, threads=2)
        for x, it, it2 in zip(images, items, items2):
            assert int(it2["status"]) == jpeg.OK
            for k in ("h", "w", "hs", "vs", "n_coef"):
                assert int(it[k]) == int(it2[k])
            assert np.array_equal(it["q"], it2["q"])
            L = R.layout(x.shape[0], x.shape[1], hs, vs)
            a = coef[int(it["coef_off"]):][:L["n_coef"]]
            b = back[int(it2["coef_off"]):][:L["n_coef"]]
            for c in range(3):
                ga, gb = (v[L["plane_off"][c]:][:L["bw"][c] * L["bh"][c] * 64].reshape(L["bh"][c], L["bw"][c], 64) for v in (a, b))
                own = np.zeros((L["bh"][c], L["bw"][c]), bool)
                own[:L["obh"][c], :L["obw"][c]] = True
                assert np.array_equal(ga[own], gb[own]), (x.shape, s, c)
                assert not gb[~own][:, 1:].any()                               # padding blocks carry no AC


def test_threads_do_not_change_the_output(jpeg):
    images = [R.pattern(h, w, "noise", seed=1) for h, w in SIZES[:12]]
    one = library_files(jpeg, images, 75, "4:2:0", threads=1)[0]
    assert one == library_files(jpeg, images, 75, "4:2:0", threads=4)[0] == library_files(jpeg, images, 75, "4:2:0", threads=99)[0]


def test_a_slice_that_is_too_small_is_reported_and_respected(jpeg):
    x = R.pattern(17, 33, "noise")
    want = R.encode(x, 75, "4:2:0")
    _, coef, items = library_files(jpeg, [x], 75, "4:2:0")
    three = np.concatenate([items, items, items])
    for short in (len(want) - 1, 700, 100, 1, 0):
        out = np.full(3 * len(want) + 64, 0xC3, np.uint8)
        off = np.array([0, len(want), len(want) + short])
        lens, status = jpeg.huffman(coef, three, out, off, np.array([len(want), short, len(want)]), threads=3)
        assert list(status) == [jpeg.OK, jpeg.CAPACITY, jpeg.OK] and list(lens) == [len(want), 0, len(want)]
        assert out[:len(want)].tobytes() == want and out[off[2]:off[2] + len(want)].tobytes() == want
        assert (out[off[2] + len(want):] == 0xC3).all()                         # the canary behind the last slice
    out = np.full(len(want) + 64, 0xC3, np.uint8)
    lens, status = jpeg.huffman(coef, items, out, np.array([0]), np.array([len(want) - 1]), threads=1)
    assert status[0] == jpeg.CAPACITY and lens[0] == 0 and (out[len(want) - 1:] == 0xC3).all()
    with pytest.raises(ValueError, match="do not fit"):
        jpeg.huffman(coef, items, out, np.array([64]), np.array([len(want) + 1]))


def test_records_that_are_not_sound_get_their_status(jpeg):
    x = R.pattern(9, 7, "noise")
    _, coef, items = library_files(jpeg, [x], 75, "4:2:0")

    def status_of(change, c=coef):
        it = items.copy()
        change(it[0])
        out = np.zeros(4096, np.uint8)
        lens, status = jpeg.huffman(c, it, out, np.array([0]), np.array([4096]), threads=1)
        assert (lens[0] == 0) == (status[0] != jpeg.OK)
        return int(status[0])

    def setter(field, value, index=None):
        def f(it):
            if index is None:
                it[field] = value
            else:
                it[field][index] = value
        return f

    assert status_of(lambda it: None) == jpeg.OK
    assert status_of(setter("status", jpeg.TRUNCATED)) == jpeg.TRUNCATED
    assert status_of(setter("ncomp", 1)) == jpeg.COLORSPACE
    assert status_of(setter("vs", 3)) == jpeg.SAMPLING
    assert status_of(setter("hs", 1)) == jpeg.SAMPLING                       # 1x2 is the 4:4:0 the decoder refuses too
    assert status_of(setter("h", 0)) == jpeg.HEADER
    assert status_of(setter("w", 16384)) == jpeg.TOO_LARGE
    assert status_of(setter("bw", 3, 0)) == jpeg.HEADER
    assert status_of(setter("plane_off", 64, 1)) == jpeg.HEADER
    assert status_of(setter("n_coef", 64)) == jpeg.HEADER
    assert status_of(setter("coef_off", -64)) == jpeg.CAPACITY
    assert status_of(setter("coef_off", coef.size)) == jpeg.CAPACITY           # the slice would end outside coef
    assert status_of(setter("q", 0, (0, 5))) == jpeg.PRECISION
    assert status_of(setter("q", 256, (1, 63))) == jpeg.PRECISION
    assert status_of(setter("q", 7, (2, 3))) == jpeg.HEADER                    # one chrominance table in the stream
    cr = R.layout(9, 7, 2, 2)["plane_off"][2]                                   # the one Cr block: the last block of the one MCU
    big = coef.copy()
    big[cr + 9] = 1024                                                          # an AC coefficient of 11 bits
    assert status_of(lambda it: None, big) == jpeg.HUFFMAN
    big = coef.copy()
    big[cr] = 2048                                                              # a DC difference of 12 bits
    assert status_of(lambda it: None, big) == jpeg.HUFFMAN
    big = coef.copy()
    big[cr + 9], big[cr] = -1023, -2047                                         # the largest baseline takes
    assert status_of(lambda it: None, big) == jpeg.OK


def test_argument_errors(jpeg):
    from mobilenet_yolo_pytorch_amd import MnyError
    from mobilenet_yolo_pytorch_amd._lib import call, load
    from mobilenet_yolo_pytorch_amd.prep import DESC
    desc = np.zeros(2, DESC)
    desc[0], desc[1] = (0, 0, 5), (0, 5, 16384)
    items, total = jpeg.enc_layout(desc, 75, "4:4:4")
    assert list(items["status"]) == [jpeg.HEADER, jpeg.TOO_LARGE] and total == 0 and not items["n_coef"].any()
    desc[0], desc[1] = (0, 8, 8), (0, 8, 8)
    items = np.zeros(2, jpeg.ITEM)
    total = ctypes.c_int64(0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    good = lambda: [p(desc), 2, 75, 2, 2, p(items), ctypes.byref(total)]
    call("mny_jpeg_enc_layout", *good())
    for k, v, what in ((0, None, "null pointer"), (5, None, "null pointer"), (6, None, "null pointer"), (1, 0, "batch size"), (1, 4097, "batch size"),
                       (2, 0, "quality"), (2, 101, "quality"), (3, 3, "sampling"), (3, 4, "sampling"), (4, 0, "sampling"), (4, 3, "sampling")):
        a = good()
        a[k] = v
        with pytest.raises(MnyError, match=what):
            call("mny_jpeg_enc_layout", *a)
    a = good()
    a[3], a[4] = 1, 2                                                           # 1x2
    with pytest.raises(MnyError, match="sampling"):
        call("mny_jpeg_enc_layout", *a)
    with pytest.raises(KeyError):
        jpeg.enc_layout(desc, 75, "4:4:0")
    coef, out = np.zeros(1024, np.int16), np.zeros(4096, np.uint8)
    off, cap, lens, status = np.zeros(2, np.int64), np.full(2, 2048, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int32)
    good = lambda: [p(coef), coef.size, p(items), 2, p(out), p(off), p(cap), p(lens), p(status), 2]
    for k in (0, 2, 4, 5, 6, 7, 8):
        a = good()
        a[k] = None
        with pytest.raises(MnyError, match="null pointer"):
            call("mny_jpeg_huffman_batch", *a)
    for k, v in ((3, 0), (3, 4097), (1, -1)):
        a = good()
        a[k] = v
        with pytest.raises(MnyError, match="batch size"):
            call("mny_jpeg_huffman_batch", *a)
    out[:] = 0xC3
    off[1], cap[1] = -1, 10                                                     # a negative slice: that image only
    call("mny_jpeg_huffman_batch", *good())
    assert list(status) == [jpeg.OK, jpeg.CAPACITY] and lens[0] > 600 and lens[1] == 0 and (out[2048:] == 0xC3).all()
    # the device stage refuses bad arguments before it launches anything
    assert load().mny_jpeg_enc_ws_bytes(0) == 0 and load().mny_jpeg_enc_ws_bytes(4097) == 0 and load().mny_jpeg_enc_ws_bytes(3) >= 4
    with pytest.raises(MnyError, match="null pointer"):
        call("mny_jpeg_coef_batch", None, None, None, 1, 8, 8, None, None, None)
    with pytest.raises(MnyError, match="16-byte aligned"):
        call("mny_jpeg_coef_batch", 4096 + 4, 4096, 4096, 1, 8, 8, 4096, 4096, None)
    with pytest.raises(MnyError, match="bad sizes"):
        call("mny_jpeg_coef_batch", 4096, 4096, 4096, 0, 8, 8, 4096, 4096, None)
    with pytest.raises(MnyError, match="bad sizes"):
        call("mny_jpeg_coef_batch", 4096, 4096, 4096, 1, 8, 16384, 4096, 4096, None)
    with pytest.raises(ValueError):
        jpeg.JpegEncoder(quality=0, device="cpu")
    with pytest.raises(ValueError):
        jpeg.JpegEncoder(subsampling="4:4:0", device="cpu")
    assert jpeg.JpegEncoder(device="cpu", threads=99).threads == 16
