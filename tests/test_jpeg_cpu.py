"""CPU: the host half of the JPEG decoder (csrc/jpeg_host.h through mny_jpeg_probe / mny_jpeg_entropy_batch) on the committed
streams of tests/golden/jpeg_cases.npz (tools/gen_golden_jpeg.py), and the specification of the device half: tests/jpeg_ref.py
restates include/mnyolo.h in numpy, takes the library's coefficients and item records and must give Pillow's pixels."""
import hashlib
import io
import os

import numpy as np
import pytest

import jpeg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def jpeg():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    hashes = {n: str(z["h_" + n]) for n in names if "h_" + n in z.files}       # cases pinned by the SHA-256 of Pillow's RGB
    return {n: (z["s_" + n], z["p_" + n] if "p_" + n in z.files else None) for n in names}, str(z["voc_like_sha256"]), hashes


@pytest.fixture(scope="module")
def decoded(jpeg, cases):
    names = sorted(cases[0])
    coef, items = jpeg.decode_host([cases[0][n][0] for n in names], threads=4)
    return names, coef, items


def _ok(cases):
    return sorted(n for n in cases[0] if n.startswith("ok_"))


def _same(img, n, cases):
    """img equals Pillow's RGB of case n: by the stored pixels, or by their stored hash."""
    if n in cases[2]:
        return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == cases[2][n]
    return np.array_equal(img, cases[0][n][1])


def test_fixture_holds_what_the_issue_lists(cases):
    names = set(cases[0])
    for sub in ("420", "422", "444", "gray"):
        for size in ("1x1", "3x5", "4x9", "8x8", "9x7", "16x16", "17x33", "37x53"):
            assert "ok_%s_%s" % (sub, size) in names
    assert {"ok_optimize", "ok_rst_blocks", "ok_rst_rows", "ok_qtables", "ok_noise_q100", "ok_noise_q50", "ok_checker_q5", "route_progressive",
            "route_cmyk", "hostile_cut_headers", "hostile_cut_scan", "hostile_cut_eoi", "hostile_flip"} <= names
    s = cases[0]["ok_rst_blocks"][0].tobytes()
    assert b"\xff\xdd" in s and b"\xff\xd0" in s and b"\xff\xd1" in s          # DRI and restart markers are really there
    assert cases[0]["ok_optimize"][0].tobytes().count(b"\xff\xc4") >= 1
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("jpeg_cases.npz", "voc_like.jpg"))
    assert total < 150000 and os.path.getsize(os.path.join(GOLDEN, "voc_like.jpg")) < 40000


def test_probe_sizes_and_sampling(jpeg, cases):
    names = sorted(cases[0])
    info = jpeg.probe([cases[0][n][0] for n in names])
    for n, r in zip(names, info):
        px = cases[0][n][1]
        if px is not None:
            assert (int(r["h"]), int(r["w"])) == px.shape[:2], n             # also for the progressive and the CMYK stream
        if not n.startswith("ok_"):
            continue
        assert int(r["status"]) == jpeg.OK, n
        kind = n.split("_")[1]
        want = {"420": (3, 2, 2), "422": (3, 2, 1), "444": (3, 1, 1), "gray": (1, 1, 1)}.get(kind, (3, 2, 2))
        assert (int(r["ncomp"]), int(r["hs"]), int(r["vs"])) == want, n
        h, w, hs, vs = int(r["h"]), int(r["w"]), want[1], want[2]
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        bw = [mx * hs, mx, mx] if want[0] == 3 else [mx, 0, 0]
        bh = [my * vs, my, my] if want[0] == 3 else [my, 0, 0]
        assert list(r["bw"]) == bw and list(r["bh"]) == bh, n
        assert int(r["n_coef"]) == 64 * sum(a * b for a, b in zip(bw, bh)), n


def test_statuses(jpeg, decoded, cases):
    names, coef, items = decoded
    st = {n: int(it["status"]) for n, it in zip(names, items)}
    for n in _ok(cases):
        assert st[n] == jpeg.OK, n
    assert st["route_progressive"] == jpeg.PROGRESSIVE and st["route_cmyk"] == jpeg.COLORSPACE
    assert st["hostile_cut_headers"] == jpeg.TRUNCATED and st["hostile_cut_scan"] == jpeg.TRUNCATED
    assert len({jpeg.OK, jpeg.PROGRESSIVE, jpeg.COLORSPACE, jpeg.TRUNCATED}) == 4
    info = jpeg.probe([cases[0][n][0] for n in names])
    for n, r, it in zip(names, info, items):                                  # what the probe refuses, the decoder refuses alike
        if int(r["status"]) != jpeg.OK:
            assert int(it["status"]) == int(r["status"]), n


def _patched(stream, find, at, value):
    b = bytearray(stream.tobytes())
    i = b.index(find)
    b[i + at] = value
    return bytes(b)


def test_unsupported_streams_get_their_own_status(jpeg, cases):
    """Header variants made by patching one byte of a good stream: each leaves with a status of its own and no pixels."""
    base = cases[0]["ok_420_37x53"][0]
    sof = b"\xff\xc0"
    variants = {
        "extended": (_patched(base, sof, 1, 0xC1), jpeg.EXTENDED),
        "arithmetic": (_patched(base, sof, 1, 0xC9), jpeg.ARITHMETIC),
        "12-bit": (_patched(base, sof, 4, 12), jpeg.PRECISION),
        "16-bit table": (_patched(base, b"\xff\xdb", 4, 0x10), jpeg.PRECISION),
        "4:4:0": (_patched(base, sof, 11, 0x12), jpeg.SAMPLING),
        "two components in the scan": (_patched(base, b"\xff\xda", 4, 2), jpeg.HEADER),
        "not a jpeg": (b"\x89PNG\r\n\x1a\n" + bytes(32), jpeg.NOT_JPEG),
        "empty": (b"", jpeg.TRUNCATED),
    }
    streams = [v[0] for v in variants.values()]
    coef, items = jpeg.decode_host(streams, threads=2)
    for (name, (_, want)), it in zip(variants.items(), items):
        assert int(it["status"]) == want, (name, int(it["status"]))
    assert not coef.any()
    # a scan that holds one of the three components: the multi-scan status
    b = bytearray(base.tobytes())
    i = b.index(b"\xff\xda")
    one = bytes(b[:i]) + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + bytes(b[i + 14:])
    assert int(jpeg.probe([one])[0]["status"]) == jpeg.MULTISCAN


def test_reference_on_library_coefficients_equals_pillow(decoded, cases):
    names, coef, items = decoded
    checked = 0
    for n, it in zip(names, items):
        if n.startswith("ok_"):
            assert _same(jpeg_ref.decode(coef, it), n, cases), n
            checked += 1
    assert checked == 39 and set(cases[2]) == {"ok_rst_blocks", "ok_rst_rows", "ok_optimize", "ok_noise_q100"}


def test_voc_like_by_hash(jpeg, cases):
    s = open(os.path.join(GOLDEN, "voc_like.jpg"), "rb").read()
    coef, items = jpeg.decode_host([s], threads=1)
    assert (int(items[0]["h"]), int(items[0]["w"]), int(items[0]["hs"]), int(items[0]["vs"])) == (375, 500, 2, 2)
    assert hashlib.sha256(jpeg_ref.decode(coef, items[0]).tobytes()).hexdigest() == cases[1]


def test_narrow_chroma_planes_are_replicated_not_filtered(decoded, cases):
    """libjpeg replicates a subsampled plane that is at most 2 samples wide; the 3- and 4-pixel-wide fixtures must really depend on it."""
    names, coef, items = decoded
    for n in ("ok_420_3x5", "ok_420_4x9", "ok_422_3x5", "ok_422_4x9"):
        it = items[names.index(n)]
        assert (int(it["w"]) + 1) // 2 == 2
        forced = jpeg_ref.decode(coef, it, force_filter=True)
        assert not np.array_equal(forced, cases[0][n][1]), n
        assert np.array_equal(jpeg_ref.decode(coef, it), cases[0][n][1]), n


def test_threads_do_not_change_the_output(jpeg, cases):
    names = ["ok_rst_blocks", "ok_rst_rows", "ok_optimize", "ok_420_37x53", "hostile_flip", "ok_noise_q100", "route_cmyk"]
    streams = [cases[0][n][0] for n in names]
    c1, i1 = jpeg.decode_host(streams, threads=1)
    c4, i4 = jpeg.decode_host(streams, threads=4)
    assert np.array_equal(c1, c4) and i1.tobytes() == i4.tobytes()
    assert c1.any()
    c99, i99 = jpeg.decode_host(streams, threads=99)                           # clamped to 16
    assert np.array_equal(c1, c99) and i1.tobytes() == i99.tobytes()


def test_restart_streams_hold_the_plain_stream_s_coefficients(jpeg, cases):
    """Restart intervals change the byte stream, not the coefficients: same image, same tables."""
    ca, ia = jpeg.decode_host([cases[0]["ok_rst_blocks"][0]], threads=1)
    cb, ib = jpeg.decode_host([cases[0]["ok_rst_rows"][0]], threads=1)
    assert np.array_equal(ca, cb) and np.array_equal(ia["q"], ib["q"])


def test_slices_and_capacity(jpeg, cases):
    """A slice that is too small is refused and nothing is written; a decoded image stays inside its slice."""
    s = cases[0]["ok_420_37x53"][0]
    need = int(jpeg.probe([s])[0]["n_coef"])
    coef = np.full(3 * need, 0x5A5A, np.int16)
    items = np.zeros(2, jpeg.ITEM)
    jpeg.entropy([s, s], coef, np.array([need, 0]), np.array([need, need - 64]), items, threads=2)
    assert int(items[0]["status"]) == jpeg.OK and int(items[1]["status"]) == jpeg.CAPACITY
    assert (coef[:need] == 0x5A5A).all() and (coef[2 * need:] == 0x5A5A).all()
    assert int(items[0]["coef_off"]) == need and not (coef[need:2 * need] == 0x5A5A).all()
    with pytest.raises(ValueError):
        jpeg.entropy([s], coef, np.array([3 * need - 8]), np.array([need]), items[:1])


def test_hostile_streams_are_only_reported(jpeg, cases):
    base = cases[0]["ok_420_37x53"][0].tobytes()
    rng = np.random.default_rng(5)
    streams = [base[:k] for k in range(0, len(base), 7)]
    for _ in range(200):
        b = bytearray(base)
        b[int(rng.integers(len(b)))] ^= int(rng.integers(1, 256))
        streams.append(bytes(b))
    coef, items = jpeg.decode_host(streams, threads=4)
    st = items["status"]
    assert ((st >= 0) & (st < len(jpeg.STATUS))).all()
    assert (st[:len(base) // 7] != jpeg.OK).sum() >= len(base) // 7 - 1         # a prefix only decodes once every MCU is there


def test_live_comparison_with_pillow(jpeg):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    streams, want = [], []
    for k in range(20):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        low = rng.integers(0, 256, (h // 5 + 2, w // 5 + 2, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC)).copy()
        img = np.clip(img.astype(np.int32) + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
        gray = k % 5 == 4
        kw = dict(quality=int(rng.integers(20, 101)), optimize=bool(k % 2))
        if not gray:
            kw["subsampling"] = ["4:2:0", "4:2:2", "4:4:4"][k % 3]
        if k % 4 == 3:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        b = io.BytesIO()
        Image.fromarray(img[..., 0].copy() if gray else img).save(b, "JPEG", **kw)
        streams.append(b.getvalue())
        want.append(np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB")))
    coef, items = jpeg.decode_host(streams, threads=3)
    for k, (it, px) in enumerate(zip(items, want)):
        assert int(it["status"]) == jpeg.OK, k
        assert np.array_equal(jpeg_ref.decode(coef, it), px), (k, px.shape)


def test_missing_pillow_names_the_image_and_its_status(jpeg, cases, monkeypatch):
    """fallback=None where Pillow cannot be imported: MnyError with the image index and the status, not an ImportError."""
    import sys
    from mobilenet_yolo_pytorch_amd import MnyError
    dec = jpeg.JpegDecoder(device="cpu")
    view = jpeg.as_stream(cases[0]["route_progressive"][0])
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(MnyError, match=r"image 7: status %d \(progressive\).*Pillow is not installed" % jpeg.PROGRESSIVE):
        dec._decode_fallback(7, view, jpeg.PROGRESSIVE)
    with pytest.raises(ValueError, match=r"image 7: the fallback must return uint8 \[h,w,3\]"):
        jpeg.JpegDecoder(device="cpu", fallback=lambda b: np.zeros((4, 4), np.uint8))._decode_fallback(7, view, jpeg.PROGRESSIVE)


def test_python_surface_without_a_device(jpeg):
    from mobilenet_yolo_pytorch_amd import augment, prep
    assert prep.is_encoded(b"\xff\xd8") and prep.is_encoded(np.zeros(4, np.uint8)) and prep.is_encoded(memoryview(b"ab"))
    assert not prep.is_encoded(np.zeros((2, 2, 3), np.uint8)) and not prep.is_encoded(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="not both"):
        prep.all_encoded([b"\xff\xd8", np.zeros((2, 2, 3), np.uint8)])
    dec = jpeg.JpegDecoder(device="cpu", threads=99)
    assert dec.threads == 16
    assert augment.TrainAugment([(32, 32)], [0, 0, 0], [1, 1, 1], 2.0, decoder=dec).decoder is dec
    assert prep.BatchPrep([(32, 32)], [0, 0, 0], [1, 1, 1], decoder=dec).decoder is dec
    with pytest.raises(ValueError):
        jpeg.as_stream(np.zeros((2, 2), np.uint8))
