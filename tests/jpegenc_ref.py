"""The baseline JPEG encoder of include/mnyolo.h ("baseline JPEG encode") restated in numpy: pixels -> quantised coefficients
(`coefficients`, what mny_jpeg_coef_batch computes on the device) -> bytes (`huffman`, what mny_jpeg_huffman_batch writes on the
host).  All of it is integer arithmetic with arithmetic shifts; the bytes are the file Pillow (libjpeg-turbo) writes for
`Image.save(buf, "JPEG", quality=q, subsampling=s)`, which tests/test_jpegenc_ref_cpu.py holds it to."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# ITU-T T.81 Annex K.1: the example quantisation tables, natural order
Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                  100, 103, 99])
Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                 + [99] * 32)
# Annex K.3: the typical Huffman tables (bits[l-1] = codes of length l, then the symbols)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    list(bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
        "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
        "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def qtables(quality):
    """-> (luminance, chrominance) for quality 1..100, natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * s + 50) // 100, 1, 255).astype(np.uint16) for b in (Q_LUM, Q_CHR))


def layout(h, w, hs, vs):
    """-> dict: the padded block grids bw / bh (whole MCUs), the components' own grids obw / obh, plane_off, n_coef."""
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    bw, bh = [mx * hs, mx, mx], [my * vs, my, my]
    cw, ch = -(-w // hs), -(-h // vs)
    obw, obh = [-(-w // 8), -(-cw // 8), -(-cw // 8)], [-(-h // 8), -(-ch // 8), -(-ch // 8)]
    off = [0, bw[0] * bh[0] * 64, (bw[0] * bh[0] + bw[1] * bh[1]) * 64]
    return dict(bw=bw, bh=bh, obw=obw, obh=obh, plane_off=off, n_coef=off[2] + bw[2] * bh[2] * 64)


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def planes(rgb, hs, vs):
    """The three component planes, each over its OWN block grid (8 * obh x 8 * obw samples), edges filled as the header says."""
    h, w = rgb.shape[:2]
    L = layout(h, w, hs, vs)
    out = []
    for c, p in enumerate(ycc(rgb)):
        H, W = 8 * L["obh"][c], 8 * L["obw"][c]
        if c == 0 or (hs == 1 and vs == 1):
            out.append(p[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)])
            continue
        x = np.arange(W)
        xa, xb = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
        if vs == 1:
            rows = p[np.minimum(np.arange(H), h - 1)]
            out.append((rows[:, xa] + rows[:, xb] + (x & 1)) >> 1)
            continue
        y = np.minimum(np.arange(H), (h + 1) // 2 - 1)               # the last DOWN-SAMPLED row is what repeats
        ra, rb = p[np.minimum(2 * y, h - 1)], p[np.minimum(2 * y + 1, h - 1)]
        out.append((ra[:, xa] + ra[:, xb] + rb[:, xa] + rb[:, xb] + 1 + (x & 1)) >> 2)
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct1(d, first):
    """libjpeg's accurate integer forward DCT along the last axis; `first`: the row pass (else the column pass)."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    n = 11 if first else 15
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(plane, q):
    """plane [8*bh, 8*bw] samples -> [bh, bw, 64] quantised coefficients, natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    v = _fdct1(blk, True)                                            # rows
    v = _fdct1(v.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)     # columns
    d = 8 * q.astype(np.int64).reshape(8, 8)
    return (np.sign(v) * ((np.abs(v) + (d >> 1)) // d)).reshape(bh, bw, 64)


def coefficients(rgb, quality, hs, vs, fill=0):
    """-> int16 [n_coef] in the layout mny_jpeg_pixels_batch reads; the padded grids' blocks outside a component's own grid
    are not computed and keep `fill`."""
    h, w = rgb.shape[:2]
    L = layout(h, w, hs, vs)
    ql, qc = qtables(quality)
    out = np.full(L["n_coef"], fill, np.int16)
    for c, p in enumerate(planes(rgb, hs, vs)):
        grid = out[L["plane_off"][c]:L["plane_off"][c] + L["bw"][c] * L["bh"][c] * 64].reshape(L["bh"][c], L["bw"][c], 64)
        grid[:L["obh"][c], :L["obw"][c]] = fdct_quant(p, ql if c == 0 else qc)
    return out


def _codes(bits, vals):
    """-> {symbol: (code, length)}, the canonical assignment of the standard."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def header(h, w, hs, vs, ql, qc):
    """SOI .. SOS as Pillow writes them for a plain save: JFIF 1.01 without density, two DQT, SOF0, four DHT, SOS."""
    seg = lambda m, body: bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    s = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    s += seg(0xDB, [0] + [int(ql[k]) for k in ZIGZAG]) + seg(0xDB, [1] + [int(qc[k]) for k in ZIGZAG])
    s += seg(0xC0, [8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in (0, 1):
        s += seg(0xC4, [t] + DC_BITS[t] + DC_VALS[t]) + seg(0xC4, [0x10 | t] + AC_BITS[t] + AC_VALS[t])
    return s + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


class CoefficientRange(ValueError):
    pass


def huffman(coef, h, w, hs, vs, ql, qc):
    """The whole stream from the coefficients.  A padding block of an MCU is coded as all-zero AC with the DC of the block coded
    just before it in that MCU; its coefficients in `coef` are not read."""
    L = layout(h, w, hs, vs)
    dc = [_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
    ac = [_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    acc, nacc, body = 0, 0, bytearray()

    def put(code, n):
        nonlocal acc, nacc
        acc = (acc << n) | code
        nacc += n
        while nacc >= 8:
            b = (acc >> (nacc - 8)) & 255
            body.append(b)
            if b == 255:
                body.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1

    grids = [coef[L["plane_off"][c]:L["plane_off"][c] + L["bw"][c] * L["bh"][c] * 64].reshape(L["bh"][c], L["bw"][c], 64).astype(np.int64)
             for c in range(3)]
    pred = [0, 0, 0]
    for my in range(L["bh"][1]):
        for mx in range(L["bw"][1]):
            for c in range(3):
                t = 0 if c == 0 else 1
                nh, nv = (hs, vs) if c == 0 else (1, 1)
                last = None
                for v in range(nv):
                    for u in range(nh):
                        by, bx = my * nv + v, mx * nh + u
                        if by < L["obh"][c] and bx < L["obw"][c]:
                            blk = grids[c][by, bx][ZIGZAG]
                        else:
                            blk = np.zeros(64, np.int64)
                            blk[0] = last
                        last = int(blk[0])
                        diff = last - pred[c]
                        pred[c] = last
                        n = abs(diff).bit_length()
                        if n > 11:
                            raise CoefficientRange("DC difference %d" % diff)
                        put(*dc[t][n])
                        if n:
                            put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
                        run = 0
                        for k in range(1, 64):
                            a = int(blk[k])
                            if a == 0:
                                run += 1
                                continue
                            while run > 15:
                                put(*ac[t][0xF0])
                                run -= 16
                            n = abs(a).bit_length()
                            if n > 10:
                                raise CoefficientRange("AC coefficient %d" % a)
                            put(*ac[t][(run << 4) | n])
                            put((a if a >= 0 else a - 1) & ((1 << n) - 1), n)
                            run = 0
                        if run:
                            put(*ac[t][0])
    if nacc:
        put((1 << (8 - nacc)) - 1, 8 - nacc)
    return header(h, w, hs, vs, ql, qc) + bytes(body) + b"\xff\xd9"


def encode(rgb, quality=75, subsampling="4:2:0"):
    hs, vs = SAMPLING[subsampling]
    ql, qc = qtables(quality)
    return huffman(coefficients(rgb, quality, hs, vs), rgb.shape[0], rgb.shape[1], hs, vs, ql, qc)


def pattern(h, w, kind, seed=0):
    """Test content: `noise` (every coefficient busy) or `smooth` (gradients with strong chroma, long zero runs)."""
    if kind == "noise":
        return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 3 + xx * 2 + seed) % 256, (xx * 5 + 20) % 256, (yy * 4 + xx) % 256], -1).astype(np.uint8)
