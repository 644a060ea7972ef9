"""numpy restatement of the device half of the JPEG decoder as include/mnyolo.h states it (mny_jpeg_pixels_batch): dequantise,
the 13-bit fixed-point inverse DCT (columns, then rows), chroma upsampling, YCbCr -> RGB.  It takes the coefficients and item
records the library's host stage wrote, so a comparison with Pillow's pixels pins the entropy stage and the specification
together without a GPU.  int64 throughout: for streams an encoder wrote nothing leaves int32."""
import numpy as np


def idct8(v, axis):
    v = np.moveaxis(v, axis, 0)
    v0, v1, v2, v3, v4, v5, v6, v7 = v
    z1 = (v2 + v6) * 4433
    t2 = z1 - v6 * 15137
    t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v7, v5, v3, v1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3])
    return np.moveaxis(out, 0, axis)


def plane(coef, item, c):
    """The uint8 plane of component c, padded to whole blocks."""
    bw, bh = int(item["bw"][c]), int(item["bh"][c])
    start = int(item["coef_off"]) + int(item["plane_off"][c])
    blk = coef[start:start + 64 * bw * bh].astype(np.int64).reshape(bh, bw, 8, 8) * item["q"][c].astype(np.int64).reshape(8, 8)
    blk = (idct8(blk, 2) + 1024) >> 11                                   # columns: along the row index
    blk = (idct8(blk, 3) + 131072) >> 18                                 # rows
    return np.clip(blk + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _left(p):
    return np.concatenate([p[:, :1], p[:, :-1]], 1)


def _right(p):
    return np.concatenate([p[:, 1:], p[:, -1:]], 1)


def upsample(p, hs, vs, force_filter=False):
    """p: the cropped chroma plane [ch, cw] (int64) -> [ch * vs, cw * hs]."""
    if hs == 1:
        return p
    if p.shape[1] <= 2 and not force_filter:                             # libjpeg replicates a plane this narrow
        return np.repeat(np.repeat(p, vs, 0), 2, 1)
    out = np.empty((p.shape[0] * vs, p.shape[1] * 2), np.int64)
    if vs == 1:
        out[:, 0::2] = (3 * p + _left(p) + 1) >> 2
        out[:, 1::2] = (3 * p + _right(p) + 2) >> 2
        return out
    s = np.empty((p.shape[0] * 2, p.shape[1]), np.int64)
    s[0::2] = 3 * p + np.concatenate([p[:1], p[:-1]], 0)
    s[1::2] = 3 * p + np.concatenate([p[1:], p[-1:]], 0)
    out[:, 0::2] = (3 * s + _left(s) + 8) >> 4
    out[:, 1::2] = (3 * s + _right(s) + 7) >> 4
    return out


def decode(coef, item, force_filter=False):
    """-> uint8 [h,w,3], what mny_jpeg_pixels_batch writes for this item."""
    assert int(item["status"]) == 0
    h, w, hs, vs = int(item["h"]), int(item["w"]), int(item["hs"]), int(item["vs"])
    y = plane(coef, item, 0)[:h, :w]
    if int(item["ncomp"]) == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cw, ch = (w + hs - 1) // hs, (h + vs - 1) // vs
    cb = upsample(plane(coef, item, 1)[:ch, :cw], hs, vs, force_filter)[:h, :w] - 128
    cr = upsample(plane(coef, item, 2)[:ch, :cw], hs, vs, force_filter)[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)
