"""Restatement of the blur / sharpen / noise stage (include/mnyolo.h, mny_aug_seq_batch) in numpy and scipy, fp64.
imgaug and cv2 are not available to pin the stage: the arithmetic in the header is the specification, and this file states
it a second time with other tools.  Every op returns (rounded uint8 image, the fp64 value before rounding), so that a
test can tell a genuine difference from an fp32 result that fell on the other side of a tie."""
import numpy as np
from scipy import ndimage

GAUSS, MEDIAN, SHARPEN, NOISE = range(4)
BAND = 1e-3            # the device's fp32 chains are within 1e-4 of the fp64 value; only a value this close to a tie may round the other way


def taps(sigma):
    d = np.arange(-2, 3, dtype=np.float64)
    t = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).astype(np.float32)


def _round(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def gaussian(img, t):
    """t: the five fp32 taps.  Rows first (unrounded), then columns; mirror = REFLECT_101."""
    t = np.asarray(t, np.float32).astype(np.float64)
    v = ndimage.correlate1d(img.astype(np.float64), t, axis=1, mode="mirror")
    v = ndimage.correlate1d(v, t, axis=0, mode="mirror")
    return _round(v), v


def median(img, k):
    out = ndimage.median_filter(img, size=(k, k, 1), mode="nearest")
    return out, out.astype(np.float64)


def sharpen_coeffs(alpha, lightness):
    a, l = float(alpha), float(lightness)
    return np.float32((1.0 - a) + a * (8.0 + l)), np.float32(-a)


def sharpen(img, c, s):
    """c, s: the fp32 centre and neighbour coefficients."""
    k = np.full((3, 3, 1), np.float64(np.float32(s)))
    k[1, 1, 0] = np.float64(np.float32(c))
    v = ndimage.correlate(img.astype(np.float64), k, mode="mirror")
    return _round(v), v


def philox4x32_10(counter0, key):
    """counter (c, 0, 0, 0) for every c of the uint32 array counter0, key = (k0, k1) -> four uint32 arrays."""
    M0, M1, W0, W1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xffffffff)
    c = [np.asarray(counter0, np.uint64) & mask] + [np.zeros(np.shape(counter0), np.uint64) for _ in range(3)]
    k0, k1 = int(key[0]), int(key[1])
    for i in range(10):
        if i:
            k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
    return [x.astype(np.uint32) for x in c]


def normals(counter0, key):
    """-> z [3, ...] fp64: Box-Muller on u_i = ((r_i >> 8) + 0.5) * 2^-24."""
    r = philox4x32_10(counter0, key)
    u = [((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for x in r]
    R0, R2 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([R0 * np.cos(2 * np.pi * u[1]), R0 * np.sin(2 * np.pi * u[1]), R2 * np.cos(2 * np.pi * u[3])])


def noise(img, scale, per_channel, key):
    h, w = img.shape[:2]
    z = normals(np.arange(h * w, dtype=np.uint64).reshape(h, w), key)
    z = np.moveaxis(z, 0, 2) if per_channel else np.repeat(z[0][:, :, None], 3, axis=2)
    d = np.float64(np.float32(scale)) * z
    return np.clip(img.astype(np.int64) + np.rint(d).astype(np.int64), 0, 255).astype(np.uint8), img.astype(np.float64) + d


def apply_op(img, rec, op):
    if op == GAUSS:
        return gaussian(img, rec["taps"])
    if op == MEDIAN:
        return median(img, int(rec["median_k"]))
    if op == SHARPEN:
        return sharpen(img, rec["sharpen_c"], rec["sharpen_s"])
    if op == NOISE:
        return noise(img, rec["noise_scale"], bool(rec["noise_per_channel"]), rec["noise_key"])
    raise ValueError(op)


def apply(img, rec):
    """One SEQ record on one image, uint8 between the ops -> (rounded, fp64 value of the last op, its input).  The comparison rule
    of the LAST op decides; an earlier inexact op is compared on its own by applying it alone."""
    out, v = img, img.astype(np.float64)
    for k in range(int(rec["n_ops"])):
        out, v = apply_op(out, rec, int(rec["op"][k]))
    return out, v


def in_band(v):
    """True where the fp64 value lies within BAND of a half-integer: the only places where fp32 may round the other way."""
    return np.abs((v - np.floor(v)) - 0.5) < BAND


def mismatch(dev, ref, v):
    """-> (number of pixels that break the rule, number of pixels inside the band).  Outside the band the device byte equals the
    rounded, clamped fp64 value; inside it may differ by one."""
    band = in_band(v)
    diff = np.abs(dev.astype(np.int64) - ref.astype(np.int64))
    return int(np.count_nonzero((~band & (diff != 0)) | (band & (diff > 1)))), int(np.count_nonzero(band))


# ---- the inputs the device tests use: the smallest shapes at which the kernels can go wrong (halo wider than the image, one ragged
# tile, several tiles both ways) x the contents that reach the clamps and the borders
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 5), (17, 33), (64, 67), (130, 257)]
CONTENTS = ("random", "zeros", "full", "checker")
GAUSS_SIGMAS = (0.5, 1.0)
SHARPEN_PARAMS = ((0.1, 0.9), (0.1, 1.1), (0.037, 1.0))
NOISE_SCALES = (0.3, 3.0, 7.65)
BAND_CAP = 0.02            # of the compared pixels of the images of 100 pixels and more, per test
SMALL_BAND_MAX = 1         # in-band pixels allowed in an image under 100 pixels


def images(seed=0):
    """-> [(shape, content, uint8 [h,w,3])], fixed by the seed."""
    r = np.random.RandomState(seed)
    out = []
    for h, w in SHAPES:
        for c in CONTENTS:
            if c == "random":
                a = r.randint(0, 256, size=(h, w, 3))
            elif c == "checker":
                a = np.repeat((((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255)[:, :, None], 3, axis=2)
            else:
                a = np.full((h, w, 3), 0 if c == "zeros" else 255)
            out.append(((h, w), c, a.astype(np.uint8)))
    return out


def band_ok(vs):
    """The precondition of a rounded comparison, on the restatement's values alone: vs = the fp64 images of one test."""
    big = [v for v in vs if v.shape[0] * v.shape[1] >= 100]
    small = [v for v in vs if v.shape[0] * v.shape[1] < 100]
    count = lambda v: int(np.count_nonzero(in_band(v).any(axis=2)))              # a pixel is in the band when one of its channels is
    n_band, n_all = sum(count(v) for v in big), sum(v.shape[0] * v.shape[1] for v in big)
    return (n_all == 0 or n_band <= BAND_CAP * n_all) and all(count(v) <= SMALL_BAND_MAX for v in small)


def noise_key(i):
    """The key of image i in the device tests (with these keys and images(0) every rounded case meets band_ok; tests/test_seq_cpu.py
    checks that before the GPU is asked)."""
    return (1000 + i, 78)
