"""Baseline JPEG decode in front of the device pipeline — the reference decodes with `cv2.imdecode` on the loader workers
(folder2lmdb.py:94) from the raw file bytes its LMDB stores (:266).  Here the decode is split where the work changes
character (include/mnyolo.h): marker parsing and Huffman decoding run in the library on the host, multi-threaded
over the images of a batch (`mny_jpeg_entropy_batch`), the quantised coefficients go up as int16 in one copy, as many bytes as
the RGB upload they replace at 4:2:0, and dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB run on the device
(`mny_jpeg_pixels_batch`, csrc/jpeg.hip) straight into the packed `src` + `mny_image_desc` layout that `mny_prep_batch`,
`mny_aug_batch` and `mny_aug_seq_batch` read.  Decoded pixels never exist in host memory.

The pixels equal Pillow's (libjpeg-turbo, default settings) bit for bit; tests pin that.  cv2.imdecode, the reference's own
call, uses the same libjpeg defaults but is not installed here, so it is unpinned.  Streams the decoder does not take
(progressive, CMYK, 12-bit, 4:4:0, multi-scan, damaged ones: a non-zero MNY_JPEG_* status per image) go through `fallback`,
by default Pillow, and land in the same buffer, so the caller sees one uniform result.  The decoder is opt-in:
`BatchPrep(..., decoder=JpegDecoder())`, `TrainAugment.from_config(cfg, decoder=JpegDecoder())`.  No CPU fallback for the
supported streams: without libmnyolo.so every call raises MnyError.

The way out is the mirror image (`JpegEncoder`, at the end of this file; the reference writes its result with `cv2.imwrite`,
inference.py:104): everything per pixel on the device into the same int16 coefficient layout (`mny_jpeg_coef_batch`,
csrc/jpegenc.hip), one copy down, headers and Huffman coding on host threads (`mny_jpeg_huffman_batch`).  The bytes equal the file
Pillow's `save(f, "JPEG", quality=, subsampling=)` writes; tests pin that too."""
import ctypes
import io

import numpy as np
import torch

from ._lib import MnyError, call, query
from .prep import DESC, is_encoded

INFO = np.dtype([("status", np.int32), ("h", np.int32), ("w", np.int32), ("ncomp", np.int32), ("hs", np.int32), ("vs", np.int32),
                 ("bw", np.int32, 3), ("bh", np.int32, 3), ("n_coef", np.int64)])                 # mny_jpeg_info
ITEM = np.dtype([("status", np.int32), ("h", np.int32), ("w", np.int32), ("ncomp", np.int32), ("hs", np.int32), ("vs", np.int32),
                 ("bw", np.int32, 3), ("bh", np.int32, 3), ("coef_off", np.int64), ("n_coef", np.int64), ("plane_off", np.int64, 3),
                 ("reserved0", np.int32, 2), ("q", np.uint16, (3, 64)), ("reserved", np.int32, 8)])   # mny_jpeg_item
assert INFO.itemsize == 56 and ITEM.itemsize == 512 and ITEM.fields["q"][1] == 96
STATUS = ("ok", "truncated", "not a JPEG", "progressive", "extended sequential", "arithmetic or lossless", "12-bit samples or 16-bit tables",
          "colour space (CMYK, YCCK, RGB)", "sampling (4:4:0 or other)", "multi-scan", "Huffman data", "marker", "header", "too large",
          "capacity")                                                                                # MNY_JPEG_*, by value
(OK, TRUNCATED, NOT_JPEG, PROGRESSIVE, EXTENDED, ARITHMETIC, PRECISION, COLORSPACE, SAMPLING, MULTISCAN, HUFFMAN, MARKER, HEADER, TOO_LARGE,
 CAPACITY) = range(15)
MAX_THREADS = 16


def as_stream(b):
    """bytes, bytearray, memoryview or a 1-D uint8 array / tensor -> a contiguous 1-D uint8 array over the same memory."""
    if isinstance(b, torch.Tensor):
        b = b.numpy()
    if isinstance(b, np.ndarray):
        if b.dtype != np.uint8 or b.ndim != 1:
            raise ValueError("an encoded image is bytes-like or a 1-D uint8 array, got %s %s" % (b.dtype, b.shape))
        return np.ascontiguousarray(b)
    if isinstance(b, (bytes, bytearray, memoryview)):
        return np.frombuffer(b, np.uint8)
    raise ValueError("an encoded image is bytes-like or a 1-D uint8 array, got %s" % type(b).__name__)


def probe(streams):
    """Host only: the INFO record of every stream (headers up to SOS)."""
    views = [as_stream(b) for b in streams]
    info = np.zeros(len(views), INFO)
    for i, v in enumerate(views):
        if v.size == 0:
            info[i]["status"] = TRUNCATED
            continue
        call("mny_jpeg_probe", ctypes.c_void_p(v.ctypes.data), v.size, ctypes.c_void_p(info[i:i + 1].ctypes.data))
    return info


def layout(info):
    """-> (coef_off per image in int16 elements, total): the images that probe well one after the other."""
    need = np.where(info["status"] == OK, info["n_coef"], 0).astype(np.int64)
    off = np.zeros(len(info), np.int64)
    off[1:] = np.cumsum(need)[:-1]
    return off, need, int(need.sum())


def entropy(streams, coef, coef_off, coef_cap, items, threads=8):
    """Host only: `mny_jpeg_entropy_batch` on numpy buffers (coef int16, items ITEM; both written in place)."""
    views = [as_stream(b) for b in streams]
    n = len(views)
    if coef.dtype != np.int16 or items.dtype != ITEM or len(items) != n or not coef.flags.c_contiguous or not items.flags.c_contiguous:
        raise ValueError("coef is a contiguous int16 array, items one ITEM record per stream")
    ptrs = (ctypes.c_void_p * n)(*[v.ctypes.data for v in views])
    lens = np.array([v.size for v in views], np.int64)
    off = np.ascontiguousarray(coef_off, np.int64)
    cap = np.ascontiguousarray(coef_cap, np.int64)
    if len(off) != n or len(cap) != n or (n and int((off + cap).max()) > coef.size) or (n and int(off.min()) < 0):
        raise ValueError("the coefficient slices do not fit the buffer")
    call("mny_jpeg_entropy_batch", ptrs, ctypes.c_void_p(lens.ctypes.data), n, ctypes.c_void_p(coef.ctypes.data), ctypes.c_void_p(off.ctypes.data),
         ctypes.c_void_p(cap.ctypes.data), ctypes.c_void_p(items.ctypes.data), int(threads))
    return items


def decode_host(streams, threads=8):
    """Host only: probe + entropy decode into fresh numpy buffers -> (coef int16, items ITEM).  For tests and tools."""
    info = probe(streams)
    off, need, total = layout(info)
    coef = np.zeros(max(total, 64), np.int16)
    items = np.zeros(len(info), ITEM)
    entropy(streams, coef, off, need, items, threads)
    return coef, items


def pillow_fallback(b):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(b))).convert("RGB"))


class JpegDecoder:
    """dec = JpegDecoder(device="cuda:0", threads=8, fallback=None)
       src, desc, max_h, max_w = dec(list_of_encoded_images)
    -> src: the decoded RGB uint8 images, HWC, packed in one buffer on `device` at offsets that are multiples of 16, as
    BatchPrep.pack lays them out; desc: their DESC array (host).  An image whose status is not 0 is decoded by
    `fallback(bytes) -> uint8 [h,w,3]` (default: Pillow, imported when first needed) and copied into the same buffer."""

    def __init__(self, device="cuda:0", threads=8, fallback=None):
        self.device = torch.device(device)
        self.threads = max(1, min(MAX_THREADS, int(threads)))
        self.fallback = fallback
        self._stage = None                          # pinned staging buffer (item records, then coefficients), grown on demand
        self._uploaded = None                       # event after the last copy out of _stage
        self._status = None
        self._fallback_idx = ()
        self.statuses = None                        # per-image MNY_JPEG_* of the last batch (host)

    def _decode_fallback(self, i, view, status):
        fb = self.fallback
        if fb is None:
            try:
                import PIL  # noqa: F401
            except ImportError:
                raise MnyError("image %d: status %d (%s) needs the fallback decoder and Pillow is not installed" % (i, status, STATUS[status]))
            fb = pillow_fallback
        a = np.asarray(fb(view.tobytes()))
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError("image %d: the fallback must return uint8 [h,w,3], got %s %s" % (i, a.dtype, a.shape))
        return np.ascontiguousarray(a)

    def sizes(self, streams):
        """Host only: (h, w) of every image from the probe; a stream without a readable frame header asks the fallback."""
        views = [as_stream(b) for b in streams]
        info = probe(views)
        out = []
        for i, (v, r) in enumerate(zip(views, info)):
            if r["h"] > 0 and r["w"] > 0:
                out.append((int(r["h"]), int(r["w"])))
            else:
                out.append(tuple(self._decode_fallback(i, v, int(r["status"])).shape[:2]))
        return out

    def host_stage(self, streams, threads=None):
        """Probe + entropy decode into the pinned staging buffer -> (items view, bytes used, coef_elems)."""
        views = [as_stream(b) for b in streams]
        n = len(views)
        if n == 0:
            raise ValueError("empty batch")
        info = probe(views)
        off, need, total = layout(info)
        coef_elems = max(total, 64)
        used = n * ITEM.itemsize + 2 * coef_elems
        if self._uploaded is not None:
            self._uploaded.synchronize()            # the last batch's copy has left the buffer
        if self._stage is None or self._stage.numel() < used:
            self._stage = torch.empty(max(used, 1 << 20), dtype=torch.uint8)
            if torch.cuda.is_available():
                self._stage = self._stage.pin_memory()
        buf = self._stage.numpy()
        items = buf[:n * ITEM.itemsize].view(ITEM)
        coef = buf[n * ITEM.itemsize:used].view(np.int16)
        entropy(views, coef, off, need, items, self.threads if threads is None else threads)
        return items, used, coef_elems

    def run_device(self, stage_dev, n, coef_elems, desc, max_h, max_w, nbytes):
        """stage_dev: the staging bytes on the device.  -> dst, `nbytes` of packed images."""
        dev = stage_dev.device
        size = query("mny_jpeg_ws_bytes", n, coef_elems)
        if size == 0:
            raise ValueError("mny_jpeg_ws_bytes refused n=%d coef_elems=%d" % (n, coef_elems))
        ws = torch.empty(size, device=dev, dtype=torch.uint8)
        dst = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
        d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        base = stage_dev.data_ptr()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_jpeg_pixels_batch", ctypes.c_void_p(base + n * ITEM.itemsize), ctypes.c_void_p(base), n, p(dst), p(d_dev), max_h, max_w, p(ws),
             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        self._status = ws[:4].view(torch.int32)
        self._keep = (stage_dev, d_dev, ws)
        return dst[:nbytes]

    def __call__(self, streams):
        views = [as_stream(b) for b in streams]
        items, used, coef_elems = self.host_stage(views)
        n = len(views)
        self.statuses = items["status"].copy()
        spare = {i: self._decode_fallback(i, views[i], int(items[i]["status"])) for i in np.flatnonzero(self.statuses != OK)}
        desc = np.zeros(n, DESC)
        off = 0
        for i in range(n):
            h, w = spare[i].shape[:2] if i in spare else (int(items[i]["h"]), int(items[i]["w"]))
            desc[i] = (off, h, w)
            off += (3 * h * w + 15) // 16 * 16
        max_h, max_w = int(desc["h"].max()), int(desc["w"].max())
        stage_dev = self._stage[:used].to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(torch.cuda.current_stream(self.device))
        dst = self.run_device(stage_dev, n, coef_elems, desc, max_h, max_w, off)
        for i, a in spare.items():                  # after the kernel, on the same stream
            o = int(desc[i]["offset"])
            dst[o:o + a.size].copy_(torch.from_numpy(a.reshape(-1)))
        self._fallback_idx = tuple(sorted(spare))
        return dst, desc, max_h, max_w

    def check(self):
        """Host sync: raise if the device refused an image that the host stage had accepted.  The status word holds only the LOWEST
        index the kernels left alone, so the comparison is with what the host expects there: the lowest image the fallback filled,
        or none.  A refused image BEHIND the first fallback image is therefore not seen; the records and descriptors are the
        decoder's own, so only a bug in this module could produce one."""
        if self._status is not None:
            v = int(self._status.item())
            want = self._fallback_idx[0] + 1 if self._fallback_idx else 0
            if v != want:
                raise RuntimeError("jpeg decode: the device reports image %d as the first one it left alone (misaligned or out-of-bounds "
                                   "descriptor, malformed item record), the host expected %s" % (v - 1, want - 1 if want else "none"))


# ---- encode: device coefficients, host entropy coding (include/mnyolo.h "baseline JPEG encode") ----------------------------
SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
HEADER_BYTES, BLOCK_BYTES = 700, 420                # what always fits: the headers, and one block at its worst with every FF stuffed


def enc_layout(desc, quality=75, subsampling="4:2:0"):
    """Host only: `mny_jpeg_enc_layout` -> (items ITEM, coef_elems) for the images of a DESC array."""
    hs, vs = SUBSAMPLING[subsampling]
    desc = np.ascontiguousarray(desc, DESC)
    items = np.zeros(len(desc), ITEM)
    total = ctypes.c_int64(0)
    call("mny_jpeg_enc_layout", ctypes.c_void_p(desc.ctypes.data), len(desc), int(quality), hs, vs, ctypes.c_void_p(items.ctypes.data),
         ctypes.byref(total))
    return items, int(total.value)


def huffman(coef, items, out, out_off, out_cap, threads=8):
    """Host only: `mny_jpeg_huffman_batch` on numpy buffers (coef int16, items ITEM, out uint8 written in place) -> (lengths, statuses)."""
    n = len(items)
    if coef.dtype != np.int16 or items.dtype != ITEM or out.dtype != np.uint8 or not (coef.flags.c_contiguous and items.flags.c_contiguous
                                                                                     and out.flags.c_contiguous):
        raise ValueError("coef is a contiguous int16 array, items ITEM records, out a contiguous uint8 array")
    off = np.ascontiguousarray(out_off, np.int64)
    cap = np.ascontiguousarray(out_cap, np.int64)
    if len(off) != n or len(cap) != n or (n and int((off + np.maximum(cap, 0)).max()) > out.size):
        raise ValueError("the output slices do not fit the buffer")
    lens = np.zeros(n, np.int64)
    status = np.zeros(n, np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    call("mny_jpeg_huffman_batch", p(coef), coef.size, p(items), n, p(out), p(off), p(cap), p(lens), p(status), int(threads))
    return lens, status


def worst_case(items):
    """Bytes that hold the stream of every record, whatever its coefficients."""
    return HEADER_BYTES + BLOCK_BYTES * (items["bw"].astype(np.int64) * items["bh"]).sum(axis=1)


def encode_host(coef, items, threads=8, caps=None):
    """Host only: entropy-code every image of (coef, items) -> (list of bytes, or None where the status is not 0; statuses).
    `caps`: bytes allowed per image (default: the worst case)."""
    caps = worst_case(items) if caps is None else np.ascontiguousarray(caps, np.int64)
    off = np.zeros(len(items), np.int64)
    off[1:] = np.cumsum(caps)[:-1]
    out = np.empty(max(int(caps.sum()), 1), np.uint8)
    lens, status = huffman(coef, items, out, off, caps, threads)
    return [out[o:o + l].tobytes() if s == OK else None for o, l, s in zip(off, lens, status)], status


class JpegEncoder:
    """enc = JpegEncoder(quality=75, subsampling="4:2:0", device="cuda:0", threads=8)
       files = enc(buf, desc)
    buf: packed uint8 RGB images, HWC, on `device` at offsets that are multiples of 16 (what JpegDecoder returns and viz writes);
    desc: their DESC array (host).  -> one `bytes` per image: the JPEG file, byte for byte what Pillow's
    `save(f, "JPEG", quality=, subsampling=)` writes for the same pixels.  One launch, one copy of the coefficients to the host,
    then the threaded host stage."""

    def __init__(self, quality=75, subsampling="4:2:0", device="cuda:0", threads=8):
        if subsampling not in SUBSAMPLING:
            raise ValueError("subsampling is one of %s, got %r" % (", ".join(SUBSAMPLING), subsampling))
        if not 1 <= int(quality) <= 100:
            raise ValueError("quality is 1..100, got %r" % (quality,))
        self.quality, self.subsampling = int(quality), subsampling
        self.device = torch.device(device)
        self.threads = max(1, min(MAX_THREADS, int(threads)))
        self.statuses = None                        # per-image MNY_JPEG_* of the last batch (host)

    def coefficients(self, buf, desc, fill=None):
        """The device stage alone -> (coef int16 on the device, items ITEM on the host, the status word on the device).
        `fill`: what the coefficient buffer holds before the launch (default: not initialised)."""
        desc = np.ascontiguousarray(desc, DESC)
        n = len(desc)
        if n == 0:
            raise ValueError("empty batch")
        if buf.dtype != torch.uint8 or buf.device != self.device or not buf.is_contiguous():
            raise ValueError("buf is a contiguous uint8 tensor on %s" % self.device)
        end = desc["offset"] + 3 * desc["h"].astype(np.int64) * desc["w"]
        if int(desc["offset"].min()) < 0 or int(end.max()) > buf.numel():
            raise ValueError("an image lies outside buf")
        items, total = enc_layout(desc, self.quality, self.subsampling)
        dev = self.device
        coef = torch.empty(max(total, 64), device=dev, dtype=torch.int16) if fill is None else \
            torch.full((max(total, 64),), fill, device=dev, dtype=torch.int16)
        ws = torch.empty(query("mny_jpeg_enc_ws_bytes", n), device=dev, dtype=torch.uint8)
        i_dev = torch.from_numpy(items.view(np.uint8).copy()).to(dev, non_blocking=True)
        d_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        call("mny_jpeg_coef_batch", p(buf), p(d_dev), p(i_dev), n, max(1, int(desc["h"].max())), max(1, int(desc["w"].max())), p(coef), p(ws),
             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        self._keep = (i_dev, d_dev)
        return coef, items, ws[:4].view(torch.int32)

    def __call__(self, buf, desc):
        coef, items, word = self.coefficients(buf, desc)
        host = torch.cat([coef.view(torch.uint8), word.view(torch.uint8)]).cpu().numpy()     # the one copy (and the sync)
        bad = int(host[-4:].view(np.int32)[0])
        if bad:
            raise ValueError("jpeg encode: image %d has a descriptor the device refused (offset not a multiple of 16, size outside "
                             "1..16383)" % (bad - 1))
        coef_h = host[:-4].view(np.int16)
        # the raw size is room enough for all but pathological content; the few images that need more get their worst case
        files, status = encode_host(coef_h, items, self.threads, np.minimum(worst_case(items), HEADER_BYTES + 3 * items["h"].astype(np.int64) * items["w"]))
        for i in np.flatnonzero(status == CAPACITY):
            one, st = encode_host(coef_h, items[i:i + 1], 1)
            files[i], status[i] = one[0], st[0]
        self.statuses = status.copy()
        if (status != OK).any():
            i = int(np.flatnonzero(status != OK)[0])
            raise MnyError("jpeg encode: image %d: status %d (%s)" % (i, status[i], STATUS[status[i]]))
        return files
