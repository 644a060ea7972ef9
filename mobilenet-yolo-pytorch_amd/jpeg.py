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
supported streams: without libmnyolo.so every call raises MnyError."""
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
