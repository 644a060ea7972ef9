"""numpy restatement of the sliced-inference stages of include/mnyolo.h (the tile grid, mny_prep_tiles, mny_det_append_tiles): the grid as
SAHI's two nested loops, the tile prep as the Pillow restatement of oracle/prep_ref.py applied to the window as an image of its own, the
append as the sequential loop of the specification with fp32 compares in np.float32 and the map in np.float64."""
import numpy as np

from oracle import prep_ref

f32, f64 = np.float32, np.float64

TILE_DESC = np.dtype([("offset", np.int64), ("h", np.int32), ("w", np.int32), ("pitch", np.int32), ("image", np.int32)])       # mny_tile_desc
TILE_MAP = np.dtype([("ax", f64), ("bx", f64), ("ay", f64), ("by", f64), ("ex", f32), ("ey", f32), ("image", np.int32),
                     ("interior", np.uint32)])                                                                                   # mny_tile_map
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8


def tile_grid(h, w, tile_h, tile_w, overlap_h, overlap_w):
    """the published loop of SAHI's get_slice_bboxes, statement by statement"""
    oy, ox = int(overlap_h * tile_h), int(overlap_w * tile_w)
    out = []
    y_max = y_min = 0
    while y_max < h:
        x_min = x_max = 0
        y_max = y_min + tile_h
        while x_max < w:
            x_max = x_min + tile_w
            if y_max > h or x_max > w:
                xmax, ymax = min(w, x_max), min(h, y_max)
                out.append((max(0, xmax - tile_w), max(0, ymax - tile_h), xmax, ymax))
            else:
                out.append((x_min, y_min, x_max, y_max))
            x_min = x_max - ox
        y_min = y_max - oy
    return out


def make_map(box, h, w, edge, size, image):
    """the mny_tile_map record of the window (x0, y0, x1, y1) of an h x w image"""
    x0, y0, x1, y1 = box
    m = np.zeros((), TILE_MAP)
    m["ax"], m["bx"] = f64(x0) / f64(w), f64(x1 - x0) / f64(w)
    m["ay"], m["by"] = f64(y0) / f64(h), f64(y1 - y0) / f64(h)
    m["ex"] = m["ey"] = f32(f64(edge) / f64(size))
    m["image"] = image
    m["interior"] = (LEFT * (x0 > 0)) | (TOP * (y0 > 0)) | (RIGHT * (x1 < w)) | (BOTTOM * (y1 < h))
    return m


def prep_window(img_hwc, box, out_h, out_w, mean, std):
    """[3,out_h,out_w] float32 of the window (x0, y0, x1, y1): a dense copy, resized as an image of its own, ToTensor, Normalize"""
    x0, y0, x1, y1 = box
    win = np.ascontiguousarray(img_hwc[y0:y1, x0:x1])
    return prep_ref.to_tensor_normalize(prep_ref.resize_bilinear_u8(win, out_h, out_w), mean, std)


def prep_tiles(src, tiles, max_h, max_w, out_h, out_w, mean, std):
    """src: flat uint8 buffer, tiles: TILE_DESC [B] -> (out [B,3,out_h,out_w] float32, status int)"""
    out = np.zeros((len(tiles), 3, out_h, out_w), f32)
    status = 0
    for b, t in enumerate(tiles):
        off, h, w, pitch = int(t["offset"]), int(t["h"]), int(t["w"]), int(t["pitch"])
        if int(t["image"]) == -1:
            continue
        if h < 1 or w < 1 or h > max_h or w > max_w or pitch < 3 * w:
            status = status or 1 + b
            continue
        win = np.stack([src[off + y * pitch:off + y * pitch + 3 * w].reshape(w, 3) for y in range(h)])
        out[b] = prep_ref.to_tensor_normalize(prep_ref.resize_bilinear_u8(win, out_h, out_w), mean, std)
    return out, status


def map_row(row, m):
    """one surviving row through the map: (float)(a + b * (double)v), two fp64 operations then one rounding"""
    r = np.array(row, dtype=f32)
    for c, (a, b) in ((0, ("ax", "bx")), (1, ("ay", "by")), (2, ("ax", "bx")), (3, ("ay", "by"))):
        with np.errstate(invalid="ignore", over="ignore"):
            r[c] = f32(f64(m[a]) + f64(m[b]) * f64(row[c]))
    return r


def cut(row, m):
    """the edge drop: strict fp32 compares, only on the interior sides"""
    i = int(m["interior"])
    ex, ey, one = f32(m["ex"]), f32(m["ey"]), f32(1.0)
    x1, y1, x2, y2 = (f32(v) for v in row[:4])
    with np.errstate(invalid="ignore"):
        return bool((i & LEFT and x1 < ex) or (i & RIGHT and x2 > one - ex) or (i & TOP and y1 < ey) or (i & BOTTOM and y2 > one - ey))


def det_append_tiles(src_rows, src_counts, maps, dst_rows, counts, dropped):
    """src_rows [B,src_stride,7], maps TILE_MAP [B], dst_rows [N,dst_stride,7] (written in place), counts / dropped [N] (updated in place)"""
    B, src_stride, _ = src_rows.shape
    N, dst_stride = dst_rows.shape[0], dst_rows.shape[1]
    for b in range(B):
        n = int(maps[b]["image"])
        if not 0 <= n < N:
            continue
        base = int(counts[n])
        room = dst_stride - base if 0 <= base <= dst_stride else 0
        t = 0
        for r in range(max(0, min(int(src_counts[b]), src_stride))):
            row = src_rows[b, r]
            if cut(row, maps[b]):
                continue
            if t < room:
                dst_rows[n, base + t] = map_row(row, maps[b])
            t += 1
        counts[n] = base + min(t, room)
        dropped[n] += t - min(t, room)
    return dst_rows, counts, dropped
