#!/usr/bin/env python3
"""Times sliced inference (slicing.Sliced) on 64 frames of 1280x720, tile 416, overlap 0.2, full view (9 records per frame, 576 records,
nine chunks of 64 slots), on procedural weights: `mny_prep_tiles` (one chunk), the chunk's forward + decode (`plan.forward_eval`,
nms=False), `mny_det_append_tiles` (one chunk into a zeroed joint buffer), the joint NMS, the host pack + upload of the frames, and the
whole call.  Beside it the sum of the plain `plan.forward_eval` calls at the same chunk sizes (the overhead of the new stages is the
whole call over that sum) and the host-side alternative: Pillow `crop` on a 16-thread pool, `BatchPrep` per chunk, the same forwards,
the candidates read back and appended in numpy (no NMS: the alternative stops where the joint buffer is complete).

    python examples/time_slice.py [--frames 64] [--windows 5] [--min-window 1.0] [--warmup 2] [--val-conf 0.3] [--no-host]

Method of examples/time_eval.py: a figure is a host clock around `reps` calls that ends in a device synchronise, divided by `reps`;
`reps` is chosen after the warm-up so that a window lasts at least `--min-window` seconds; the median of `--windows` windows is
reported with their spread (max - min).  No accuracy is measured: the weights are procedural.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from mobilenet_yolo_pytorch_amd import _lib, ops, synthetic, yolo  # noqa: E402
from mobilenet_yolo_pytorch_amd.prep import BatchPrep  # noqa: E402
from mobilenet_yolo_pytorch_amd.slicing import Sliced, tile_grid  # noqa: E402
from oracle import procedural  # noqa: E402
from time_eval import measure  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
S, TILE, OVERLAP, BATCH = 416, 416, 0.2, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--val-conf", type=float, default=0.3)
    ap.add_argument("--no-host", action="store_true", help="skip the host-side alternative")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_slice.py needs the MI355X"
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = a.val_conf
    base = synthetic.photos([(720, 1280)] * 4, seed=0)
    frames = [base[i % 4] for i in range(a.frames)]
    sl = Sliced(m, size=S, tile=(TILE, TILE), overlap=OVERLAP, full_view=True, edge=0, batch=BATCH, mean=MEAN, std=STD)
    det = sl(frames)
    b = next(iter(sl._bufs.values()))
    src, tiles_dev, maps_dev = sl._keep
    N, Bc, chunks = a.frames, b["x"].shape[0], tiles_dev.shape[0]
    plan = m._plan(Bc, S, S, False)
    vc = [a.val_conf] * 2
    mw = (a.windows, a.min_window, a.warmup)
    res = {"frames": N, "records": 9 * N, "chunk": Bc, "chunks": chunks, "val_conf": a.val_conf, "windows": a.windows, "min_window_s": a.min_window,
           "warmup": a.warmup, "joint_candidates_per_frame": round(float(b["counts"].float().mean()), 1),
           "kept_per_frame": round(sum(len(d) for d in det) / N, 1)}
    res["pack_upload"] = measure(lambda: sl._prep.pack(frames)[0].to("cuda", non_blocking=True), *mw)
    res["prep_tiles_chunk"] = measure(lambda: ops.prep_tiles(src, tiles_dev[0], Bc, 720, 1280, S, S, sl._prep.mean, sl._prep.std, out=b["x"],
                                                             ws=b["prep_ws"]), *mw)
    res["forward_eval_chunk"] = measure(lambda: plan.forward_eval(b["x"], vc, nms=False), *mw)
    joint, counts, dropped = torch.zeros_like(b["rows"]), torch.zeros_like(b["counts"]), torch.zeros_like(b["counts"])

    def append():
        counts.zero_()
        ops.det_append_tiles(plan.rows, plan.cnt1, maps_dev[0], joint, counts, dropped)

    res["det_append_tiles_chunk"] = measure(append, *mw)
    res["det_append_tiles_chunk"]["rows_per_slot"] = round(float(plan.cnt1.float().mean()), 1)
    sl(frames)
    C, cap = m.num_classes, b["cap"]
    res["joint_nms"] = measure(lambda: _lib.call(
        "mny_nms_per_class", ops._p(b["rows"]), ops._p(b["seg_begin"]), ops._p(b["counts"]), N, N * cap, cap, C, ctypes.c_double(sl.nms_thr),
        ops._p(b["out_idx"]), ops._p(b["out"]), ops._p(b["out_rows"]), ctypes.c_void_p(b["ws"].data_ptr()), ops._st()), *mw)
    res["sliced_call"] = measure(lambda: sl(frames), *mw)
    res["forwards_sum_ms"] = round(chunks * res["forward_eval_chunk"]["ms"], 4)
    res["sliced_over_forwards"] = round(res["sliced_call"]["ms"] / res["forwards_sum_ms"], 4)
    res["sliced_minus_pack_over_forwards"] = round((res["sliced_call"]["ms"] - res["pack_upload"]["ms"]) / res["forwards_sum_ms"], 4)
    if not a.no_host:
        from PIL import Image
        _, maps, _ = sl.records(sl.originals[1])
        boxes = [(i, box) for i in range(N) for box in [(0, 0, 1280, 720)] + tile_grid(720, 1280, TILE, TILE, OVERLAP, OVERLAP)]
        R = len(boxes)
        pil = [Image.fromarray(f) for f in frames]
        bp = BatchPrep([(S, S)], MEAN, STD)
        pool = ThreadPoolExecutor(max_workers=16)
        ax, bx, ay, by = (maps[k].astype(np.float64) for k in ("ax", "bx", "ay", "by"))

        def host():
            crops = list(pool.map(lambda ib: np.asarray(pil[ib[0]].crop(ib[1])), boxes))
            crops += [crops[-1]] * (chunks * Bc - R)                                    # the last chunk padded to the plan's batch
            joint_h = [[] for _ in range(N)]
            for k in range(chunks):
                x = bp(crops[k * Bc:(k + 1) * Bc], size=(S, S))
                plan.forward_eval(x, vc, nms=False)
                rows, cnt = plan.rows.cpu().numpy(), plan.cnt1.cpu().numpy()
                for s in range(min(Bc, R - k * Bc)):
                    r, q = rows[s, :cnt[s]].copy(), k * Bc + s
                    r[:, [0, 2]] = (ax[q] + bx[q] * r[:, [0, 2]].astype(np.float64)).astype(np.float32)
                    r[:, [1, 3]] = (ay[q] + by[q] * r[:, [1, 3]].astype(np.float64)).astype(np.float32)
                    joint_h[boxes[q][0]].append(r)
            return [np.concatenate(j) for j in joint_h]

        res["host_alternative"] = measure(host, min(a.windows, 3), a.min_window, 1)
        res["host_over_sliced"] = round(res["host_alternative"]["ms"] / res["sliced_call"]["ms"], 4)
        pool.shutdown()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
