#!/usr/bin/env python3
"""Times the anchor fitting on the device (csrc/anchors.hip through mobilenet_yolo_pytorch_amd.anchors) beside the numpy restatement
tests/anchor_ref.py on the host, on two label sets: VOC-sized (about 40 k boxes, k = 6) and BDD100K-sized (about 1.3 M boxes, k = 9),
log-normal shapes.  Three figures each: k-means to convergence (max_iter = the restatement's step count, so both sides do the same
work), one fitness launch at P = 64, and a 1000-generation evolution at P = 64.

    python examples/time_anchors.py [--sets voc,bdd] [--generations 1000] [--windows 5] [--warmup 2] [--ref-generations 3] [--no-ref]

A figure is a host clock around `reps` calls that ends in a device synchronise, divided by `reps`; the median of `--windows` windows
is reported with their spread (max - min).  The restatement's evolution is timed over `--ref-generations` generations and scaled to the
full count (each generation does the same work).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mobilenet_yolo_pytorch_amd import anchors  # noqa: E402

SETS = {"voc": (40000, 6), "bdd": (1300000, 9)}
P = 64


def shapes(n, seed):
    r = np.random.default_rng(seed)
    area = np.exp(r.normal(8.3, 1.2, n))
    ratio = np.exp(r.normal(0.0, 0.45, n))
    return np.clip(np.stack((np.sqrt(area * ratio), np.sqrt(area / ratio)), 1), 2.0, 640.0).astype(np.float32)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(fn, windows, warmup, min_window=0.5):
    for _ in range(warmup):
        fn()
    reps = max(1, int(np.ceil(min_window / max(timed(fn, 1), 1e-6))))
    ts = [timed(fn, reps) * 1e3 for _ in range(windows)]
    return {"ms": round(statistics.median(ts), 4), "spread_ms": round(max(ts) - min(ts), 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="voc,bdd")
    ap.add_argument("--generations", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-generations", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true", help="skip the host passes of the restatement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_anchors.py needs the MI355X"
    res = {"P": P, "generations": a.generations, "windows": a.windows, "warmup": a.warmup}
    for name in a.sets.split(","):
        n, k = SETS[name]
        wh = shapes(n, 0)
        d = torch.from_numpy(wh).cuda()
        init = anchors.default_init(d, k)
        centres, state = anchors.kmeans(d, k, init=init, max_iter=300)
        steps, conv = state.tolist()[:2]
        r = {"boxes": n, "k": k, "kmeans_steps": steps, "kmeans_converged": bool(conv)}
        r["kmeans"] = measure(lambda: anchors.kmeans(d, k, init=init, max_iter=steps), a.windows, a.warmup)
        cand = centres[None] * torch.from_numpy(anchors.draw_factors(1, 1, P, k)[0]).cuda()
        r["fitness_P64"] = measure(lambda: anchors.fitness_counts(d, cand, 0.25), a.windows, a.warmup)
        factors = torch.from_numpy(anchors.draw_factors(0, a.generations, P, k)).cuda()
        r["evolve"] = measure(lambda: anchors.evolve(d, centres, a.generations, P, 0.25, factors=factors), a.windows, a.warmup)
        if not a.no_ref:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import anchor_ref
            i0 = init.cpu().numpy()
            t0 = time.perf_counter()
            ref = anchor_ref.kmeans(wh, i0, steps)
            r["numpy_kmeans_s"] = round(time.perf_counter() - t0, 3)
            r["kmeans_bit_equal"] = bool(ref["centres"].tobytes() == centres.cpu().numpy().tobytes())
            c0 = cand.cpu().numpy()
            t0 = time.perf_counter()
            fr, _ = anchor_ref.fitness(wh, c0, 0.25)
            r["numpy_fitness_P64_s"] = round(time.perf_counter() - t0, 3)
            r["fitness_bit_equal"] = bool(np.array_equal(fr, anchors.fitness_counts(d, cand, 0.25)[0].cpu().numpy()))
            g = max(1, a.ref_generations)
            f = factors[:g].cpu().numpy()
            t0 = time.perf_counter()
            anchor_ref.evolve(wh, ref["centres"], f, 0.25, 2.0)
            r["numpy_evolve_s_scaled"] = round((time.perf_counter() - t0) / g * a.generations, 2)
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
