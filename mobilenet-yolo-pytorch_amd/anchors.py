"""Anchors fitted to a label set on the device ("autoanchor"): k-means under the shape IoU, the fitness and best-possible recall of
candidate anchor sets, a mutation search, and a census of what the YOLO loss's target assignment will do with a set of anchors.

The reference ships hand-tuned anchors per dataset (models/voc/config.yaml, models/bdd100k/config.yaml) and assigns positives purely
from the IoU of [0,0,w,h] against them (models/yolo_loss.py:132-145: the best of all anchors, or any above iou_thresh), so anchors that
do not fit a dataset cost recall silently.  It has no code that fits them: the arithmetic here is specified in include/mnyolo.h
("Anchor fitting"), runs in csrc/anchors.hip and is restated in tests/anchor_ref.py.  k-means and the search are NOT pinned against any
third-party implementation; the census is pinned against the loss kernel and, through the oracle, the reference's get_target.

    fit = anchors.autoanchor(label_list, config)            # label_list: [n_i,5] tensors (label, cx, cy, w, h), relative
    config["yolo"]["anchors"], config["yolo"]["mask"] = fit["anchors"], fit["mask"]
    model = yolo(config)                                    # the anchors of a live model are not changed: build a new one

There is no CPU fallback: without libmnyolo.so every call raises MnyError.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, query

MIN_SIDE, MAX_SIDE = 2.0 ** -20, 65536.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pair(img_size):
    if isinstance(img_size, (int, float)):
        return float(img_size), float(img_size)
    a, b = img_size
    return float(a), float(b)


def _pack_targets(targets, device=None):
    """list of [n_i,5] tensors / arrays, or one packed [T,5] tensor -> fp32 [T,5] on the device (one upload)."""
    if isinstance(targets, (list, tuple)):
        parts = [t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t)) for t in targets]
        parts = [t.reshape(-1, 5) for t in parts if t.numel()]
        if device is None:
            device = next((t.device for t in parts if t.device.type == "cuda"), torch.device("cuda", torch.cuda.current_device()))
        if not parts:
            return torch.zeros(0, 5, device=device)
        if all(t.device.type == "cpu" for t in parts):
            return torch.cat(parts).to(torch.float32).to(device, non_blocking=True)
        return torch.cat([t.to(device) for t in parts]).to(torch.float32)
    t = targets if isinstance(targets, torch.Tensor) else torch.as_tensor(np.asarray(targets))
    if t.dim() != 2 or t.shape[1] != 5:
        raise ValueError("packed targets must be [T,5] = (label, cx, cy, w, h), got %s" % (tuple(t.shape),))
    if device is None:
        device = t.device if t.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    return t.to(device).to(torch.float32).contiguous()


def wh_from_targets(targets, img_size, offsets=None):
    """The (w, h) of every label in pixels: fp32 [N,2] on the device.  `targets` is the list of [n_i,5] tensors the model takes, or a
    packed [T,5] tensor (its `offsets`, as the loss takes them, are accepted and not needed); img_size = side or (w, h).  The product
    relative size * img_size is one fp32 multiplication."""
    t = _pack_targets(targets)
    w, h = _pair(img_size)
    return (t[:, 3:5] * torch.tensor([w, h], dtype=torch.float32, device=t.device)).contiguous()


def _wh(wh):
    if not isinstance(wh, torch.Tensor) or wh.dim() != 2 or wh.shape[1] != 2:
        raise ValueError("wh must be a [N,2] tensor of (w, h) in pixels")
    if wh.device.type != "cuda":
        raise RuntimeError("anchor fitting needs CUDA tensors (the HIP path is the only path)")
    wh = wh.detach().to(torch.float32).contiguous()
    if wh.data_ptr() % 16:
        wh = wh.clone()
    return wh


def _ws(k, P, device):
    return torch.empty(query("mny_anchor_ws_bytes", int(k), int(P)) // 8 + 2, device=device, dtype=torch.int64)


def default_init(wh, k):
    """The shapes at the (2i+1)/(2k) quantiles of a stable sort of the valid boxes by fp32 area: [k,2] on the device, no host sync.
    (torch plumbing; an invalid box sorts last.)"""
    wh = _wh(wh)
    ok = ((wh >= MIN_SIDE) & (wh <= MAX_SIDE)).all(1)
    area = torch.where(ok, wh[:, 0] * wh[:, 1], torch.full_like(wh[:, 0], float("inf")))
    order = torch.sort(area, stable=True)[1]
    m = ok.sum()
    idx = ((2 * torch.arange(k, device=wh.device) + 1) * m) // (2 * k)
    return wh[order[idx.clamp(max=wh.shape[0] - 1)]].contiguous()


def kmeans(wh, k, init=None, max_iter=300, with_labels=False):
    """-> (centres [k,2] fp32, state int64[4] = {steps until convergence, converged, skipped, 0}), both on the device, no host sync.
    with_labels=True appends (labels int32 [N], -1 for a skipped box, and best_iou fp32 [N])."""
    wh = _wh(wh)
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError("k = %d outside 1..32" % k)
    centres = default_init(wh, k) if init is None else torch.as_tensor(init, dtype=torch.float32).to(wh.device).reshape(-1, 2).clone()
    if centres.shape[0] != k:
        raise ValueError("init holds %d centres, k = %d" % (centres.shape[0], k))
    N = wh.shape[0]
    labels = torch.empty(max(N, 1), device=wh.device, dtype=torch.int32)
    best = torch.empty(max(N, 1), device=wh.device, dtype=torch.float32) if with_labels else None
    state = torch.empty(4, device=wh.device, dtype=torch.int64)
    ws = _ws(k, 1, wh.device)
    call("mny_anchor_kmeans", _p(wh), N, _p(centres), k, int(max_iter), _p(labels), _p(best), _p(state), _p(ws), _st())
    return (centres, state, labels[:N], best[:N]) if with_labels else (centres, state)


def _cands(candidates, device):
    c = torch.as_tensor(candidates, dtype=torch.float32).to(device)
    if c.dim() == 2:
        c = c[None]
    if c.dim() != 3 or c.shape[2] != 2:
        raise ValueError("candidates must be [P,k,2] or [k,2], got %s" % (tuple(c.shape),))
    return c.contiguous()


def fitness_counts(wh, candidates, thr=0.25):
    """-> (FR int64 [P,2] = (sum of qi(best IoU) over the boxes above thr, their count), valid int64 [1]); device, no host sync."""
    wh = _wh(wh)
    c = _cands(candidates, wh.device)
    fr = torch.empty(c.shape[0], 2, device=wh.device, dtype=torch.int64)
    valid = torch.empty(1, device=wh.device, dtype=torch.int64)
    call("mny_anchor_fitness", _p(wh), wh.shape[0], _p(c), c.shape[0], c.shape[1], float(thr), _p(fr), _p(valid), _st())
    return fr, valid


def fitness(wh, candidates, thr=0.25):
    """-> (mean best IoU [P], recall [P]) as float64 device tensors, no host sync: per candidate set [k,2], the mean over the valid
    boxes of the best IoU where it exceeds `thr` (thr = 0: the plain mean best IoU), and the share of boxes whose best IoU does."""
    fr, valid = fitness_counts(wh, candidates, thr)
    n = valid.to(torch.float64)
    return fr[:, 0].to(torch.float64) * 2.0 ** -32 / n, fr[:, 1].to(torch.float64) / n


def draw_factors(seed, G, P, k, mutation_prob=0.9, sigma=0.1):
    """The mutation factors of `evolve`: fp32 [G,P,k,2].  One numpy.random.Generator(PCG64(seed)); a mask (uniform < mutation_prob), a
    per-candidate scale (uniform) and normals, in that order, each in one call; factor = 1 + mask * scale * normal * sigma, clipped to
    [0.3, 3.0].  Not part of the ABI: any factors can be handed to evolve(factors=...)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mask = rng.random((G, P, k, 2)) < mutation_prob
    scale = rng.random((G, P, 1, 1))
    normal = rng.standard_normal((G, P, k, 2))
    return np.clip(1.0 + mask * scale * normal * sigma, 0.3, 3.0).astype(np.float32)


def evolve(wh, anchors, generations=1000, population=64, thr=0.25, seed=0, min_size=2.0, factors=None):
    """Mutation search from `anchors` [k,2]: every generation scores `population` candidates (the parent and population - 1 mutants)
    in one launch and keeps the best, so the fitness never decreases.  -> (anchors [k,2] fp32, history int64 [G,2] = (winning F, its
    index)), on the device, no host sync."""
    wh = _wh(wh)
    a = torch.as_tensor(anchors, dtype=torch.float32).to(wh.device).reshape(-1, 2).contiguous()
    k, G, P = a.shape[0], int(generations), int(population)
    if factors is None:
        factors = draw_factors(seed, G, P, k)
    f = torch.as_tensor(factors, dtype=torch.float32)
    if tuple(f.shape) != (G, P, k, 2):
        raise ValueError("factors must be [%d,%d,%d,2], got %s" % (G, P, k, tuple(f.shape)))
    f = f.to(wh.device, non_blocking=True).contiguous()
    out = torch.empty_like(a)
    history = torch.empty(G, 2, device=wh.device, dtype=torch.int64)
    ws = _ws(k, P, wh.device)                      # 0 bytes for a k or P out of range: the call below refuses them before any launch
    call("mny_anchor_evolve", _p(wh), wh.shape[0], _p(a), k, _p(f), G, P, float(thr), float(min_size), _p(out), _p(history), _p(ws), _st())
    return out, history


def scale_anchors(anchors, img_size, device):
    """Pixel anchors -> fp32 [n,2] relative to the image exactly as the loss plan forms them: (aw / img_size[0], ah / img_size[1]) in
    double precision, rounded once to fp32."""
    a, b = _pair(img_size)
    t = torch.as_tensor(anchors).to(device).to(torch.float64).reshape(-1, 2)
    return (t / torch.tensor([a, b], dtype=torch.float64, device=device)).to(torch.float32).contiguous()


def census(targets, anchors, mask, iou_thresh, img_size, grids):
    """What the loss's target assignment (mny_yolo_loss) will do with `anchors` (pixels, [n,2]) on `targets`: heads mask[H][A] with
    grid sizes grids[H].  -> {"best": [n] histogram of the best anchor, "pos": [H,A] positives per head and anchor slot (pos[h].sum()
    is the loss's count of head h), "orphans": [1] targets no head takes, "outside": [H]} as int64 device tensors, no host sync."""
    t = _pack_targets(targets)
    a = scale_anchors(anchors, img_size, t.device)
    m = np.ascontiguousarray(mask, np.int32)
    if m.ndim != 2:
        raise ValueError("mask must be [H][A] with as many anchors in every head")
    g = np.ascontiguousarray(grids, np.int32).reshape(-1)
    if len(g) != m.shape[0]:
        raise ValueError("%d grids for %d heads" % (len(g), m.shape[0]))
    n, (H, A) = a.shape[0], m.shape
    out = torch.empty(n + H * A + 1 + H, device=t.device, dtype=torch.int64)
    call("mny_anchor_census", _p(t) if t.shape[0] else None, t.shape[0], _p(a), n, _hp(m), _hp(g), H, A, float(iou_thresh), _p(out), _st())
    return {"best": out[:n], "pos": out[n:n + H * A].view(H, A), "orphans": out[n + H * A:n + H * A + 1], "outside": out[n + H * A + 1:]}


def autoanchor(targets, config, k=None, max_iter=300, generations=1000, population=64, thr=0.25, seed=0, min_size=2.0, strides=(32, 16)):
    """Fit config["yolo"]'s anchors to `targets`: shapes at config["img_w"], k-means, evolve, sort by area descending (the config lists
    the largest anchors first and head 0, the coarsest grid, owns them), round to integers.
    -> {"anchors": [[w,h]] * k, "mask": [[0..A-1], [A..2A-1], ...], "report": {...}} ready for config["yolo"].
    report: mean best IoU ("fitness") and recall at `thr`, and the census, for the config's own anchors ("before", when it has k of
    them), the k-means centres, the evolved anchors and the rounded result.  Building the report is the only host synchronisation."""
    y = config["yolo"]
    heads = len(y["mask"])
    k = int(k) if k is not None else len(y["anchors"])
    if k % heads:
        raise ValueError("k = %d anchors do not divide among %d heads" % (k, heads))
    A = k // heads
    img = (config["img_w"], config["img_h"])
    t = _pack_targets(targets)
    wh = wh_from_targets(t, config["img_w"])
    centres, state = kmeans(wh, k, max_iter=max_iter)
    evolved, history = evolve(wh, centres, generations, population, thr, seed, min_size)

    def by_area(a):
        return a[torch.sort(a[:, 0] * a[:, 1], descending=True, stable=True)[1]]

    centres_s, evolved_s = by_area(centres), by_area(evolved)
    final = by_area(torch.clamp(torch.round(evolved_s), min=1.0))
    mask = [list(range(h * A, (h + 1) * A)) for h in range(heads)]
    grids = [int(config["img_w"]) // int(s) for s in strides[:heads]]
    if len(grids) != heads:
        raise ValueError("%d strides for %d heads" % (len(strides), heads))
    stages = [("kmeans", centres_s), ("evolved", evolved_s), ("rounded", final)]
    before_mask = None
    if len(y["anchors"]) == k and all(len(m) == A for m in y["mask"]):
        stages.insert(0, ("before", torch.tensor(y["anchors"], dtype=torch.float32, device=wh.device)))
        before_mask = y["mask"]
    fit, rec = fitness(wh, torch.stack([a for _, a in stages]), thr)
    cens = [census(t, a, before_mask if name == "before" else mask, y["iou_thresh"], img, grids) for name, a in stages]
    # ---- the one synchronisation ----
    fit, rec = fit.tolist(), rec.tolist()
    st = state.tolist()
    report = {"boxes": int(wh.shape[0]), "skipped": st[2], "thr": float(thr), "grids": grids,
              "kmeans_steps": st[0], "kmeans_converged": bool(st[1]), "evolve_improved": int((history[:, 1] != 0).sum())}
    for i, (name, a) in enumerate(stages):
        c = {key: v.tolist() for key, v in cens[i].items()}
        report[name] = {"anchors": a.tolist(), "fitness": fit[i], "recall": rec[i], "best": c["best"], "pos": c["pos"],
                        "orphans": c["orphans"][0], "outside": c["outside"]}
    return {"anchors": [[int(w), int(h)] for w, h in final.tolist()], "mask": mask, "report": report}
