"""float64 numpy restatement of the segmentation evaluator (include/mnyolo.h: mny_seg_confusion / mny_seg_upsample / mny_seg_metrics).

The rules: p = sigmoid(logit); output row Y of an image of H rows reads head rows clamp(y0) and clamp(y0 + 1) with weight ty, where
ny = (2Y+1) h - H, y0 = floor(ny / 2H), ry = ny - y0 2H (integers) and ty = ry / 2H; columns alike; v = a (1-ty) + b ty with
a = p00 (1-tx) + p01 tx, b = p10 (1-tx) + p11 tx; id = 0 unless max_c v_c > 0.5, else 1 + the lowest arg-max (a NaN never wins);
ground-truth ids above C are ignored; conf[g][pred] counts the rest.  The integer arithmetic is the device's; values are float64.

Error budget of the device's fp32 values against this file (what the GPU tests assert):
  * expf is within 1 ulp, then one add and one correctly rounded divide: p has a relative error <= 2^-22;
  * each weight (ty, tx) has one rounding, each (1 - t) one more;
  * two levels of (2 products + 1 add) on values in [0, 1]: v has an absolute error below 3 * 2^-22;
  * VALUE_TOL = 2^-19 on a value and GAP_TOL = 2^-18 on a difference of two values leave a factor of two over that.
A pixel is AMBIGUOUS when the decision could flip inside that budget: |m - 0.5| < 2^-18, or m > 0.5 and the gap to the
second-largest channel is < 2^-18.  The GPU tests compare predictions at unambiguous pixels only; `CASES` lists their inputs, and
tests/test_segeval_ref_cpu.py checks on the CPU that every case meets its ambiguity condition."""
import numpy as np

VALUE_TOL = 2.0 ** -19
GAP_TOL = 2.0 ** -18


def positions(n_out, n_in):
    """-> (i0 clamped, i1 clamped, weight) of every output index; integer arithmetic as on the device."""
    i = np.arange(n_out, dtype=np.int64)
    n = (2 * i + 1) * n_in - n_out
    i0 = n // (2 * n_out)                                   # floor division
    r = n - i0 * 2 * n_out
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), r.astype(np.float64) / float(2 * n_out)


def sigmoid(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def upsample(logits_hwc, H, W):
    """[h,w,C] logits -> [C,H,W] float64 interpolated probabilities."""
    p = sigmoid(logits_hwc)
    h, w, _ = p.shape
    y0, y1, ty = positions(H, h)
    x0, x1, tx = positions(W, w)
    tx, ty = tx[None, :, None], ty[:, None, None]
    with np.errstate(invalid="ignore"):
        a = p[y0][:, x0] * (1 - tx) + p[y0][:, x1] * tx
        b = p[y1][:, x0] * (1 - tx) + p[y1][:, x1] * tx
        v = a * (1 - ty) + b * ty
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def predict(v):
    """[C,H,W] values -> (uint8 id map, bool ambiguity mask)."""
    s = np.where(np.isnan(v), -np.inf, v)
    m = s.max(axis=0)
    pred = np.where(m > 0.5, 1 + s.argmax(axis=0), 0).astype(np.uint8)        # argmax: the first (lowest) maximum
    amb = np.abs(m - 0.5) < GAP_TOL
    if v.shape[0] > 1:
        second = np.sort(s, axis=0)[-2]
        with np.errstate(invalid="ignore"):
            amb |= (m > 0.5) & (m - second < GAP_TOL)
    return pred, amb


def confusion(pred, label, C):
    """-> (int64 [(C+1),(C+1)] with rows = ground truth, ignored count)."""
    g = label.astype(np.int64).reshape(-1)
    keep = g <= C
    conf = np.bincount(g[keep] * (C + 1) + pred.astype(np.int64).reshape(-1)[keep], minlength=(C + 1) ** 2)
    return conf.reshape(C + 1, C + 1).astype(np.int64), int((~keep).sum())


def metrics(conf):
    """-> float64 [C+4]: iou[0..C], miou, miou_fg, pixel_acc (NaN where undefined)."""
    conf = np.asarray(conf, np.int64)
    diag = np.diag(conf)
    den = conf.sum(1) + conf.sum(0) - diag
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(den > 0, diag.astype(np.float64) / den.astype(np.float64), np.nan)
        acc = np.float64(diag.sum()) / np.float64(conf.sum()) if conf.sum() else np.nan

    def mean(a):
        a = a[~np.isnan(a)]
        return a.sum() / len(a) if len(a) else np.nan
    return np.concatenate([iou, [mean(iou), mean(iou[1:]), acc]])


def evaluate(logits, labels, C):
    """logits [N,h,w,C], labels: N uint8 maps -> dict(values, preds, ambiguous, conf, ignored) over the batch."""
    vals, preds, ambs = [], [], []
    conf, ign = np.zeros((C + 1, C + 1), np.int64), 0
    for x, lab in zip(logits, labels):
        v = upsample(x, *lab.shape)
        pred, amb = predict(v)
        c, i = confusion(pred, lab, C)
        conf += c
        ign += i
        vals.append(v), preds.append(pred), ambs.append(amb)
    return {"values": vals, "preds": preds, "ambiguous": ambs, "conf": conf, "ignored": ign}


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------
# name: (kind, h, w, C, sizes, label mode, seed).  kind "exact": logits from a small asymmetric set plus per-channel offsets, the
# reference must find NO ambiguous pixel; "normal": N(0, 2) logits, at most 0.1 % ambiguous pixels.  The shapes are the smallest
# that reach every path of csrc/segeval.hip: scale 16 (aligned rows), a non-integer scale (unaligned rows), widths around the
# 16-byte piece and one-row images, labels smaller than the head, many images per launch and more than one launch (96 images per
# launch), C = 1..3 (register counters) and 5 / 16 (LDS histogram), a tile cut below 32 rows by the LDS stage (wide_down), more
# than 256 column groups per row and row bands of several rows (wide_bands).
_WIDTHS = [(1, 1), (1, 15), (1, 16), (1, 17), (1, 33), (5, 1), (7, 15), (3, 16), (9, 17), (4, 33), (2, 3), (50, 17)]


def _mixed(n, seed, top=40):
    r = np.random.RandomState(seed)
    return [(int(a), int(b)) for a, b in zip(r.randint(1, top + 1, n), r.randint(1, top + 1, n))]


CASES = {
    "scale16_c2": ("exact", 3, 5, 2, [(48, 80)], "random", 1),
    "nonint_c2": ("exact", 4, 7, 2, [(50, 90), (48, 80), (50, 90)], "random", 2),
    "widths_c3": ("exact", 4, 7, 3, _WIDTHS, "random", 3),
    "many70_c2": ("exact", 4, 7, 2, _mixed(70, 4), "random", 4),
    "many100_c1": ("exact", 3, 5, 1, _mixed(100, 5, 24), "random", 5),
    "scale16_c5": ("exact", 3, 5, 5, [(48, 80), (33, 47)], "random", 6),
    "nonint_c16": ("exact", 4, 7, 16, [(50, 90), (7, 15), (1, 17)], "random", 7),
    "wide_down_c16": ("exact", 64, 48, 16, [(4, 6), (40, 30)], "random", 8),
    "wide_bands_c2": ("exact", 3, 5, 2, [(2, 4200), (40, 300), (33, 130)], "random", 9),
    "wide_bands_c5": ("normal", 3, 5, 5, [(2, 4200), (40, 300)], "random", 15),
    "normal_c2": ("normal", 4, 7, 2, [(50, 90), (48, 80), (17, 33)], "random", 11),
    "normal_c3": ("normal", 3, 5, 3, [(48, 80)] + _mixed(20, 12), "random", 12),
    "normal_c5": ("normal", 4, 7, 5, [(50, 90), (33, 47)], "random", 13),
    "normal_c16": ("normal", 4, 7, 16, _mixed(12, 14), "random", 14),
    "all_background": ("exact", 3, 5, 2, [(48, 80), (9, 17)], "background", 21),
    "all_one_class": ("exact", 3, 5, 2, [(48, 80), (9, 17)], "class2", 22),
    "all_ignored": ("exact", 3, 5, 2, [(48, 80), (9, 17)], "ignored", 23),
    "nan_inf_c2": ("exact", 4, 7, 2, [(50, 90), (4, 7)], "random", 24),
    "nan_inf_c5": ("exact", 4, 7, 5, [(50, 90), (4, 7)], "random", 25),
}


def make_case(name):
    """-> (logits float32 [N,h,w,C], labels: list of uint8 [H_i,W_i]); deterministic."""
    kind, h, w, C, sizes, mode, seed = CASES[name]
    r = np.random.RandomState(seed)
    N = len(sizes)
    if kind == "exact":
        offs = 0.07 * np.arange(C) - 0.4 + 0.013 * (np.arange(C) % 3)
        x = r.choice(np.array([-3.0, -1.0, 2.0, 5.0]), size=(N, h, w, C)) + offs
    else:
        x = r.normal(0.0, 2.0, size=(N, h, w, C))
    x = x.astype(np.float32)
    if name.startswith("nan_inf"):
        x[0, 1, 2, 0] = np.nan
        x[0, 2, 5, C - 1] = np.inf
        x[0, 3, 1, 0] = -np.inf
        x[1, 0, 0, :] = np.nan                              # every channel NaN: background
    labels = []
    for (H, W) in sizes:
        if mode == "background":
            lab = np.zeros((H, W), np.uint8)
        elif mode == "class2":
            lab = np.full((H, W), 2, np.uint8)
        elif mode == "ignored":
            lab = np.full((H, W), 255, np.uint8)
        else:
            lab = r.randint(0, C + 1, size=(H, W)).astype(np.uint8)
            lab[r.rand(H, W) < 0.05] = 255
            lab[r.rand(H, W) < 0.02] = C + 1                # the smallest ignored id
        labels.append(lab)
    return x, labels


def ambiguity_ok(name, res):
    """The input condition of a case: exact -> no ambiguous pixel, normal -> at most 0.1 % of the pixels."""
    n_amb = sum(int(a.sum()) for a in res["ambiguous"])
    n_pix = sum(a.size for a in res["ambiguous"])
    return (n_amb == 0) if CASES[name][0] == "exact" else (n_amb <= 1e-3 * n_pix), n_amb, n_pix
