"""Thin torch-tensor wrappers over the C ABI (include/mnyolo.h).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic op is a HIP kernel
of libmnyolo.so.  All tensors are contiguous, on a CUDA(=HIP) device; activations are NHWC, fp32 or — selecting the
`*_bf16` twins of the entry points — bf16; weights, BN coefficients, statistics and workspaces are always fp32.
A `view` is the tuple (tensor, scale|None, shift|None, act) — see mnyolo.h "View arguments".
"""
import ctypes

import torch

from . import _lib
from ._lib import ACT_NONE, YoloHead, call, query

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype in (torch.float32, torch.int32, torch.bfloat16) and t.is_contiguous(), \
        "libmnyolo needs contiguous fp32/bf16/int32 device tensors (got %s %s)" % (t.device, t.dtype)
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _new(*shape, like=None, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def _k(name, t):
    """entry point for the storage type of activation tensor `t`"""
    return name + "_bf16" if t.dtype == torch.bfloat16 else name


# ---- stem -------------------------------------------------------------------------------------------
def stem_fwd(x_nchw, w, want_stats=True, dtype=torch.float32):
    N, _, H, W = x_nchw.shape
    Co = w.shape[0]
    y = _new(N, (H + 1) // 2, (W + 1) // 2, Co, like=x_nchw, dtype=dtype)
    parts = query("mny_stem_stat_parts", N, H, W, Co)
    stats = _new(parts, 2, Co, like=x_nchw) if want_stats else None
    call(_k("mny_stem_fwd", y), _p(x_nchw), _p(w), _p(y), _p(stats), N, H, W, Co, _st())
    return y, stats


def stem_wgrad(x_nchw, dy):
    N, _, H, W = x_nchw.shape
    Co = dy.shape[3]
    parts = query("mny_stem_wgrad_parts", N, H, W, Co)
    ws = _new(parts, Co * 27, like=dy)
    dw = _new(Co, 3, 3, 3, like=dy)
    call(_k("mny_stem_wgrad", dy), _p(x_nchw), _p(dy), _p(dw), _p(ws), N, H, W, Co, _st())
    return dw


def stem_bnwgrad(x_nchw, g, y, scale, shift, act, gamma, mean, invstd):
    """Stem weight gradient from the unit's output gradient g (BN-backward-apply redone on load). -> (dw, dgamma, dbeta)"""
    N, _, H, W = x_nchw.shape
    Co = y.shape[3]
    M = y.numel() // Co
    parts = query("mny_bn_bwd_parts", M, Co)
    red = _new(parts, 2, Co, like=gamma)
    call(_k("mny_bn_bwd_reduce", y), _p(g), _p(y), _p(scale), _p(shift), act, _p(mean), _p(invstd), _p(red), M, Co, _st())
    dgamma, dbeta, coef = _new(Co, like=gamma), _new(Co, like=gamma), _new(3, Co, like=gamma)
    call("mny_bn_bwd_finalize", _p(red), parts, M, _p(gamma), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(coef), Co, _st())
    ws = _new(query("mny_stem_wgrad_parts", N, H, W, Co), Co * 27, like=gamma)
    dw = _new(Co, 3, 3, 3, like=gamma)
    call(_k("mny_stem_bnwgrad", y), _p(x_nchw), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(dw), _p(ws), N, H, W, Co, _st())
    return dw, dgamma, dbeta


# ---- depthwise --------------------------------------------------------------------------------------
def dw_fwd(view, w, stride, want_stats=True):
    x, sc, sh, act = view
    N, H, W, C = x.shape
    K = w.shape[-1]
    Ho, Wo = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
    y = _new(N, Ho, Wo, C, like=x, dtype=x.dtype)
    stats = _new(query("mny_dw_stat_parts_x", N, H, W, C, K, stride, 1 if x.dtype == torch.bfloat16 else 0), 2, C, like=x) if want_stats else None
    call(_k("mny_dw_fwd", x), _p(x), _p(sc), _p(sh), act, _p(w), _p(y), _p(stats), N, H, W, C, K, stride, _st())
    return y, stats


def dw_bwd_data(dy, w, in_hw, stride, addend=None, out=None):
    N, _, _, C = dy.shape
    H, W = in_hw
    K = w.shape[-1]
    dx = out if out is not None else _new(N, H, W, C, like=dy, dtype=dy.dtype)
    call(_k("mny_dw_bwd_data", dy), _p(dy), _p(w), _p(addend), _p(dx), N, H, W, C, K, stride, _st())
    return dx


def dw_bwd_weight(view, dy, K, stride):
    x, sc, sh, act = view
    N, H, W, C = x.shape
    ws = _new(query("mny_dw_wgrad_parts", N, H, W, C, K, stride), C * K * K, like=x)
    dw = _new(C, 1, K, K, like=x)
    call(_k("mny_dw_bwd_weight", x), _p(x), _p(sc), _p(sh), act, _p(dy), _p(dw), _p(ws), N, H, W, C, K, stride, _st())
    return dw


def dw_bnbwd(g, y, scale, shift, act, coef, xview, w, addend=None, in_stats=None):
    """Fused BN-backward-apply + dw weight/data gradient of a 3x3 stride-1 unit -> (dx, dw).
    in_stats = (mean, invstd) of the unit that produced x: also returns that unit's BN-backward partial sums [parts,2,C]."""
    x, xs, xh, xact = xview
    N, H, W, C = x.shape
    k = w.shape[-1]                                     # 3, or 5 (tile form)
    parts = query("mny_dw_bnbwd_parts_k", N, H, W, C, k, (1 if x.dtype == torch.bfloat16 else 0) | (2 if in_stats is not None else 0))
    ws = _new(parts, C * k * k, like=x)
    dx = torch.empty_like(x)
    dw = _new(C, 1, k, k, like=x)
    if in_stats is None:
        call(_k("mny_dw_bnbwd", x), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(x), _p(xs), _p(xh), xact, _p(w), _p(addend), _p(dx),
             _p(dw), _p(ws), N, H, W, C, k, 1, _st())
        return dx, dw
    red = _new(parts, 2, C, like=x)
    call(_k("mny_dw_bnbwd_red", x), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(x), _p(xs), _p(xh), xact, _p(in_stats[0]), _p(in_stats[1]),
         _p(w), _p(addend), _p(dx), _p(dw), _p(ws), _p(red), N, H, W, C, k, 1, _st())
    return dx, dw, red


def dw_bnbwd_s2(g, y, scale, shift, act, coef, xview, w, addend=None):
    """Fused BN-backward-apply + weight / data gradient of a 3x3 STRIDE-2 depthwise unit -> (dx, dw)."""
    x, xs, xh, xact = xview
    N, H, W, C = x.shape
    ws = _new(query("mny_dw_bnbwd_s2_parts", N, H, W, C), C * 9, like=x)
    dx = torch.empty_like(x)
    dw = _new(C, 1, 3, 3, like=x)
    call(_k("mny_dw_bnbwd_s2", x), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(x), _p(xs), _p(xh), xact, _p(w), _p(addend), _p(dx),
         _p(dw), _p(ws), N, H, W, C, _st())
    return dx, dw


def dw_bnbwd_s2k5(g, y, scale, shift, act, coef, xview, w, addend=None, in_stats=None):
    """Fused BN-backward-apply + weight / data gradient of a 5x5 STRIDE-2 depthwise unit -> (dx, dw) or, with in_stats = (mean, invstd) of the
    unit that produced x, (dx, dw, red[parts, 2, C]): that unit's BN-backward sums as partial rows."""
    x, xs, xh, xact = xview
    N, H, W, C = x.shape
    parts = query("mny_dw_bnbwd_s2k5_parts", N, H, W, C)
    ws = _new(parts, C * 25, like=w)
    dx = torch.empty_like(x)
    dw = _new(C, 1, 5, 5, like=w)
    red = _new(parts, 2, C, like=w) if in_stats is not None else None
    mu, istd = in_stats if in_stats is not None else (None, None)
    call(_k("mny_dw_bnbwd_s2k5", x), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(x), _p(xs), _p(xh), xact, _p(mu), _p(istd), _p(w), _p(addend),
         _p(dx), _p(dw), _p(ws), _p(red), N, H, W, C, _st())
    return (dx, dw) if red is None else (dx, dw, red)


# ---- pointwise --------------------------------------------------------------------------------------
def pw_fwd(view, w2d, bias=None, addend=None, want_stats=True, out=None):
    """bf16 activations take bf16 weights (mny_pw_fwd_bf16)."""
    x, sc, sh, act = view
    assert w2d.dtype == x.dtype, "pw_fwd: weight dtype %s must match the activation storage type %s" % (w2d.dtype, x.dtype)
    K = x.shape[-1]
    M = x.numel() // K
    Nc = w2d.shape[0]
    y = out if out is not None else _new(*x.shape[:-1], Nc, like=x, dtype=x.dtype)
    stats = _new(query(_k("mny_pw_stat_parts", x), M, K, Nc), 2, Nc, like=x) if want_stats else None
    call(_k("mny_pw_fwd", x), _p(x), _p(sc), _p(sh), act, _p(w2d), _p(bias), _p(addend), _p(y), _p(stats), M, K, Nc, _st())
    return y, stats


def pw_wgrad(view, dy, want_dbias=False):
    x, sc, sh, act = view
    K = x.shape[-1]
    M = x.numel() // K
    Nc = dy.shape[-1]
    ws = _new(query("mny_pw_wgrad_ws_floats", M, K, Nc), like=x)
    dw = _new(Nc, K, like=x)
    db = _new(Nc, like=x) if want_dbias else None
    call(_k("mny_pw_wgrad", x), _p(x), _p(sc), _p(sh), act, _p(dy), _p(dw), _p(db), _p(ws), M, K, Nc, _st())
    return dw, db


def pw_bnbwd(g, y, scale, shift, act, mean, invstd, gamma, xview, w2d, addend=None, want_dx=True):
    """Fused BN-backward + wgrad + dgrad of a thin expand unit -> (dx|None, dw, dgamma, dbeta)."""
    x, xs, xh, xact = xview
    K, Nc = x.shape[-1], y.shape[-1]
    M = y.numel() // Nc
    assert query(_k("mny_pw_bnbwd_supported", y), M, K, Nc) == 1
    ws = _new(query("mny_pw_bnbwd_ws_floats", M, K, Nc), like=y, dtype=torch.float32)
    dx = torch.empty_like(x) if want_dx else None
    dw, dgamma, dbeta = _new(Nc, K, like=y, dtype=torch.float32), _new(Nc, like=y, dtype=torch.float32), _new(Nc, like=y, dtype=torch.float32)
    call(_k("mny_pw_bnbwd", y), _p(g), _p(y), _p(scale), _p(shift), act, _p(mean), _p(invstd), _p(gamma), _p(x), _p(xs), _p(xh), xact,
         _p(w2d), _p(addend), _p(dx), _p(dw), _p(dgamma), _p(dbeta), _p(ws), M, K, Nc, _st())
    return dx, dw, dgamma, dbeta


def pw_dgrad_bnred(dy, wT, y_unit, scale, shift, act, mean, invstd, addend=None):
    """dx = dy @ W (wT = [Nc][K]) [+ addend] and the BN-backward partial sums of the unit whose (complete) output gradient dx is.
    -> (dx [M,Nc], red [parts,2,Nc])"""
    M, K = dy.numel() // dy.shape[-1], dy.shape[-1]
    Nc = wT.shape[0]
    parts = query("mny_pw_dgrad_bnred_parts", M, K, Nc)
    dx = torch.empty(*dy.shape[:-1], Nc, device=dy.device, dtype=torch.float32)
    red = torch.empty(parts, 2, Nc, device=dy.device, dtype=torch.float32)
    if addend is None:
        call("mny_pw_dgrad_bnred", _p(dy), _p(wT), _p(dx), _p(y_unit), _p(scale), _p(shift), int(act), _p(mean), _p(invstd), _p(red), M, K, Nc, _st())
    else:
        call("mny_pw_dgrad_bnred_add", _p(dy), _p(wT), _p(addend), _p(dx), _p(y_unit), _p(scale), _p(shift), int(act), _p(mean), _p(invstd), _p(red),
             M, K, Nc, _st())
    return dx, red


def transpose(w2d, dtype=torch.float32):
    R, C = w2d.shape
    out = _new(C, R, like=w2d, dtype=dtype)
    call(_k("mny_transpose", out), _p(w2d), _p(out), R, C, _st())
    return out


# ---- batch norm -------------------------------------------------------------------------------------
def bn_finalize(stats, count, gamma, beta, running_mean=None, running_var=None):
    C = gamma.numel()
    scale, shift, mean, invstd = (_new(C, like=gamma) for _ in range(4))
    call("mny_bn_finalize", _p(stats), stats.shape[0], count, _p(gamma), _p(beta), BN_EPS, BN_MOMENTUM,
         _p(running_mean), _p(running_var), _p(scale), _p(shift), _p(mean), _p(invstd), C, _st())
    return scale, shift, mean, invstd


def bn_eval_coeffs(gamma, beta, rm, rv):
    C = gamma.numel()
    scale, shift = _new(C, like=gamma), _new(C, like=gamma)
    call("mny_bn_eval_coeffs", _p(gamma), _p(beta), _p(rm), _p(rv), BN_EPS, _p(scale), _p(shift), C, _st())
    return scale, shift


def bn_backward(g, y, scale, shift, act, gamma, mean, invstd, out=None):
    """-> (dy, dgamma, dbeta) for z = scale*y+shift, a = act(z), given g = dL/da."""
    C = y.shape[-1]
    M = y.numel() // C
    parts = query("mny_bn_bwd_parts", M, C)
    red = _new(parts, 2, C, like=y)
    call(_k("mny_bn_bwd_reduce", y), _p(g), _p(y), _p(scale), _p(shift), act, _p(mean), _p(invstd), _p(red), M, C, _st())
    dgamma, dbeta, coef = _new(C, like=y), _new(C, like=y), _new(3, C, like=y)
    call("mny_bn_bwd_finalize", _p(red), parts, M, _p(gamma), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(coef), C, _st())
    dy = out if out is not None else torch.empty_like(y)
    call(_k("mny_bn_bwd_apply", y), _p(g), _p(y), _p(scale), _p(shift), act, _p(coef), _p(dy), M, C, _st())
    return dy, dgamma, dbeta


# ---- glue -------------------------------------------------------------------------------------------
def add_views(a, b=None, up=None, out=None):
    x = a[0]
    N, H, W, C = x.shape
    o = out if out is not None else torch.empty_like(x)
    bt, bsc, bsh, bact = b if b is not None else (None, None, None, ACT_NONE)
    call(_k("mny_add_views", x), _p(a[0]), _p(a[1]), _p(a[2]), a[3], _p(bt), _p(bsc), _p(bsh), bact, _p(up), _p(o), N, H, W, C, _st())
    return o


def upsample_bwd(src, dst=None, accumulate=False):
    N, H, W, C = src.shape
    d = dst if dst is not None else _new(N, H // 2, W // 2, C, like=src, dtype=src.dtype)
    call(_k("mny_upsample_bwd", src), _p(src), _p(d), int(accumulate), N, H, W, C, _st())
    return d


def axpy(src, dst, alpha=None, accumulate=False):
    call(_k("mny_axpy", src), _p(src), _p(alpha), _p(dst), int(accumulate), src.numel(), _st())
    return dst


# ---- detection --------------------------------------------------------------------------------------
def make_head(N, g, A, C, n_anchors_all, ignore_thresh, iou_thresh, iou_weighting):
    return YoloHead(N, g, A, C, n_anchors_all, ignore_thresh, iou_thresh, iou_weighting)


def yolo_loss(head, targets, t_off, anchors_all, mask, hp, ws=None):
    """head [N,g,g,A*(5+C)] -> (out7 [7] device tensor, dhead).  `ws`: a caller's uint8 workspace of at least
    mny_yolo_loss_ws_bytes (its contents do not matter: every field is written before it is read)."""
    nbytes = query("mny_yolo_loss_ws_bytes", ctypes.byref(hp), 0)
    if ws is None:
        ws = torch.empty(nbytes, device=head.device, dtype=torch.uint8)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes, "yolo_loss: workspace too small"
    out7 = _new(7, like=head)
    dhead = torch.empty_like(head)
    call("mny_yolo_loss", _p(head), _p(targets), _p(t_off), _p(anchors_all), _p(mask), ctypes.byref(hp),
         _p(out7), _p(dhead), ctypes.c_void_p(ws.data_ptr()), _st())
    return out7, dhead


def yolo_decode(head, anchors_all, mask, hp, val_conf, rows=None, row_stride=None, base_counts=None):
    cells = hp.A * hp.g * hp.g
    row_stride = row_stride or cells
    if rows is None:
        rows = _new(hp.N, row_stride, 7, like=head)
    counts = _new(hp.N, like=head, dtype=torch.int32)
    call("mny_yolo_decode", _p(head), _p(anchors_all), _p(mask), ctypes.byref(hp), float(val_conf), _p(rows), int(row_stride),
         _p(base_counts), _p(counts), _st())
    return rows, counts


def nms_per_class(rows, seg_begin, seg_count, num_classes, thr=0.45, max_seg_rows=0, gather=True):
    """rows [capacity,7]; seg_begin/seg_count int32 [S] (device).
    -> (out_idx int32 [capacity], out_counts int32 [S], out_rows [capacity,7]|None, prefix int32 [S+1], status int32 [1])"""
    capacity = rows.shape[0]
    S = seg_begin.numel()
    nbytes = query("mny_nms_ws_bytes", S, capacity, num_classes)
    ws = torch.empty(nbytes, device=seg_begin.device, dtype=torch.uint8)
    out_idx = torch.empty(max(capacity, 1), device=seg_begin.device, dtype=torch.int32)
    out_counts = torch.empty(S, device=seg_begin.device, dtype=torch.int32)
    out_rows = torch.empty(max(capacity, 1), 7, device=seg_begin.device) if gather else None
    call("mny_nms_per_class", _p(rows) if capacity else None, _p(seg_begin), _p(seg_count), S, capacity, int(max_seg_rows), num_classes,
         float(thr), _p(out_idx), _p(out_counts), _p(out_rows), ctypes.c_void_p(ws.data_ptr()), _st())
    so = query("mny_nms_status_offset", S, capacity, num_classes)
    po = query("mny_nms_prefix_offset", S, capacity, num_classes)
    status = ws[so:so + 4].view(torch.int32)
    prefix = ws[po:po + 4 * (S + 1)].view(torch.int32)
    return out_idx, out_counts, out_rows, prefix, status


# ---- post-processing options (csrc/postproc.hip) ----------------------------------------------------
def class_mask(classes, num_classes, device):
    """The DEVICE uint32 words of mny_yolo_decode_ex's class filter: bit (c & 31) of word (c >> 5) for every c in `classes`."""
    words = [0] * ((int(num_classes) + 31) // 32)
    for c in classes:
        words[c >> 5] |= 1 << (c & 31)
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).to(device)


def yolo_decode_ex(head, anchors_all, mask, hp, obj_thr, score_thr=-1.0, multi_label=False, class_mask=None, rows=None, row_stride=None,
                   base_counts=None):
    """-> (rows [N,row_stride,7], counts int32 [N], dropped int32 [N]).  row_stride defaults to the worst case of the mode."""
    cells = hp.A * hp.g * hp.g
    row_stride = row_stride or cells * (hp.C if multi_label else 1)
    if rows is None:
        rows = _new(hp.N, row_stride, 7, like=head)
    counts = _new(hp.N, like=head, dtype=torch.int32)
    dropped = _new(hp.N, like=head, dtype=torch.int32)
    call("mny_yolo_decode_ex", _p(head), _p(anchors_all), _p(mask), ctypes.byref(hp), float(obj_thr), float(score_thr), int(bool(multi_label)),
         _p(class_mask), _p(rows), int(row_stride), _p(base_counts), _p(counts), _p(dropped), _st())
    return rows, counts, dropped


def nms_agnostic(rows, seg_begin, seg_count, thr=0.45, max_seg_rows=0, gather=True):
    """Class-agnostic twin of nms_per_class (one bucket per segment; out_rows carries the original rows).  Same return tuple."""
    capacity = rows.shape[0]
    S = seg_begin.numel()
    ws = torch.empty(query("mny_nms_agnostic_ws_bytes", S, capacity), device=seg_begin.device, dtype=torch.uint8)
    out_idx = torch.empty(max(capacity, 1), device=seg_begin.device, dtype=torch.int32)
    out_counts = torch.empty(S, device=seg_begin.device, dtype=torch.int32)
    out_rows = torch.empty(max(capacity, 1), 7, device=seg_begin.device) if gather else None
    call("mny_nms_agnostic", _p(rows) if capacity else None, _p(seg_begin), _p(seg_count), S, capacity, int(max_seg_rows),
         float(thr), _p(out_idx), _p(out_counts), _p(out_rows), ctypes.c_void_p(ws.data_ptr()), _st())
    so = query("mny_nms_agnostic_status_offset", S, capacity)
    po = query("mny_nms_agnostic_prefix_offset", S, capacity)
    return out_idx, out_counts, out_rows, ws[po:po + 4 * (S + 1)].view(torch.int32), ws[so:so + 4].view(torch.int32)


def det_topk(rows, seg_begin, out_idx, out_counts, out_rows, max_det, ws=None):
    """Behind nms_per_class / nms_agnostic on the same rows and segments: every segment keeps its `max_det` best entries, in place on
    out_idx / out_counts / out_rows.  -> the new prefix, int32 [S+1]"""
    S = seg_begin.numel()
    capacity = rows.shape[0]
    assert all(t.dtype == torch.int32 for t in (seg_begin, out_idx, out_counts)) and out_counts.numel() == S
    assert out_rows is None or (out_rows.dtype == torch.float32 and out_rows.shape[-1] == 7)
    nbytes = query("mny_det_topk_ws_bytes", S, capacity)
    if ws is None:
        ws = torch.empty(nbytes, device=seg_begin.device, dtype=torch.uint8)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes, "det_topk: workspace too small"
    prefix = torch.empty(S + 1, device=seg_begin.device, dtype=torch.int32)
    call("mny_det_topk", _p(rows) if capacity else None, _p(seg_begin), S, capacity, int(max_det), _p(out_idx), _p(out_counts), _p(out_rows),
         _p(prefix), ctypes.c_void_p(ws.data_ptr()), _st())
    return prefix


# ---- test-time augmentation (csrc/tta.hip) ----------------------------------------------------------
def tta_view(src, Hd, Wd, flip=False, out=None):
    """src [N,C,Hs,Ws] fp32 NCHW -> [N,C,Hd,Wd]: mirrored (flip) then resized bilinearly, half-pixel centres, fp64 arithmetic."""
    N, C, Hs, Ws = src.shape
    assert src.dtype == torch.float32, "tta_view takes the fp32 input batch"
    dst = out if out is not None else _new(N, C, int(Hd), int(Wd), like=src)
    assert tuple(dst.shape) == (N, C, int(Hd), int(Wd)) and dst.dtype == torch.float32
    call("mny_tta_view", _p(src), _p(dst), N, C, Hs, Ws, int(Hd), int(Wd), int(bool(flip)), _st())
    return dst


def det_append(src_rows, src_counts, dst_rows, counts, flip=False):
    """Append image n's first src_counts[n] rows of src_rows [N,src_stride,7] behind the counts[n] rows of dst_rows [N,dst_stride,7]
    (x un-mirrored with `flip`); counts is updated in place.  -> counts"""
    N = counts.numel()
    assert src_rows.dim() == 3 and dst_rows.dim() == 3 and src_rows.shape[2] == 7 and dst_rows.shape[2] == 7
    assert src_rows.shape[0] == N and dst_rows.shape[0] == N and src_counts.numel() == N
    assert src_rows.dtype == torch.float32 and dst_rows.dtype == torch.float32
    assert src_counts.dtype == torch.int32 and counts.dtype == torch.int32
    call("mny_det_append", _p(src_rows) if src_rows.numel() else None, src_rows.shape[1], _p(src_counts), int(bool(flip)),
         _p(dst_rows) if dst_rows.numel() else None, dst_rows.shape[1], _p(counts), N, _st())
    return counts


def nms_merge(rows, seg_begin, seg_count, out_idx, out_counts, prefix, out_rows, thr=0.45):
    """Behind nms_per_class(..., gather=True) on the same rows / segments: columns 0..3 of every kept row in out_rows become the
    score-weighted mean of the candidates of its class with IoU > thr (and itself), in place.  -> out_rows"""
    S = seg_begin.numel()
    assert out_rows is not None and out_rows.dtype == torch.float32 and out_rows.shape[-1] == 7
    assert all(t.dtype == torch.int32 for t in (seg_begin, seg_count, out_idx, out_counts, prefix)) and prefix.numel() == S + 1
    call("mny_nms_merge", _p(rows) if rows.numel() else None, _p(seg_begin), _p(seg_count), S, _p(out_idx), _p(out_counts), _p(prefix),
         float(thr), _p(out_rows), _st())
    return out_rows


# ---- sliced inference (csrc/slice.hip) ---------------------------------------------------------------
def _raw(t):
    """a uint8 device table (mny_tile_desc / mny_tile_map records) or byte buffer"""
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    return ctypes.c_void_p(t.data_ptr())


def prep_tiles(src, tiles, B, max_h, max_w, out_h, out_w, mean3, std3, out=None, ws=None):
    """src: uint8 device buffer of packed RGB HWC images; tiles: the B mny_tile_desc records as a uint8 device tensor; mean3 / std3:
    ctypes float[3].  -> (out [B,3,out_h,out_w] fp32, ws: the int32 at ws[:4] is the status word)"""
    B, out_h, out_w = int(B), int(out_h), int(out_w)
    assert tiles.numel() >= 24 * B, "prep_tiles: the tile table is shorter than B records"
    if out is None:
        out = torch.empty(B, 3, out_h, out_w, device=src.device, dtype=torch.float32)
    assert tuple(out.shape) == (B, 3, out_h, out_w) and out.dtype == torch.float32 and out.is_contiguous()
    nbytes = query("mny_prep_tiles_ws_bytes", B, int(max_h), int(max_w), out_h, out_w)
    if ws is None:
        ws = torch.empty(nbytes, device=src.device, dtype=torch.uint8)
    assert ws.dtype == torch.uint8 and ws.numel() >= nbytes, "prep_tiles: workspace too small"
    call("mny_prep_tiles", _raw(src), _raw(tiles), B, int(max_h), int(max_w), out_h, out_w, mean3, std3, _p(out), _raw(ws), _st())
    return out, ws


def det_append_tiles(src_rows, src_counts, maps, dst_rows, counts, dropped):
    """Append slot b's surviving rows of src_rows [B,src_stride,7], mapped through maps[b] (the B mny_tile_map records as a uint8 device
    tensor), behind the counts[n] rows of image n = maps[b].image in dst_rows [N,dst_stride,7]; counts and dropped [N] are updated in
    place.  -> counts"""
    B, N = src_counts.numel(), counts.numel()
    assert src_rows.dim() == 3 and dst_rows.dim() == 3 and src_rows.shape[2] == 7 and dst_rows.shape[2] == 7
    assert src_rows.shape[0] == B and dst_rows.shape[0] == N and dropped.numel() == N and maps.numel() >= 48 * B
    assert src_rows.dtype == torch.float32 and dst_rows.dtype == torch.float32
    assert src_counts.dtype == torch.int32 and counts.dtype == torch.int32 and dropped.dtype == torch.int32
    call("mny_det_append_tiles", _p(src_rows) if src_rows.numel() else None, src_rows.shape[1], _p(src_counts) if B else None,
         _raw(maps) if B else None, B, _p(dst_rows) if dst_rows.numel() else None, dst_rows.shape[1], _p(counts) if N else None,
         _p(dropped) if N else None, N, _st())
    return counts
