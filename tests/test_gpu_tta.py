"""Test-time augmentation on the MI355X: the three kernels of csrc/tta.hip against the numpy restatement (tests/tta_ref.py) bit for bit,
the single-identity-view invariant against model(x), the whole TTA call against the oracle pipeline on the same heads, and a `seg:`
config.  Every kernel comparison is exact (array_equal)."""
import json
import os

import numpy as np
import pytest
import torch

import tta_ref
from oracle import procedural

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
f32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- mny_tta_view ----------------------------------------------------------------------------------------------------
# (source shape, Hd, Wd, flip, position of the one inf or None, outputs that touch the inf through zero-weight taps only: a slice)
VIEW_CASES = {
    # rows: source coordinates 0.333, 2.0, 3.667 -> output row 1 reads row 3 with weight exactly 0
    "5x7_to_3x4": ((2, 3, 5, 7), 3, 4, False, (0, 1, 3, 2), (0, 1, 1, slice(None))),
    "5x7_to_3x4_mirrored": ((2, 3, 5, 7), 3, 4, True, (1, 2, 3, 6), (1, 2, 1, slice(None))),
    "1x1_to_4x4": ((1, 3, 1, 1), 4, 4, False, None, None),
    "64_to_32": ((2, 3, 64, 64), 32, 32, False, None, None),
    "64_to_96": ((2, 3, 64, 64), 96, 96, False, None, None),
    "64_to_96_mirrored": ((2, 3, 64, 64), 96, 96, True, None, None),
    # same size: every second tap has weight 0; the output left of the mirrored inf reads it as its x1 tap, the one above as its y1 tap
    "64_mirrored_copy": ((2, 3, 64, 64), 64, 64, True, (1, 0, 20, 30), (1, 0, slice(19, 20), slice(32, 33))),
    "33x65_to_32": ((1, 1, 33, 65), 32, 32, False, None, None),
    "33x65_to_32_mirrored": ((1, 1, 33, 65), 32, 32, True, None, None),
}


@pytest.mark.parametrize("case", list(VIEW_CASES))
def test_view_equals_restatement(case):
    from mobilenet_yolo_pytorch_amd import ops
    shape, hd, wd, flip, inf_at, clean = VIEW_CASES[case]
    src = np.random.default_rng(len(case)).uniform(-2.0, 2.0, size=shape).astype(f32)
    src.flat[0] = -abs(src.flat[0])                                                 # (a negative value also in the 1x1 sources)
    if inf_at is not None:
        src[inf_at] = np.inf
    want = tta_ref.tta_view(src, hd, wd, flip)
    got = ops.tta_view(_dev(src), hd, wd, flip).cpu().numpy()
    assert got.shape == want.shape == shape[:2] + (hd, wd)
    assert not np.isnan(want).any()
    assert np.array_equal(got, want)
    if inf_at is not None:
        assert np.isinf(want).any() and np.isfinite(want[clean]).all() and np.isfinite(got[clean]).all()
    if (hd, wd) == shape[2:]:
        assert np.array_equal(got, src[:, :, :, ::-1] if flip else src)             # an exact (mirrored) copy


def test_view_zero_weight_neighbours_of_the_mirrored_copy_stay_finite():
    """In the same-size mirrored copy the inf at column 30 lands at column 33; the outputs at columns 32 (x1 tap) and row 19 (y1 tap)
    read it with weight exactly 0 and must stay what the source holds."""
    from mobilenet_yolo_pytorch_amd import ops
    src = np.random.default_rng(3).uniform(-2.0, 2.0, size=(1, 1, 64, 64)).astype(f32)
    src[0, 0, 20, 30] = np.inf
    got = ops.tta_view(_dev(src), 64, 64, True).cpu().numpy()
    assert np.isinf(got[0, 0, 20, 33]) and np.isinf(got).sum() == 1 and not np.isnan(got).any()
    assert np.array_equal(got, src[:, :, :, ::-1])


# ---- mny_det_append ----------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def _append_case(dst_stride, base):
    rng = np.random.default_rng(11)
    N, stride = 3, 5
    srcs = [rng.uniform(0.0, 1.0, size=(N, stride, 7)).astype(f32) for _ in range(2)]
    src_counts = [np.array([0, 1, stride], dtype=np.int32), np.array([stride, 0, 1], dtype=np.int32)]
    dst = np.full((N + 1, dst_stride, 7), SENTINEL, dtype=f32)                     # one more block behind the last image: a guard
    return srcs, src_counts, dst, np.array(base, dtype=np.int32)


@pytest.mark.parametrize("dst_stride,base", [(12, [2, 0, 3]), (4, [0, 0, 0]), (7, [2, 7, 3])], ids=["roomy", "one_row_short", "full_image"])
def test_append_equals_restatement(dst_stride, base):
    """source counts {0, 1, full stride}, non-zero base counts, two successive appends (plain, then mirrored).  `one_row_short`: the
    full-stride image is clamped to dst_stride = 4 rows; `full_image`: an image whose segment is full already takes nothing.  Everything
    outside the written ranges, the block behind the last image included, keeps the sentinel."""
    from mobilenet_yolo_pytorch_amd import ops
    srcs, src_counts, dst, counts = _append_case(dst_stride, base)
    d_dst, d_counts = _dev(dst), _dev(counts)
    for k, flip in enumerate((False, True)):
        tta_ref.det_append(srcs[k], src_counts[k], flip, dst[:3], counts)
        ops.det_append(_dev(srcs[k]), _dev(src_counts[k]), d_dst[:3], d_counts, flip=flip)
        assert np.array_equal(d_counts.cpu().numpy(), counts), (k, d_counts.tolist(), counts.tolist())
        assert np.array_equal(d_dst.cpu().numpy(), dst), k
    assert counts.max() <= dst_stride and (dst[3] == SENTINEL).all()
    written = sum(int(c) for c in counts) - sum(base)
    assert int((dst[:3, :, 0] != SENTINEL).sum()) == written > 0
    if dst_stride == 4:
        assert counts.tolist() == [4, 1, 4]                                         # image 2: 5 offered, 4 fit; then 1 offered, 0 fit
    if dst_stride == 12:                                                            # the mirrored rows: one fp32 subtraction each
        r, w = srcs[1][0, 0], dst[0, 2]
        assert np.array_equal(w, np.array([f32(1) - r[2], r[1], f32(1) - r[0], r[3], r[4], r[5], r[6]], dtype=f32))


# ---- mny_nms_merge -----------------------------------------------------------------------------------------------------
THR = 0.5                                      # the threshold-edge pair has IoU 0.5 exactly
NUM_CLASSES = 5
SEG_CAP = 512


def _clusters(rng, n, cls):
    """n boxes of class `cls` scattered round 6 centres (the same centres for every class: classes overlap each other)"""
    centres = np.array([[0.05, 0.05], [0.55, 0.05], [0.05, 0.55], [0.55, 0.55], [0.3, 0.3], [0.6, 0.3]], dtype=f32)
    k = rng.integers(0, len(centres), size=n)
    xy = centres[k] + rng.uniform(-0.02, 0.02, size=(n, 2)).astype(f32)
    wh = f32(0.3) + rng.uniform(-0.02, 0.02, size=(n, 2)).astype(f32)
    rows = np.zeros((n, 7), dtype=f32)
    rows[:, 0:2], rows[:, 2:4] = xy, xy + wh
    rows[:, 4] = rng.uniform(0.1, 1.0, size=n).astype(f32)
    rows[:, 5] = rng.uniform(0.1, 1.0, size=n).astype(f32)
    rows[:, 6] = cls
    return rows


def _segment(kind, rng):
    if kind == "empty":
        return np.zeros((0, 7), dtype=f32)
    if kind == "big":                          # buckets of 300, 65 and 1 rows
        parts = [_clusters(rng, 300, 0), _clusters(rng, 65, 1), _clusters(rng, 1, 2)]
    elif kind == "grid":                       # a bucket of 300 rows that keeps 280: more kept boxes than one workgroup has lanes
        cell = np.stack(np.meshgrid(np.arange(20), np.arange(14)), -1).reshape(-1, 2).astype(f32) * f32(0.05)
        xy = np.concatenate([cell, cell[::14]]) + rng.uniform(-0.002, 0.002, size=(300, 2)).astype(f32)
        g = _clusters(rng, 300, 0)
        g[:, 0:2], g[:, 2:4] = xy, xy + f32(0.04)
        parts = [g, _clusters(rng, 65, 1)]
    else:                                      # buckets of 63 and 64 rows, and the special rows of the CPU test
        edge = np.array([[0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 2], [0.0, 0.0, 1.0, 0.5, 0.5, 1.0, 2],      # IoU exactly THR: not merged
                         [0.3, 0.3, 0.3, 0.3, 0.9, 0.5, 2]], dtype=f32)                              # zero area: NaN with itself, keeps itself
        zero_w = np.array([[0.0, 0.0, 0.5, 0.5, 0.0, 1.0, 3], [0.0625, 0.0, 0.5625, 0.5, 0.5, 0.0, 3],
                           [0.0, 0.0625, 0.5, 0.5625, 0.0, 0.0, 3]], dtype=f32)                      # a whole cluster of weight 0
        parts = [_clusters(rng, 63, 0), _clusters(rng, 64, 1), edge, zero_w]
    rows = np.concatenate(parts)
    return rows[rng.permutation(len(rows))]                                         # classes interleaved in the segment


@pytest.mark.parametrize("kinds", [("big",), ("special", "empty"), ("grid", "empty", "special")], ids=["one", "two_one_empty", "three_one_empty"])
def test_merge_equals_restatement(kinds):
    from mobilenet_yolo_pytorch_amd import ops
    rng = np.random.default_rng(17)
    segs = [_segment(k, rng) for k in kinds]
    S = len(segs)
    rows = np.full((S * SEG_CAP, 7), SENTINEL, dtype=f32)
    for s, r in enumerate(segs):
        rows[s * SEG_CAP:s * SEG_CAP + len(r)] = r
    begin = np.arange(S, dtype=np.int32) * SEG_CAP
    count = np.array([len(r) for r in segs], dtype=np.int32)
    d_rows, d_begin, d_count = _dev(rows), _dev(begin), _dev(count)
    out_idx, out_counts, out_rows, prefix, status = ops.nms_per_class(d_rows, d_begin, d_count, NUM_CLASSES, thr=THR, max_seg_rows=SEG_CAP)
    out_rows.view(-1)[int(prefix[-1].item()) * 7:] = SENTINEL                        # (the tail behind the kept rows is uninitialised)
    before = out_rows.cpu().numpy().copy()
    ops.nms_merge(d_rows, d_begin, d_count, out_idx, out_counts, prefix, out_rows, thr=THR)
    after = out_rows.cpu().numpy()
    assert int(status.item()) == 0
    pre, kept_n, idx = prefix.cpu().numpy(), out_counts.cpu().numpy(), out_idx.cpu().numpy()
    assert np.array_equal(np.diff(pre), kept_n)
    assert np.array_equal(after[:, 4:], before[:, 4:])                              # confidence, class score and class: untouched
    assert np.array_equal(after[pre[-1]:], before[pre[-1]:])                        # nothing behind the kept rows is written
    most, moved = 0, 0
    for s, r in enumerate(segs):
        kept = idx[begin[s]:begin[s] + kept_n[s]] - begin[s]
        assert np.array_equal(before[pre[s]:pre[s + 1]], r[kept])                   # row order: the NMS's
        want = tta_ref.nms_merge(r, kept, THR)
        assert np.array_equal(after[pre[s]:pre[s + 1]], want), (s, kinds[s])
        members = [tta_ref.merge_members(r, int(i), THR) for i in kept]
        assert all(len({float(r[j, 6]) for j in m}) == 1 for m in members)          # classes never mix
        most = max([most] + [len(m) for m in members])
        moved += int((want[:, :4] != r[kept][:, :4]).any(axis=1).sum())
        if kinds[s] == "empty":
            assert kept_n[s] == 0
        if kinds[s] == "grid":
            assert kept_n[s] > 256
        if kinds[s] == "special":
            cls = r[kept][:, 6]
            assert (cls == 2).sum() == 3 and (cls == 3).sum() == 1                   # edge pair + zero-area box all kept; one of the zero-weight cluster
            for c in (2, 3):
                assert np.array_equal(want[cls == c], r[kept][cls == c])            # ... and none of them moves
            zi = int(kept[cls == 3][0])
            assert len(tta_ref.merge_members(r, zi, THR)) == 3                      # (the zero-weight cluster IS a cluster: the fallback is what keeps it)
    assert most >= 3 and moved > 0, "no cluster was merged: the case is vacuous"


def test_merge_no_segments_and_no_rows():
    from mobilenet_yolo_pytorch_amd import _lib, ops
    _lib.call("mny_nms_merge", None, None, None, 0, None, None, None, 0.5, None, None)              # S == 0: nothing to do
    rows = torch.zeros(4, 7, device="cuda")
    begin, count = _dev(np.array([0, 2], dtype=np.int32)), _dev(np.array([0, 0], dtype=np.int32))
    out_idx, out_counts, out_rows, prefix, _ = ops.nms_per_class(rows, begin, count, 3)
    out_rows.fill_(SENTINEL)
    ops.nms_merge(rows, begin, count, out_idx, out_counts, prefix, out_rows)
    assert out_counts.tolist() == [0, 0] and bool((out_rows == SENTINEL).all())
    _lib.call("mny_det_append", None, 0, None, 0, None, 0, None, 0, None)                          # N == 0


# ---- the TTA call ------------------------------------------------------------------------------------------------------
def _model(val_conf):
    from mobilenet_yolo_pytorch_amd import yolo
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG, sync_metrics=True)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = val_conf
    return m


def test_single_identity_view_equals_model():
    from mobilenet_yolo_pytorch_amd.tta import TTA
    m = _model(0.3)
    x = procedural.images(2, 96, 96, seed=10).cuda()
    want = [d.cpu().numpy() for d in m(x)]
    got = TTA(m, views=[(96, False)], merge=False)(x)
    assert isinstance(got, list) and len(got) == 2 and all(d.is_cuda and d.shape[1] == 7 for d in got)
    assert sum(len(d) for d in want) > 0
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.cpu().numpy(), b)
    again = m(x)                                                                    # and model(x) is what it was
    for a, b in zip(again, want):
        assert np.array_equal(a.cpu().numpy(), b)


VAL_CONF = 0.3


@pytest.mark.parametrize("nms_thr,min_members", [(0.3, 3), (0.45, 2)], ids=["thr0.30_three_members", "thr0.45_default"])
def test_tta_equals_oracle_pipeline_on_same_heads(nms_thr, min_members):
    """Views (96, plain) and (64, mirrored), merge on.  Each view's GPU heads decoded by the oracle, un-mirrored, concatenated per image
    in view order, the oracle's per-class NMS, then the restated merge; counts exact, rows to the tolerance of
    test_eval_detections_equal_oracle_pipeline_on_same_heads (same heads on both sides; the oracle's decode rounds differently).
    The case must not be vacuous: every image's joint segment holds >= 50 candidates and some kept box has >= 3 members (both asserted).
    Procedural weights scatter classes and box sizes, so at the default nms_thr = 0.45 no val_conf reaches three members with these two
    views (measured: 2 at most, also with all 195 candidates of an image, for image seeds 10..13); at nms_thr = 0.3 and val_conf = 0.3
    this batch has 74 / 78 candidates and one three-member cluster per image.  The threshold is an argument like any other.  The second
    case runs the same comparison at the default 0.45, where the largest cluster has two members (asserted)."""
    from mobilenet_yolo_pytorch_amd.tta import TTA
    from oracle import nms_ref, yolo_ref
    m = _model(VAL_CONF)
    x = procedural.images(2, 96, 96, seed=10).cuda()
    tta = TTA(m, views=[(96, False), (64, True)], merge=True, nms_thr=nms_thr)
    det = tta(x)
    bufs = next(iter(tta._bufs.values()))
    assert np.array_equal(bufs["x"][1].cpu().numpy(), tta_ref.tta_view(x.cpu().numpy(), 64, 64, True))    # what the second plan was fed
    joint_counts = bufs["counts"].tolist()
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    per_image = [[] for _ in range(2)]
    near = 0
    for size, flip in tta.views:
        plan = m._plans[(2, size, size, False)]
        for hi in range(2):
            heads = plan.heads[hi].cpu()
            specs[hi].val_conf = VAL_CONF
            for n, r in enumerate(yolo_ref.decode_rows(heads, specs[hi], [size, size], layout="nhwc")):
                r = r.numpy().astype(f32).copy()
                if flip:
                    x1, x2 = r[:, 0].copy(), r[:, 2].copy()
                    r[:, 0], r[:, 2] = f32(1.0) - x2, f32(1.0) - x1
                per_image[n].append(r)
            specs[hi].val_conf = VAL_CONF - 1e-5
            near += sum(int((r[:, 4] <= VAL_CONF + 1e-5).sum()) for r in yolo_ref.decode_rows(heads, specs[hi], [size, size], layout="nhwc"))
    assert near == 0, "the seeded batch has a candidate within 1e-5 of val_conf: pick another seed"
    most, moved = 0, 0
    for n in range(2):
        rows = np.concatenate(per_image[n])
        assert len(rows) == joint_counts[n] and len(rows) >= 50, (len(rows), joint_counts[n])
        _, idx = nms_ref.nms_rows(torch.from_numpy(rows), 20, thr=nms_thr)
        idx = idx.numpy()
        want = tta_ref.nms_merge(rows, idx, nms_thr)
        most = max([most] + [len(tta_ref.merge_members(rows, int(i), nms_thr)) for i in idx])
        moved += int((want[:, :4] != rows[idx][:, :4]).any(axis=1).sum())
        assert len(det[n]) == len(want), (n, len(det[n]), len(want))
        np.testing.assert_allclose(det[n].cpu().numpy(), want, rtol=1e-5, atol=1e-4)
    assert most >= min_members and moved > 0, "no kept box has %d members: the merge is not exercised" % min_members


def _bdd():
    from mobilenet_yolo_pytorch_amd import yolo
    man = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))
    torch.manual_seed(0)
    m = yolo(man["config"], sync_metrics=True)
    procedural.fill_state_dict_(m)
    return man["config"]["seg"]["num_classes"], m.cuda().eval()


@pytest.mark.parametrize("views", [[(64, False), (32, True)], [(64, False), (64, True)]], ids=["smaller_mirrored", "same_size_mirrored"])
def test_tta_on_a_seg_config_returns_the_identity_views_seg(views):
    """`same_size_mirrored`: the mirrored view runs on the identity view's own plan (plans are cached per size) and overwrites its seg
    buffers; the seg map and the logits must still be the identity view's."""
    from mobilenet_yolo_pytorch_amd import MnyError
    from mobilenet_yolo_pytorch_amd.tta import TTA
    C, m = _bdd()
    x = procedural.images(2, 64, 64, seed=22).cuda()
    _, seg_mirrored = m(torch.flip(x, dims=[3]).contiguous())
    z_mirrored = m.seg_logits()
    _, seg_plain = m(x)
    z_plain = m.seg_logits()
    assert not np.array_equal(seg_plain, seg_mirrored) and not torch.equal(z_plain, z_mirrored)       # (the mirror is visible in the seg head)
    tta = TTA(m, views=views)
    with pytest.raises(MnyError, match="no TTA call"):
        tta.seg_logits()
    det, seg = tta(x)
    assert isinstance(det, list) and len(det) == 2 and all(d.shape[1] == 7 and d.is_cuda for d in det)
    assert isinstance(seg, np.ndarray) and seg.shape == (C, 4, 4) and np.array_equal(seg, seg_plain)
    z = tta.seg_logits()
    assert z.shape == (2, 4, 4, C) and z.dtype == torch.float32 and torch.equal(z, z_plain)
    with pytest.raises(MnyError, match="no eval forward"):                          # the views overwrote the plans: the model's own is withdrawn
        m.seg_logits()
    _, seg_again = m(x)                                                             # ... and model(x) is what it was
    assert np.array_equal(seg_again, seg_plain) and torch.equal(m.seg_logits(), z_plain) and torch.equal(tta.seg_logits(), z_plain)
