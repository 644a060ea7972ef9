"""Post-processing options on the MI355X: mny_yolo_decode_ex bit for bit against the device's own mny_yolo_decode where the two must
agree and against the numpy restatement (tests/post_ref.py) elsewhere, the capacity rule, the class-agnostic NMS against
mny_nms_per_class on class-zeroed rows, mny_det_topk against the restatement, and the Detector / TTA calls on a small model."""
import json
import os

import numpy as np
import pytest
import torch

import post_ref
import tta_ref
from oracle import procedural

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
f32 = np.float32
SENTINEL = -7.0

ANCHORS = np.array([[0.1, 0.2], [0.3, 0.25], [0.6, 0.5]], dtype=f32)
# the 256-cell chunk loop ends before (1, 128 cells), on (256) and after (289, 363) a boundary and runs a second trip
GRIDS = [(1, 1), (2, 8), (1, 16), (1, 17), (3, 11)]
CLASSES = [1, 2, 20, 33, 80]
OBJ_THR, SCORE_THR = 0.4, 0.25
# seed per (A, g, C, N), chosen on the CPU so that no conf and no conf * cls of the case lies within 1e-5 of OBJ_THR / SCORE_THR in
# the restatement (asserted in test_decode_equals_restatement): the first seed >= 0 that keeps 2e-5 away; 0 where not listed
SEEDS = {(2, 8, 33, 1): 1, (2, 8, 33, 3): 1, (1, 16, 20, 3): 1, (1, 16, 33, 1): 1, (1, 16, 33, 3): 1, (1, 16, 80, 3): 1, (1, 17, 20, 3): 1,
         (1, 17, 33, 1): 1, (1, 17, 33, 3): 1, (1, 17, 80, 3): 1, (3, 11, 20, 3): 1, (3, 11, 33, 1): 1, (3, 11, 33, 3): 1, (3, 11, 80, 3): 1}
CASES = [(A, g, C, N) for A, g in GRIDS for C in CLASSES for N in (1, 3)]


def _id(case):
    return "A%d_g%d_C%d_N%d" % case


def make_head(A, g, C, N, seed):
    """random NHWC head: objectness and class logits wide (both ends of the sigmoid, few values near a threshold), box logits narrow
    (sizes of a few units at most: the 1e-4 tolerance is absolute)"""
    rng = np.random.default_rng(seed)
    h = rng.normal(0.0, 4.0, size=(N, g, g, A, 5 + C))
    h[..., 0:2] = rng.normal(0.0, 1.0, size=(N, g, g, A, 2))
    h[..., 2:4] = rng.normal(0.0, 0.5, size=(N, g, g, A, 2))
    return h.reshape(N, g, g, A * (5 + C)).astype(f32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _args(ops, A, g, C, N):
    return _dev(ANCHORS), _dev(np.arange(A, dtype=np.int32)), ops.make_head(N, g, A, C, len(ANCHORS), 0.5, 0.2, 0.01)


def _subset(C):
    """a class filter that crosses the word boundary where C does"""
    return sorted({0, C // 2, C - 1, min(C - 1, 31), min(C - 1, 32)})


# ---- decode, bitwise against mny_yolo_decode -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_compat_settings_equal_yolo_decode_bitwise(case):
    """multi_label = 0, no score test, no mask, row_stride >= cells: rows and counts are mny_yolo_decode's, also for a second head
    appended through base_counts inside a wider row_stride (both buffers start from the same sentinel fill and end up equal)"""
    from mobilenet_yolo_pytorch_amd import ops
    A, g, C, N = case
    head = _dev(make_head(A, g, C, N, seed=1))
    anchors, mask, hp = _args(ops, A, g, C, N)
    cells = A * g * g
    want_rows, want_counts = ops.yolo_decode(head, anchors, mask, hp, 0.3)
    rows, counts, dropped = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3)
    assert torch.equal(counts, want_counts) and dropped.tolist() == [0] * N
    assert int(counts.sum()) > 0 or cells == 1
    for n in range(N):
        assert torch.equal(rows[n, :counts[n]], want_rows[n, :counts[n]])
    stride = 2 * cells + 3
    a = torch.full((N, stride, 7), SENTINEL, device="cuda")
    b = a.clone()
    _, c1 = ops.yolo_decode(head, anchors, mask, hp, 0.3, rows=a, row_stride=stride)
    _, c2 = ops.yolo_decode(head, anchors, mask, hp, 0.6, rows=a, row_stride=stride, base_counts=c1)
    _, d1, x1 = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, rows=b, row_stride=stride)
    _, d2, x2 = ops.yolo_decode_ex(head, anchors, mask, hp, 0.6, rows=b, row_stride=stride, base_counts=d1)
    assert torch.equal(c1, d1) and torch.equal(c2, d2) and torch.equal(a, b) and x1.tolist() == x2.tolist() == [0] * N


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_multi_label_rows_of_the_best_class_equal_yolo_decode_bitwise(case):
    """score test off, no mask: every cell above obj_thr emits its C classes in order, and the row of the cell's best class is the row
    mny_yolo_decode emits, in all seven columns"""
    from mobilenet_yolo_pytorch_amd import ops
    A, g, C, N = case
    head = _dev(make_head(A, g, C, N, seed=2))
    anchors, mask, hp = _args(ops, A, g, C, N)
    single, sc = ops.yolo_decode(head, anchors, mask, hp, 0.3)
    rows, counts, dropped = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, multi_label=True)
    assert rows.shape[1] == A * g * g * C and dropped.tolist() == [0] * N
    assert torch.equal(counts, sc * C)
    for n in range(N):
        k = int(sc[n])
        per_cell = rows[n, :k * C].view(k, C, 7)
        assert torch.equal(per_cell[:, :, 6], torch.arange(C, device="cuda", dtype=torch.float32).expand(k, C))
        best = single[n, :k, 6].long()
        assert torch.equal(per_cell[torch.arange(k, device="cuda"), best], single[n, :k])


# ---- decode against the restatement ---------------------------------------------------------------------------------------
MODES = {"single": (False, -1.0, False), "single_score_mask": (False, SCORE_THR, True), "multi_score": (True, SCORE_THR, False),
         "multi_score_mask": (True, SCORE_THR, True), "multi_mask": (True, -1.0, True)}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_decode_equals_restatement(case):
    """counts, class column and row order exact; columns 0..5 at the project's decode tolerance (rtol=0, atol=1e-4).  Device expf and
    numpy exp may differ in the last bits, so the case's seed keeps every conf and every score 1e-5 away from its threshold: asserted
    here on the restatement alone, no row and no case is left out."""
    from mobilenet_yolo_pytorch_amd import ops
    A, g, C, N = case
    head = make_head(A, g, C, N, seed=SEEDS.get(case, 0))
    m_obj, m_score = post_ref.margins(head, ANCHORS, list(range(A)), OBJ_THR, SCORE_THR)
    assert m_obj > 1e-5 and m_score > 1e-5, "seed %d: a conf / score within 1e-5 of its threshold (%g, %g)" % (SEEDS.get(case, 0), m_obj, m_score)
    anchors, mask, hp = _args(ops, A, g, C, N)
    d_head = _dev(head)
    emitted = 0
    for name, (multi, score_thr, masked) in MODES.items():
        words = post_ref.class_mask_words(_subset(C), C) if masked else None
        want = post_ref.decode_candidates(head, ANCHORS, list(range(A)), OBJ_THR, score_thr, multi, words)
        cmask = ops.class_mask(_subset(C), C, "cuda") if masked else None
        if masked:
            assert np.array_equal(cmask.cpu().numpy().view(np.uint32), words)
        rows, counts, dropped = ops.yolo_decode_ex(d_head, anchors, mask, hp, OBJ_THR, score_thr, multi, cmask)
        assert counts.tolist() == [len(w) for w in want] and dropped.tolist() == [0] * N, name
        for n in range(N):
            got = rows[n, :len(want[n])].cpu().numpy()
            assert np.array_equal(got[:, 6], want[n][:, 6]), name
            np.testing.assert_allclose(got[:, :6], want[n][:, :6], rtol=0, atol=1e-4, err_msg=name)
        emitted += sum(len(w) for w in want)
    assert emitted > 0 or A * g * g == 1


@pytest.mark.parametrize("A,g", GRIDS)
def test_exact_heads_equal_restatement_bitwise(A, g):
    """logits from {-inf, 0, +inf} with tw = th = 0: every sigmoid is 0, 0.5 or 1 and every score 0, 0.25, 0.5 or 1 on both sides, the
    thresholds sit on those values; every column compared bit for bit"""
    from mobilenet_yolo_pytorch_amd import ops
    C, N = 3, 3
    rng = np.random.default_rng(A * 100 + g)
    head = rng.choice(np.array([-np.inf, 0.0, np.inf], dtype=f32), size=(N, g, g, A, 5 + C))
    head[..., 2:4] = 0.0
    head = head.reshape(N, g, g, A * (5 + C))
    anchors, mask, hp = _args(ops, A, g, C, N)
    cmask, words = ops.class_mask([0, 2], C, "cuda"), post_ref.class_mask_words([0, 2], C)
    seen = set()
    for obj_thr in (0.0, 0.5):
        for score_thr in (-1.0, 0.0, 0.25, 0.5):
            for multi in (False, True):
                for masked in (False, True):
                    want = post_ref.decode_candidates(head, ANCHORS, list(range(A)), obj_thr, score_thr, multi, words if masked else None)
                    rows, counts, dropped = ops.yolo_decode_ex(_dev(head), anchors, mask, hp, obj_thr, score_thr, multi, cmask if masked else None)
                    assert counts.tolist() == [len(w) for w in want] and dropped.tolist() == [0] * N
                    for n in range(N):
                        assert np.array_equal(rows[n, :len(want[n])].cpu().numpy(), want[n]), (obj_thr, score_thr, multi, masked, n)
                        seen |= set((want[n][:, 4] * want[n][:, 5]).tolist())
    if A * g * g > 1:
        assert seen == {0.0, 0.25, 0.5, 1.0}


# ---- capacity -------------------------------------------------------------------------------------------------------------
def test_capacity_counts_dropped_prefix_and_nothing_past_the_segment():
    from mobilenet_yolo_pytorch_amd import ops
    A, g, C, N = 3, 11, 20, 3
    head = _dev(make_head(A, g, C, N, seed=3))
    anchors, mask, hp = _args(ops, A, g, C, N)
    full, total, _ = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, 0.1, True)
    T = total.tolist()
    assert min(T) > 300 and len(set(T)) == 3
    for stride in (1, max(T), max(T) - 1, min(T), min(T) - 1):
        buf = torch.full((N + 1, stride, 7), SENTINEL, device="cuda")               # one more block behind the last image: a guard
        _, counts, dropped = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, 0.1, True, rows=buf[:N], row_stride=stride)
        assert counts.tolist() == [min(t, stride) for t in T] and dropped.tolist() == [t - min(t, stride) for t in T]
        for n in range(N):
            assert torch.equal(buf[n, :counts[n]], full[n, :counts[n]])             # the written prefix is the unclamped result's
            assert bool((buf[n, counts[n]:] == SENTINEL).all())
        assert bool((buf[N] == SENTINEL).all())
    # a second head behind the first: image 0 has no room left, image 1 room for 5 rows, image 2 a base outside 0..row_stride
    stride = T[1] + 5
    buf = torch.full((N + 1, stride, 7), SENTINEL, device="cuda")
    base = _dev(np.array([stride, T[1], stride + 1], dtype=np.int32))
    _, counts, dropped = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, 0.1, True, rows=buf[:N], row_stride=stride, base_counts=base)
    assert counts.tolist() == [stride, stride, stride + 1] and dropped.tolist() == [T[0], T[1] - 5, T[2]]
    assert torch.equal(buf[1, T[1]:], full[1, :5])
    buf[1, T[1]:] = SENTINEL
    assert bool((buf == SENTINEL).all())
    neg = _dev(np.array([-1, 0, 0], dtype=np.int32))
    _, counts, dropped = ops.yolo_decode_ex(head, anchors, mask, hp, 0.3, 0.1, True, rows=buf[:N], row_stride=stride, base_counts=neg)
    assert counts[0].item() == -1 and dropped[0].item() == T[0] and bool((buf[0] == SENTINEL).all())


# ---- class-agnostic NMS ---------------------------------------------------------------------------------------------------
def dense_rows(n, C, seed):
    """boxes on a coarse lattice (dense overlaps, exact IoU ties) and quantised scores (ties)"""
    r = np.random.RandomState(seed)
    xy = np.round(r.rand(n, 2) * 16) / 16
    wh = 0.125 + np.round(r.rand(n, 2) * 4) / 16
    conf = np.round(r.rand(n, 1), 1) + 0.05
    return np.concatenate((xy - wh / 2, xy + wh / 2, conf, np.ones((n, 1)), r.randint(0, C, size=(n, 1))), 1).astype(f32)


def sparse_rows(n, C, seed):
    """small boxes, most of them kept; quantised scores: ties across classes"""
    r = np.random.RandomState(seed)
    xy = r.rand(n, 2)
    wh = 0.02 + 0.03 * r.rand(n, 2)
    conf = np.round(r.rand(n, 1), 1) + 0.05
    return np.concatenate((xy - wh / 2, xy + wh / 2, conf, np.ones((n, 1)), r.randint(0, C, size=(n, 1))), 1).astype(f32)


def _segments(sizes, C, gen, seed=0):
    segs = [gen(n, C, seed + 10 * i) for i, n in enumerate(sizes)]
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    rows = np.concatenate(segs) if sum(sizes) else np.zeros((0, 7), dtype=f32)
    d_rows = _dev(rows) if len(rows) else torch.zeros(1, 7, device="cuda")[:0]
    return segs, off, rows, d_rows, _dev(off[:-1].copy()), _dev(np.array(sizes, dtype=np.int32))


# all eight sizes in one call (small segments on average: the one-workgroup path, 8193 through the global-scratch kernel); 2049 and
# 8193 alone (a call that averages more than 2048 rows per segment: the bit-matrix path, 8193 past its LDS image)
@pytest.mark.parametrize("sizes", [[0, 1, 63, 64, 65, 300, 2049, 8193], [2049], [8193]], ids=["all_sizes", "2049_alone", "8193_alone"])
def test_agnostic_nms_equals_per_class_on_class_zeroed_rows(sizes):
    from mobilenet_yolo_pytorch_amd import ops
    C = 7
    segs, off, rows, d_rows, beg, cnt = _segments(sizes, C, dense_rows)
    zeroed = d_rows.clone()
    zeroed[:, 6] = 0
    w_idx, w_counts, _, w_prefix, w_status = ops.nms_per_class(zeroed, beg, cnt, 1, 0.45, max_seg_rows=max(sizes))
    idx, counts, out_rows, prefix, status = ops.nms_agnostic(d_rows, beg, cnt, 0.45, max_seg_rows=max(sizes))
    assert int(status.item()) == 0 and int(w_status.item()) == 0
    assert torch.equal(counts, w_counts) and torch.equal(prefix, w_prefix)
    pre = prefix.tolist()
    for s, n in enumerate(sizes):
        k = int(counts[s])
        assert (k > 0) == (n > 0)
        got = idx[off[s]:off[s] + k]
        assert torch.equal(got, w_idx[off[s]:off[s] + k])
        assert torch.equal(out_rows[pre[s]:pre[s + 1]], d_rows[got.long()])            # the ORIGINAL rows, class included
    # the flag does something: the class-aware NMS keeps more of the same rows
    _, c_counts, _, _, _ = ops.nms_per_class(d_rows, beg, cnt, C, 0.45, max_seg_rows=max(sizes))
    assert int(c_counts.sum()) > int(counts.sum())
    if len(sizes) > 1:
        s = 5                                                                          # and the restatement agrees (300 rows)
        assert np.array_equal(idx[off[s]:off[s] + int(counts[s])].cpu().numpy() - off[s], post_ref.nms_agnostic(segs[s], 0.45))


# ---- top-k ---------------------------------------------------------------------------------------------------------------
def _grid_rows(n, C, seed):
    """n disjoint boxes (cells of a 65 x 65 grid): every NMS keeps them all; quantised scores"""
    r = np.random.RandomState(seed)
    cell = r.permutation(65 * 65)[:n]
    xy = np.stack((cell % 65, cell // 65), 1) / 70.0
    conf = np.round(r.rand(n, 1), 1) + 0.05
    return np.concatenate((xy, xy + 1.0 / 80, conf, np.ones((n, 1)), r.randint(0, C, size=(n, 1))), 1).astype(f32)


TOPK_CASES = {"S1": ([700], sparse_rows), "S5_two_empty": ([300, 0, 700, 0, 65], sparse_rows), "S1_dense": ([300], dense_rows),
              # the kept count below, on and above the 4096 entries the sort holds in LDS
              "kept_4095": ([4095], _grid_rows), "kept_4096": ([4096], _grid_rows), "kept_4097_and_more": ([0, 4097, 40], _grid_rows)}


@pytest.mark.parametrize("agnostic", [False, True], ids=["per_class", "agnostic"])
@pytest.mark.parametrize("max_det", [1, 100, 300])
@pytest.mark.parametrize("case", list(TOPK_CASES))
def test_topk_equals_restatement_and_merge_follows(case, max_det, agnostic):
    from mobilenet_yolo_pytorch_amd import ops
    sizes, gen = TOPK_CASES[case]
    C, thr = 5, 0.45
    segs, off, rows, d_rows, beg, cnt = _segments(sizes, C, gen, seed=3)
    nms = (lambda: ops.nms_agnostic(d_rows, beg, cnt, thr, max_seg_rows=max(sizes))) if agnostic else \
          (lambda: ops.nms_per_class(d_rows, beg, cnt, C, thr, max_seg_rows=max(sizes)))
    idx, counts, out_rows, _, status = nms()
    assert int(status.item()) == 0
    before_idx, before_counts = idx.cpu().numpy().copy(), counts.tolist()
    if case.startswith("kept_"):
        assert before_counts == sizes
    out_rows.view(-1)[sum(before_counts) * 7:] = SENTINEL
    prefix = ops.det_topk(d_rows, beg, idx, counts, out_rows, max_det)
    want = [post_ref.det_topk(rows, before_idx[off[s]:off[s] + before_counts[s]], max_det) for s in range(len(sizes))]
    assert counts.tolist() == [len(w) for w in want] == [min(k, max_det) for k in before_counts]
    assert prefix.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
    got_idx, got_rows = idx.cpu().numpy(), out_rows.cpu().numpy()
    pre = prefix.tolist()
    for s in range(len(sizes)):
        assert np.array_equal(got_idx[off[s]:off[s] + len(want[s])], want[s]), s
        assert np.array_equal(got_idx[off[s] + len(want[s]):off[s] + before_counts[s]],
                              before_idx[off[s] + len(want[s]):off[s] + before_counts[s]])      # entries behind the cap are left alone
        assert np.array_equal(got_rows[pre[s]:pre[s + 1]], rows[want[s]]), s
    assert (got_rows[sum(before_counts):] == SENTINEL).all()                          # nothing behind the NMS's own rows is written
    # the merge works on the reduced lists without change
    ops.nms_merge(d_rows, beg, cnt, idx, counts, prefix, out_rows, thr=thr)
    merged = out_rows.cpu().numpy()
    for s in range(len(sizes)):
        assert np.array_equal(merged[pre[s]:pre[s + 1]], tta_ref.nms_merge(segs[s], want[s] - off[s], thr)), s


def test_topk_ties_across_classes_and_segments_that_only_reorder():
    """quantised scores: the cap cuts through a run of equal scores of several classes, and the position in the NMS output decides"""
    from mobilenet_yolo_pytorch_amd import ops
    sizes = [700, 0, 65]
    segs, off, rows, d_rows, beg, cnt = _segments(sizes, 5, sparse_rows, seed=3)
    idx, counts, out_rows, _, _ = ops.nms_per_class(d_rows, beg, cnt, 5, 0.45, max_seg_rows=700)
    before_idx, before_counts = idx.cpu().numpy().copy(), counts.tolist()
    ops.det_topk(d_rows, beg, idx, counts, out_rows, 100)
    kept = idx[:100].cpu().numpy()
    score = rows[kept, 4] * rows[kept, 5]
    cut = score[-1]
    first = before_idx[:before_counts[0]]
    tied = first[(rows[first, 4] * rows[first, 5]) == cut]
    assert len(set(rows[tied, 6].tolist())) > 1 and len(tied) > int((score == cut).sum()) > 0     # the cap splits a tie of several classes
    assert np.array_equal(kept[score == cut], tied[:int((score == cut).sum())])                   # ... and the earlier positions win
    assert counts.tolist() == [100, 0, before_counts[2]] and before_counts[2] <= 100
    assert sorted(idx[off[2]:off[2] + before_counts[2]].tolist()) == sorted(before_idx[off[2]:off[2] + before_counts[2]].tolist())


def test_topk_no_segments():
    from mobilenet_yolo_pytorch_amd import ops
    empty = torch.zeros(0, device="cuda", dtype=torch.int32)
    prefix = ops.det_topk(torch.zeros(4, 7, device="cuda"), empty, torch.zeros(4, device="cuda", dtype=torch.int32), empty, None, 5)
    assert prefix.tolist() == [0]


# ---- the whole call ---------------------------------------------------------------------------------------------------------
def _model(val_conf):
    from mobilenet_yolo_pytorch_amd import yolo
    torch.manual_seed(0)
    m = yolo(procedural.VOC_CONFIG, sync_metrics=True)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    for hs in m.yolo_losses:
        hs.val_conf = val_conf
    return m


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.is_cuda and a.shape == b.shape and torch.equal(a, b)


def test_detector_with_default_options_equals_model_bitwise():
    from mobilenet_yolo_pytorch_amd import Detector, MnyError, PostProcess
    m = _model(0.3)
    x = procedural.images(2, 96, 96, seed=10).cuda()
    want = m(x)
    assert sum(len(d) for d in want) > 0
    det = Detector(m, PostProcess())
    _same(det(x), want)
    _same(Detector(m)(x), want)
    _same(m(x), want)                                                               # model(x) is what it was: the plan's buffers are intact
    # a candidate buffer that is too small is an error that names the image, never a silent drop
    with pytest.raises(MnyError, match=r"image \d+ has \d+ candidates more"):
        Detector(m, PostProcess(conf_thres=0.0, multi_label=True, max_candidates=10))(x)
    _same(m(x), want)
    _same(det(x), want)
    m.train()
    with pytest.raises(MnyError, match="model.eval"):
        det(x)


def test_detector_on_a_seg_config_returns_the_seg_map_of_model():
    from mobilenet_yolo_pytorch_amd import Detector, PostProcess, yolo
    man = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))
    torch.manual_seed(0)
    m = yolo(man["config"], sync_metrics=True)
    procedural.fill_state_dict_(m)
    m = m.cuda().eval()
    x = procedural.images(2, 64, 64, seed=22).cuda()
    want, seg = m(x)
    z = m.seg_logits()
    got, got_seg = Detector(m, PostProcess())(x)
    _same(got, want)
    assert isinstance(got_seg, np.ndarray) and np.array_equal(got_seg, seg) and torch.equal(m.seg_logits(), z)


def test_tta_with_default_options_equals_tta_bitwise():
    from mobilenet_yolo_pytorch_amd import PostProcess
    from mobilenet_yolo_pytorch_amd.tta import TTA
    m = _model(0.3)
    x = procedural.images(2, 96, 96, seed=10).cuda()
    views = [(96, False), (64, True)]
    want = TTA(m, views)(x)
    assert sum(len(d) for d in want) > 0
    _same(TTA(m, views, post=PostProcess())(x), want)
    _same(TTA(m, views, merge=False, post=PostProcess())(x), TTA(m, views, merge=False)(x))
    capped = TTA(m, views, post=PostProcess(max_det=3, agnostic=True))(x)
    assert [len(d) for d in capped] == [min(3, len(d)) for d in TTA(m, views, post=PostProcess(agnostic=True))(x)]


def test_detector_options_equal_the_restated_pipeline_on_the_same_heads():
    """multi_label + agnostic + max_det + a class filter: the plan's own heads through the restatement (decode of both heads appended
    per image, agnostic NMS, top-k); counts and classes exact.  Rows: atol=1e-4, the decode tolerance, plus rtol=1e-6: procedural
    weights give boxes thousands of units wide (exp(tw) of a large logit), where one ulp of fp32 is already 4e-3, so an absolute bound
    alone cannot hold; device expf and numpy exp agree to a few ulp and the four roundings of the box arithmetic follow, 16 ulp = 1e-6
    relative bounds the sum.  The thresholds keep 1e-5 away from every conf and score of these heads (asserted on the restatement)."""
    from mobilenet_yolo_pytorch_amd import Detector, PostProcess
    m = _model(0.3)
    x = procedural.images(2, 96, 96, seed=10).cuda()
    classes = [c for c in range(20) if c != 4]
    post = PostProcess(conf_thres=0.2, score_thres=0.1, iou_thres=0.5, multi_label=True, agnostic=True, max_det=6, classes=classes)
    det = Detector(m, post)(x)
    plan = m._plans[(2, 96, 96, False)]
    words = post_ref.class_mask_words(classes, 20)
    per_image = [[] for _ in range(2)]
    for hi in range(2):
        head, anchors, mask = plan.heads[hi].cpu().numpy(), plan.anchors[hi].cpu().numpy(), plan.masks[hi].tolist()
        m_obj, m_score = post_ref.margins(head, anchors, mask, 0.2, 0.1)
        assert m_obj > 1e-5 and m_score > 1e-5, (m_obj, m_score)
        for n, r in enumerate(post_ref.decode_candidates(head, anchors, mask, 0.2, 0.1, True, words)):
            per_image[n].append(r)
    capped = 0
    for n in range(2):
        rows = np.concatenate(per_image[n])
        assert len(rows) > 50 and 4 not in rows[:, 6]
        kept = post_ref.nms_agnostic(rows, 0.5)
        capped += len(kept) > 6
        want = rows[post_ref.det_topk(rows, kept, 6)]
        got = det[n].cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got[:, 6], want[:, 6])
        np.testing.assert_allclose(got[:, :6], want[:, :6], rtol=1e-6, atol=1e-4)
    assert capped > 0, "max_det never bites: the case is vacuous"
