"""Segmentation evaluator on the GPU (csrc/segeval.hip, segeval.py) against the float64 restatement tests/segeval_ref.py: the
interpolated probabilities within 2^-19, the predicted id maps at every unambiguous pixel, the confusion matrix exactly, the
metrics bit for bit; accumulation, determinism, the label containers of SegEvaluator.add, and yolo.seg_logits() on the BDD100K
config.  The inputs (segeval_ref.CASES) and their ambiguity conditions are checked on the CPU by tests/test_segeval_ref_cpu.py."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import segeval_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, labels, reference results) of a case, computed once and shared; nothing below writes into them."""
    x, labels = R.make_case(name)
    return x, labels, R.evaluate(x, labels, R.CASES[name][3])


def run_case(name, **kw):
    """-> (evaluator, predicted id maps as numpy) of one add() on the case's inputs."""
    from mobilenet_yolo_pytorch_amd import segeval
    x, labels, _ = case(name)
    ev = segeval.SegEvaluator(R.CASES[name][3])
    preds = ev.add(torch.from_numpy(x).cuda(), labels, pred_out=True, **kw)
    return ev, [p.cpu().numpy() for p in preds]


def same(a, b):
    """equal values, NaN at the same places"""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_upsample_within_the_error_budget(name):
    from mobilenet_yolo_pytorch_amd import segeval
    x, labels, ref = case(name)
    got = segeval.upsample(torch.from_numpy(x).cuda(), [l.shape for l in labels])
    worst = 0.0
    for g, want in zip(got, ref["values"]):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == want.shape
        assert np.array_equal(np.isnan(g), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            worst = max(worst, float(np.abs(g.astype(np.float64) - want)[ok].max()))
    print("%s: max |v_gpu - v_ref| = %.3e (2^-19 = %.3e)" % (name, worst, R.VALUE_TOL))
    assert worst <= R.VALUE_TOL


def test_identity_size_is_the_sigmoid_bit_for_bit():
    from mobilenet_yolo_pytorch_amd import _lib, segeval
    x = torch.from_numpy(np.random.RandomState(5).normal(0, 2, (3, 6, 9, 2)).astype(np.float32)).cuda()
    got = segeval.upsample(x, [(6, 9)] * 3)
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    for i in range(3):
        want = torch.zeros(2, 6, 9, device="cuda")
        _lib.call("mny_seg_sigmoid", p(x[i:i + 1].contiguous()), 6, 9, 2, p(want), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert torch.equal(got[i], want)
    pred = segeval.predict(x, [(6, 9)] * 3)
    for i in range(3):
        v = got[i]
        want = torch.where(v.max(0).values > 0.5, v.argmax(0) + 1, torch.zeros_like(v.argmax(0))).to(torch.uint8)
        assert torch.equal(pred[i], want)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_predictions_and_confusion(name):
    x, labels, ref = case(name)
    C = R.CASES[name][3]
    ok, n_amb, n_pix = R.ambiguity_ok(name, ref)
    assert ok, "%s: %d of %d pixels are ambiguous" % (name, n_amb, n_pix)
    ev, preds = run_case(name)
    conf, ign = ev.confusion.cpu().numpy(), int(ev.ignored.item())
    own = np.zeros_like(conf)
    for got, want, amb, lab in zip(preds, ref["preds"], ref["ambiguous"], labels):
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got[~amb], want[~amb])
        own += R.confusion(got, lab, C)[0]
    assert conf.dtype == np.int64 and np.array_equal(conf, own)         # the matrix is the one of the GPU's own id maps
    assert ign == ref["ignored"] and conf.sum() + ign == n_pix
    if n_amb == 0:
        assert np.array_equal(conf, ref["conf"])
    # metrics: each value one division of exact integers; the two means within (C + 1) ulps of 1
    r = ev.compute_device()
    got = torch.cat([r["iou"], r["miou"], r["miou_fg"], r["pixel_acc"]]).cpu().numpy()
    want = R.metrics(conf)
    assert got.dtype == np.float64 and same(got[:C + 1], want[:C + 1]) and same(got[C + 3], want[C + 3])
    for k in (C + 1, C + 2):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or abs(got[k] - want[k]) <= (C + 1) * 2.0 ** -52
    d = ev.compute()
    assert list(d["iou"]) == ev.class_names and same(np.array(list(d["iou"].values())), want[:C + 1])
    assert same(np.array([d["miou"], d["miou_fg"], d["pixel_acc"]]), got[C + 1:])


def test_degenerate_label_sets_give_nan_metrics_without_error():
    for name in ("all_background", "all_one_class"):
        ev, _ = run_case(name)
        m = ev.compute()
        iou = list(m["iou"].values())
        conf = ev.confusion.cpu().numpy()
        for k in range(3):
            assert np.isnan(iou[k]) == (conf[k].sum() + conf[:, k].sum() == 0)
        assert not np.isnan(m["pixel_acc"])
    ev, _ = run_case("all_ignored")
    m = ev.compute()
    assert int(ev.confusion.sum()) == 0 and int(ev.ignored.item()) == 48 * 80 + 9 * 17
    assert all(np.isnan(v) for v in m["iou"].values()) and np.isnan(m["miou"]) and np.isnan(m["miou_fg"]) and np.isnan(m["pixel_acc"])


def test_accumulation_merge_reset_and_determinism():
    from mobilenet_yolo_pytorch_amd import segeval
    x, labels, ref = case("many70_c2")
    xs = torch.from_numpy(x).cuda()
    a = segeval.SegEvaluator(2)
    a.add(xs, labels)
    once, ign = a.confusion.clone(), a.ignored.clone()
    a.add(xs, labels)
    assert torch.equal(a.confusion, 2 * once) and torch.equal(a.ignored, 2 * ign)
    b = segeval.SegEvaluator(2)
    pa = b.add(xs, labels, pred_out=True)
    assert torch.equal(b.confusion, once) and torch.equal(b.ignored, ign)          # two runs: bit-identical
    pb = segeval.predict(xs, [l.shape for l in labels])
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))                          # pred_out without labels: the same maps
    b.merge(a)
    assert torch.equal(b.confusion, 3 * once) and torch.equal(b.ignored, 3 * ign)
    b.reset()
    assert int(b.confusion.sum()) == 0 and int(b.ignored.item()) == 0
    half = segeval.SegEvaluator(2)                                                  # a split batch adds up to the whole
    half.add(xs[:30], labels[:30])
    half.add(xs[30:], labels[30:])
    assert torch.equal(half.confusion, once) and torch.equal(half.ignored, ign)


def test_add_takes_host_lists_device_lists_and_one_tensor():
    from mobilenet_yolo_pytorch_amd import segeval
    x, labels, ref = case("nonint_c2")                                              # (50,90), (48,80), (50,90)
    xs = torch.from_numpy(x).cuda()
    want = torch.from_numpy(ref["conf"]).cuda()

    def conf_of(xs, labs, **kw):
        ev = segeval.SegEvaluator(2)
        ev.add(xs, labs, **kw)
        return ev.confusion, int(ev.ignored.item())
    assert torch.equal(conf_of(xs, labels)[0], want)
    assert torch.equal(conf_of(xs, [torch.from_numpy(l) for l in labels])[0], want)
    dev = [torch.from_numpy(l).cuda() for l in labels]
    assert torch.equal(conf_of(xs, dev)[0], want)
    assert torch.equal(conf_of(xs, [dev[0], labels[1], dev[2]])[0], want)           # mixed members
    odd = torch.zeros(50 * 90 + 3, dtype=torch.uint8, device="cuda")                # a member at an odd address is copied
    odd[3:] = dev[0].reshape(-1)
    assert torch.equal(conf_of(xs, [odd[3:].view(50, 90), dev[1], dev[2]])[0], want)
    assert torch.equal(conf_of(xs, dev, pred_out=True)[0], want)
    # one [N,H,W] tensor, H*W a multiple of 16 (in place) and not (padded per image)
    for idx, size in (((1, 1), (48, 80)), ((0, 2), (50, 90))):
        sub = xs[list(idx)]
        r = R.evaluate(x[list(idx)], [labels[i] for i in idx], 2)
        stack = np.stack([labels[i] for i in idx])
        assert stack.shape[1:] == size
        for t in (torch.from_numpy(stack), torch.from_numpy(stack).cuda()):
            c, ig = conf_of(sub, t)
            assert np.array_equal(c.cpu().numpy(), r["conf"]) and ig == r["ignored"]
    with pytest.raises(ValueError, match="label maps for"):
        conf_of(xs, labels[:2])
    with pytest.raises(ValueError, match="channels"):
        segeval.SegEvaluator(3).add(xs, labels)


def _bdd(act_dtype):
    from oracle import procedural
    from mobilenet_yolo_pytorch_amd import yolo
    man = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))
    torch.manual_seed(0)
    m = yolo(man["config"], sync_metrics=True, act_dtype=act_dtype)
    procedural.fill_state_dict_(m)
    return man["config"], m.cuda().eval()


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_module_seg_logits(act_dtype):
    from oracle import procedural
    from mobilenet_yolo_pytorch_amd import MnyError, segeval
    cfg, m = _bdd(act_dtype)
    C = cfg["seg"]["num_classes"]
    with pytest.raises(MnyError, match="no eval forward"):
        m.seg_logits()
    x = procedural.images(2, 64, 64, seed=22).cuda()
    det, seg = m(x)
    assert isinstance(det, list) and len(det) == 2 and isinstance(seg, np.ndarray) and seg.shape == (C, 4, 4)
    z = m.seg_logits()
    assert z.shape == (2, 4, 4, C) and z.dtype == torch.float32 and z.is_cuda
    up = segeval.upsample(z[:1], [(4, 4)])[0]
    assert np.array_equal(up.cpu().numpy(), seg)                                    # image 0 at the identity size IS seg_out
    det2, seg2 = m(x)                                                               # the eval return is what it was
    assert np.array_equal(seg, seg2) and [tuple(a.shape) for a in det] == [tuple(b.shape) for b in det2]
    assert torch.equal(z, m.seg_logits())                                           # ... and z was a clone
    ev = segeval.SegEvaluator(C)
    labels = [np.random.RandomState(i).randint(0, C + 1, (64, 64)).astype(np.uint8) for i in range(2)]
    ev.add(z, labels)
    assert int(ev.confusion.sum()) == 2 * 64 * 64


@pytest.mark.parametrize("act_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_seg_logits_needs_a_seg_section(act_dtype):
    from oracle import procedural
    from mobilenet_yolo_pytorch_amd import MnyError, yolo
    m = yolo(procedural.VOC_CONFIG, act_dtype=act_dtype).cuda().eval()
    with pytest.raises(MnyError, match="seg"):
        m.seg_logits()
    m(procedural.images(2, 64, 64, seed=1).cuda())
    with pytest.raises(MnyError, match="seg"):
        m.seg_logits()
