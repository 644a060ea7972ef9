"""Oracle pinning: oracle/yolo_ref.py vs fixtures captured from the real reference
(tools/gen_golden.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import crowded_cases as CC
from oracle import procedural, yolo_ref

G = os.path.join(os.path.dirname(__file__), "golden")


def _targets(z):
    return list(torch.split(torch.from_numpy(z["t_all"]), z["t_counts"].tolist()))


def test_iou_and_ciou_tables():
    z = np.load(os.path.join(G, "iou_tables.npz"))
    a, b = torch.from_numpy(z["a"]), torch.from_numpy(z["b"])
    iou = yolo_ref.pair_iou(a, b).numpy()
    assert np.array_equal(np.isnan(iou), np.isnan(z["iou"]))          # 0/0 -> NaN like the reference
    assert np.array_equal(np.nan_to_num(iou), np.nan_to_num(z["iou"]))  # bit-exact
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            t, u = yolo_ref.ciou_pair(a[i:i + 1], b[j:j + 1])
            got = np.array([t.item(), u.item()], np.float32)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(z["ciou"][i, j]))
            np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(z["ciou"][i, j]), rtol=0, atol=1e-7)


def test_q1_box_weights_cancel():
    z = np.load(os.path.join(G, "iou_tables.npz"))
    x = torch.from_numpy(z["q1_x"])
    ref = float(z["q1"])
    assert abs(float(((x - 1) ** 2).sum()) - ref) < 1e-6


def test_loss_tuple_and_grad_match_reference():
    z = np.load(os.path.join(G, "loss_decode.npz"))
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    tg = _targets(z)
    for hi in range(2):
        head = torch.from_numpy(z["head%d" % hi]).clone().requires_grad_(True)
        res = yolo_ref.loss_forward(head, tg, specs[hi], [352, 352])
        res[0].backward()
        got = np.array([float(v) for v in res])
        np.testing.assert_allclose(got, z["tuple%d" % hi], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(head.grad.numpy(), z["grad%d" % hi], rtol=1e-5, atol=1e-9)
        assert z["tuple%d" % hi][6] > 0                                # fixtures do contain positives


def test_crowded_loss_tuple_and_grad_match_reference():
    """The oracle against the real YOLOLoss on two crowded scenes (voc-g11, voc-g22 of crowded_cases): 10+ repeated-cell
    positives per head, cells with two class bits, ignored-then-positive cells, targets on several anchors.  Same tolerances as
    test_loss_tuple_and_grad_match_reference; the checksums show that the generator still produces the captured inputs."""
    z = np.load(os.path.join(G, "loss_crowded.npz"))
    for hi, cid in enumerate(("voc-g11", "voc-g22")):
        assert z["case%d" % hi].tolist() == list(CC.ALL[cid][1:3]) + [CC.ALL[cid][4]]
        spec, img, head, tg = CC.make(cid)
        t_all = torch.cat(tg)
        sums = [head.double().sum().item(), head.double().abs().sum().item(), t_all.double().sum().item(),
                (t_all.double() ** 2).sum().item(), float(len(t_all))]
        np.testing.assert_allclose(sums, z["sum%d" % hi], rtol=1e-12, atol=0)
        br = yolo_ref.loss_branches(head, tg, spec, [img, img])
        assert br["dup_cell"] >= 10 and br["two_cls"] >= 3 and br["multi_anchor_t"] >= 1, br
        hr = head.clone().requires_grad_(True)
        res = yolo_ref.loss_forward(hr, tg, spec, [img, img])
        res[0].backward()
        np.testing.assert_allclose(np.array([float(v) for v in res]), z["tuple%d" % hi], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(hr.grad.numpy(), z["grad%d" % hi], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("cid", sorted(CC.ALL))
def test_crowded_cases_enter_the_branches_and_keep_off_the_thresholds(cid):
    """Every input that tests/test_gpu_detect.py compares with the oracle: the minimum branch counts (crowded cases), and every
    decision at least IOU_DELTA (1e-5) from its IoU threshold / CELL_DELTA (1e-4) from a cell edge, so that the few-ulp
    difference between the GPU's expf / division and libm cannot flip one.  Several anchors per target: >= 2 on head-0 cases
    only, >= 1 on head 1 (crowded_cases.MIN_MULTI_ANCHOR says why).  Seeds are chosen so that this holds; no case is dropped."""
    spec, img, head, tg = CC.make(cid)
    br = yolo_ref.loss_branches(head, tg, spec, [img, img])
    print(cid, br)
    assert br["nan"] == 0 and br["outside"] == 0 and br["bad_label"] == 0
    if cid in CC.CROWDED:
        for k, v in CC.MIN_COUNTS.items():
            assert br[k] >= v, (cid, k, br[k], v)
        assert br["multi_anchor_t"] >= CC.MIN_MULTI_ANCHOR[CC.ALL[cid][3]], (cid, br["multi_anchor_t"])
    for k in ("m_ignore", "m_recall", "m_anchor", "m_argmax"):
        assert br[k] >= CC.IOU_DELTA, (cid, k, br[k])
    assert br["m_cell"] >= CC.CELL_DELTA, (cid, br["m_cell"])


def test_loss_branches_of_the_earlier_direct_cases_stay_sparse_and_skip_outside():
    """loss_branches on the hand-made fixture counts what was hand-made (one repeated cell on head 1, with two classes), and
    skip_outside drops exactly the positives of a target whose cell lies outside the grid while keeping it in the ignore mask."""
    z = np.load(os.path.join(G, "loss_decode.npz"))
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    tg = _targets(z)
    b1 = yolo_ref.loss_branches(torch.from_numpy(z["head1"]), tg, specs[1], [352, 352])
    assert b1["dup_cell"] == 1 and b1["two_cls"] == 1 and b1["outside"] == 0
    assert b1["pos"] == int(round(z["tuple1"][6] * 4))
    head = torch.from_numpy(z["head0"])
    inside = [t.clone() for t in tg]
    out = [t.clone() for t in tg]
    out[3] = torch.cat((out[3], torch.tensor([[4, 1.0, 0.5, 0.4, 0.7]])))              # cx*g == g: reference raises IndexError
    with pytest.raises(IndexError):
        yolo_ref.loss_forward(head, out, specs[0], [352, 352])
    a = yolo_ref.loss_forward(head, inside, specs[0], [352, 352])
    b = yolo_ref.loss_forward(head, out, specs[0], [352, 352], skip_outside=True)
    assert yolo_ref.loss_branches(head, out, specs[0], [352, 352])["outside"] == 1
    assert a[6] == b[6]                                                                # no positive added
    assert float(a[0]) != float(b[0])                                                  # but its box does ignore cells
    assert [float(v) for v in yolo_ref.loss_forward(head, inside, specs[0], [352, 352], skip_outside=True)] == [float(v) for v in a]


def test_loss_layout_nhwc_equals_nchw():
    z = np.load(os.path.join(G, "loss_decode.npz"))
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    head = torch.from_numpy(z["head1"])
    a = yolo_ref.loss_forward(head, _targets(z), specs[1], [352, 352])
    b = yolo_ref.loss_forward(head.permute(0, 2, 3, 1).contiguous(), _targets(z), specs[1], [352, 352], layout="nhwc")
    assert float(a[0]) == float(b[0])


def test_decode_rows_bit_exact():
    z = np.load(os.path.join(G, "loss_decode.npz"))
    specs = yolo_ref.specs_from_config(procedural.VOC_CONFIG)
    for hi in range(2):
        head = torch.from_numpy(z["head%d" % hi])
        for vc in (1, 3, 5):
            specs[hi].val_conf = vc / 10
            rows = yolo_ref.decode_rows(head, specs[hi], [352, 352])
            assert [len(r) for r in rows] == z["dec%d_%d_counts" % (hi, vc)].tolist()
            assert np.array_equal(torch.cat(rows).numpy(), z["dec%d_%d_rows" % (hi, vc)])   # Q13: bit-identical


def test_state_key_manifest_counts():
    for name, n in (("voc", 430), ("bdd100k", 450)):
        m = json.load(open(os.path.join(G, "state_keys_%s.json" % name)))
        assert len(m["keys"]) == n
