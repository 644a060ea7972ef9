"""The crowded-scene inputs of the YOLO-loss tests, in one place: tests/test_oracle_detect.py asserts on the CPU that every
case enters the branches and keeps its distance from every threshold, tests/test_gpu_detect.py runs the same cases through
the HIP kernels.  Inputs are regenerated from the seed (oracle/procedural.py crowded_scene); nothing is stored.

Seeds were picked with the oracle alone (yolo_ref.loss_branches): the first seed from 0 whose margins are at least three
times the deltas below.  Rejected on the way: voc-g13 seed 0 (cell edge 2.8e-4), voc-g22 seeds 0-2 (ignore margin 2.9e-5,
7.6e-5; cell edge 1.8e-4), bdd-g26 seed 0 (cell edge 1.6e-4), voc-n256 seeds 0-2 (ignore margin 1.3e-6; argmax gap 1.4e-5;
anchor margin 1.7e-5), one-image-200 seed 0 (ignore margin 9.1e-5)."""
import json
import os

from oracle import procedural, yolo_ref

G = os.path.join(os.path.dirname(__file__), "golden")

# id: (config, N, g, head, seed, max_targets, per-image counts or None)
CROWDED = {
    "voc-g10": ("voc", 8, 10, 0, 0, 40, None),
    "voc-g11": ("voc", 8, 11, 0, 0, 40, None),          # also pinned against the real reference (loss_crowded.npz)
    "voc-g13": ("voc", 12, 13, 0, 1, 40, None),
    "voc-g19": ("voc", 6, 19, 0, 0, 40, None),
    "voc-g20": ("voc", 8, 20, 1, 0, 40, None),
    "voc-g22": ("voc", 8, 22, 1, 3, 40, None),          # also pinned against the real reference (loss_crowded.npz)
    "voc-g38": ("voc", 6, 38, 1, 0, 40, None),
    "voc-n64": ("voc", 64, 11, 0, 0, 16, None),
    "bdd-g26": ("bdd", 32, 26, 1, 1, 40, None),         # 7 classes, other anchors, 416 input
    "voc-n256": ("voc", 256, 22, 1, 3, 8, None),        # 371 712 cells: the grid-stride loops of passes 1 and 4
}
# compared with the oracle like the above, but too small or too lopsided for the minimum branch counts: margins only
EXTRA = {
    "one-image-200": ("voc", 6, 13, 0, 1, 40, [3, 200, 0, 1, 2, 5]),   # the serial loop of one thread of pass 2
    "n1": ("voc", 1, 11, 0, 0, 40, None),
}
ALL = dict(CROWDED, **EXTRA)

# every crowded case reaches at least these (yolo_ref.loss_branches)
MIN_COUNTS = {"dup_cell": 8, "two_cls": 3, "ign2pos": 10, "ignored": 100, "recall": 15, "zero_hit": 10}
# a target hits several anchors of one head only where two anchors are nested with area ratio > iou_thresh^2.  VOC's large
# anchors (head 0) offer that freely; head 1's pairs are further apart (only 49x94 inside 73x201 qualifies, with 2 % of
# slack in area), so head-1 cases need one, which crowded_scene's hand-made geometric-mean targets guarantee.
MIN_MULTI_ANCHOR = {0: 2, 1: 1}
# GPU expf / division differ from libm by a few ulp: on an IoU <= 1 an absolute 1e-6.  Ten times that on every IoU
# decision; 1e-4 of a cell on cx*g, cy*g (a float product of magnitude <= 38, ulp 4e-6).
IOU_DELTA = 1e-5
CELL_DELTA = 1e-4


def config(name):
    if name == "voc":
        return procedural.VOC_CONFIG
    return json.load(open(os.path.join(G, "state_keys_bdd100k.json")))["config"]


def make(case_id):
    """-> (spec, img, head_nchw, targets)"""
    cfg_name, N, g, hi, seed, max_targets, counts = ALL[case_id]
    cfg = config(cfg_name)
    spec = yolo_ref.specs_from_config(cfg)[hi]
    img = cfg["img_h"]
    head, tg = procedural.crowded_scene(N, g, spec, seed, img=img, max_targets=max_targets, counts=counts)
    return spec, img, head, tg
