"""CPU: the plan compiler (engine.NetPlan) builds the training plans of both architectures in both storage types on CPU tensors, through
the recording call list of tools/plan_listing.py (no kernel runs), and the lists have the structure the GPU tests see only after a full
step: which fused units were formed, every parameter gradient has a producer, marks and the gradient arena are laid out in order.

N=4, 96x96, MNY_SIDE_STREAM=0 (a side stream is a device object)."""
import collections
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("mbv2", "f32"), ("mbv2", "bf16"), ("mbv3", "f32"), ("mbv3", "bf16")]


@pytest.fixture(scope="module")
def plans():
    """The four plans, built once; engine.CallList and the environment are as before afterwards."""
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import plan_listing
    finally:
        sys.path.pop(0)
    from mobilenet_yolo_pytorch_amd import engine
    saved_cls, saved_env = engine.CallList, os.environ.get("MNY_SIDE_STREAM")
    os.environ["MNY_SIDE_STREAM"] = "0"
    try:
        built = {c: plan_listing.build_plan(REPO, c[0], c[1], 4, 96) for c in CASES}
        lines = {c: plan_listing.listing(p) for c, p in built.items()}
    finally:
        engine.CallList = saved_cls
        if saved_env is None:
            del os.environ["MNY_SIDE_STREAM"]
        else:
            os.environ["MNY_SIDE_STREAM"] = saved_env
    return built, lines


def _called(plan, which):
    """Counter of the entry points actually called by a list, and of the labels they stand for."""
    calls = getattr(plan, which).calls
    return (collections.Counter(getattr(c[0], "__name__", c[2]) for c in calls), collections.Counter(c[2] for c in calls))


def test_every_plan_builds_with_both_lists_and_a_listing(plans):
    built, lines = plans
    for c in CASES:
        p = built[c]
        assert 100 < len(p.fwd.calls) < 400 and 100 < len(p.bwd.calls) < 600, (c, len(p.fwd.calls), len(p.bwd.calls))
        assert len(lines[c]) == len(p.fwd.calls) + len(p.bwd.calls) + 4
        assert not p.side_on and not any(ln.split()[2].startswith("py:") for ln in lines[c][:-4])     # no fork / join without a side stream


def test_mobilenetv2_fp32_forms_its_fused_units(plans):
    p = plans[0][("mbv2", "f32")]
    fwd, _ = _called(p, "fwd")
    bwd, bwd_labels = _called(p, "bwd")
    assert bwd["mny_stemdw_bwd"] == 1 and bwd["mny_stem_bnwgrad"] == 0
    assert bwd["mny_pj_bwd"] == 6
    assert fwd["mny_exdw_fwd"] == fwd["mny_exdw_stats"] == bwd_labels["mny_exdw_bwd"] >= 1
    assert bwd["mny_exdw_bwd"] + bwd["mny_exdw_bwd_red"] == bwd_labels["mny_exdw_bwd"]
    assert len(p.exdw_pw) == len(p.exdw_dw) == fwd["mny_exdw_fwd"]


def test_mobilenetv3_bf16_forms_its_gates(plans):
    p = plans[0][("mbv3", "bf16")]
    assert len(p.gates) == 8 and all(set(g) >= {"t", "se0", "se3", "mul", "add"} for g in p.gates.values())
    assert sum(1 for u in p.units.values() if u.Y is None) == 16          # the two hidden units of every gate are never materialised
    fwd, _ = _called(p, "fwd")
    bwd, _ = _called(p, "bwd")
    assert fwd["mny_gate_fwd_bf16"] == bwd["mny_gate_bwd1_bf16"] == bwd["mny_gate_bwd2_bf16"] == bwd["mny_gate_bwd3_bf16"] == 8


@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_every_parameter_gradient_has_a_producer(plans, case):
    """Every slot of the arena is an argument of some backward call, or the destination of a deferred combine (meta `writes`)."""
    p = plans[0][case]
    import torch
    seen = set()
    for entry in p.bwd.calls:
        seen.update(a.data_ptr() for a in p.bwd.raw.get(id(entry), ()) if isinstance(a, torch.Tensor))
        seen.update((entry[3] or {}).get("writes", ()))
    missing = [nm for nm in p.grad_params if p.gviews[nm].data_ptr() not in seen]
    assert not missing, missing
    assert len(p.grad_params) == len(set(p.grad_params)) == len(p.grad_slots) > 100


@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_marks_follow_the_list_and_the_arena_is_laid_out_in_order(plans, case):
    """bwd.marks (node name -> index behind the node's calls, in backward node order) never go back and end where the list ends — but for
    the one forced combine of the deferred weight-gradient partials that closes every list (fork, mny_reduce_batch and the low-rank
    corrections it triggers), which belongs to no node: the last mark is the index at which exactly that tail begins.  (The marks of the
    parent commit are the same: 261 of 264 calls for MobileNetV2 fp32, one less than the length for the other three plans.)
    grad_slots: offsets sorted, 4-float aligned, the last slot's end (rounded up to 4 floats) is the end of gflat."""
    p = plans[0][case]
    marks = list(p.bwd.marks.values())
    assert marks == sorted(marks) and marks[0] > 0
    tail = [c[2] for c in p.bwd.calls[marks[-1]:]]
    assert marks[-1] <= len(p.bwd.calls) and tail.count("mny_reduce_batch") <= 1
    assert all(name in ("fork", "mny_reduce_batch", "mny_lr_wfix") for name in tail), tail
    if tail:
        assert tail[0] == "mny_reduce_batch"                     # (fork only with a side stream)
    offs = [p.grad_slots[nm][0] for nm in p.grad_params]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 4 == 0 for o in offs)
    assert all(offs[k] + p.grad_slots[p.grad_params[k]][1] <= offs[k + 1] for k in range(len(offs) - 1))
    last = p.grad_params[-1]                                    # the stem's BatchNorm bias: no padded-head slack behind it, its extent is its
    assert last.endswith(".bias") and p.net.param_tensors[last].dim() == 1     # size rounded up to 4 floats
    assert offs[-1] + (p.grad_slots[last][1] + 3) // 4 * 4 == p.gflat.numel()
