"""CPU: the frozen-parameter frontier (mobilenet_yolo_pytorch_amd.frontier) on the three graphs, the plan-cache key's signature of the
frozen set and the BatchNorm modes, the BatchNorm-mode refusals, and the data-parallel buckets over an arena of trainable slots only."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mobilenet_yolo_pytorch_amd import MnyError, arch, dp, frontier
from oracle import procedural

G = os.path.join(os.path.dirname(__file__), "golden")


def _graphs():
    bdd = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))["config"]
    y = procedural.VOC_CONFIG["yolo"]
    return {"mbv2_voc": arch.mbv2_yolo_graph(y["num_classes"], y["num_anchors"]),
            "mbv2_bdd": arch.mbv2_yolo_graph(bdd["yolo"]["num_classes"], bdd["yolo"]["num_anchors"], bdd["seg"]["num_classes"]),
            "mbv3": arch.mbv3_yolo_graph(y["num_classes"], y["num_anchors"])}


def _all_params(g):
    return [nm for nd in g.nodes for nm in frontier.node_params(nd)]


def _is_backbone(nd):
    return (nd.conv or nd.out.name).startswith("backbone.")


@pytest.mark.parametrize("which", ["mbv2_voc", "mbv2_bdd", "mbv3"])
def test_all_trainable_keeps_every_live_node(which):
    g = _graphs()[which]
    live = frontier.live_values(g)
    fr = frontier.Frontier(g)
    assert [nd.out.id for nd in fr.order] == [nd.out.id for nd in reversed(g.nodes) if nd.out.id in live]
    assert fr.grad_values == live
    want = []
    for nd in fr.order:
        want += [nm for nm in frontier.node_params(nd) if nm not in want]
    assert fr.grad_params == want and len(set(want)) == len(want)
    if which == "mbv2_voc":
        assert len(fr.grad_params) == 202                      # the dead seg branch of a config without a `seg` section takes no gradient
        assert any(nd.out.id not in live for nd in g.nodes)
    if which == "mbv2_bdd":
        assert fr.grad_values == {nd.out.id for nd in g.nodes}


@pytest.mark.parametrize("which", ["mbv2_voc", "mbv2_bdd", "mbv3"])
def test_frozen_backbone_cuts_at_the_neck(which):
    g = _graphs()[which]
    live = frontier.live_values(g)
    frozen = {nm for nm in _all_params(g) if nm.startswith("backbone.")}
    fr = frontier.Frontier(g, frozen)
    assert frozen
    fed = 0
    for nd in g.nodes:
        if _is_backbone(nd):
            assert not fr.needs_grad(nd.out), nd.out.name
            continue
        assert fr.needs_grad(nd.out) == (nd.out.id in live), nd.out.name
        for v in nd.ins:                                         # the units fed by the backbone's two outputs need no input gradient
            if v.node is not None and _is_backbone(v.node):
                assert not fr.needs_grad(v), (nd.out.name, v.name)
                fed += fr.needs_grad(nd.out)
            elif fr.needs_grad(nd.out):
                assert fr.needs_grad(v), (nd.out.name, v.name)
    assert fed >= 2
    assert not any(nm.startswith("backbone.") for nm in fr.grad_params)
    full = frontier.Frontier(g)
    assert fr.grad_params == [nm for nm in full.grad_params if nm not in frozen]          # production order unchanged


@pytest.mark.parametrize("which", ["mbv2_voc", "mbv2_bdd", "mbv3"])
def test_only_the_last_head_conv_trainable(which):
    g = _graphs()[which]
    frozen = {nm for nm in _all_params(g) if not nm.startswith("yolo_headS32.3.")}
    fr = frontier.Frontier(g, frozen)
    assert [nd.conv for nd in fr.order] == ["yolo_headS32.3"]
    assert fr.grad_params == ["yolo_headS32.3.weight", "yolo_headS32.3.bias"]
    assert not fr.needs_grad(fr.order[0].ins[0])
    # a conv in the middle of the S32 branch: exactly the nodes on a path from it to a loss
    frozen = {nm for nm in _all_params(g) if nm != "connect_for_S32.conv.1.conv.weight"}
    fr = frontier.Frontier(g, frozen)
    src = next(nd for nd in g.nodes if nd.conv == "connect_for_S32.conv.1.conv")
    reach = {src.out.id}
    for nd in g.nodes:
        if any(v.id in reach for v in nd.ins):
            reach.add(nd.out.id)
    assert fr.grad_values == reach & frontier.live_values(g)
    assert len(fr.grad_values) > 4 and not fr.needs_grad(src.ins[0])
    assert fr.grad_params == ["connect_for_S32.conv.1.conv.weight"]


@pytest.mark.parametrize("which", ["mbv2_voc", "mbv3"])
def test_frozen_parameter_above_a_trainable_one_keeps_its_node_and_loses_its_slot(which):
    g = _graphs()[which]
    frozen = {nm for nd in g.nodes if nd.bn for nm in (nd.bn + ".weight", nd.bn + ".bias")}       # BN affine frozen, convs train
    fr, full = frontier.Frontier(g, frozen), frontier.Frontier(g)
    assert [nd.out.id for nd in fr.order] == [nd.out.id for nd in full.order]
    assert fr.grad_values == full.grad_values
    assert fr.grad_params == [nm for nm in full.grad_params if nm not in frozen] and fr.grad_params
    # one frozen conv in the head: its node stays (the neck below it trains), its slot goes
    fr = frontier.Frontier(g, {"yolo_headS16.1.conv.weight"})
    assert fr.grad_values == full.grad_values
    assert fr.grad_params == [nm for nm in full.grad_params if nm != "yolo_headS16.1.conv.weight"]


def test_mbv3_module_applied_twice_has_one_slot_and_two_contributions():
    g = _graphs()["mbv3"]

    def applications(fr):
        n = {}
        for nd in fr.order:
            if nd.conv:
                n[nd.conv] = n.get(nd.conv, 0) + 1
        return n
    fr = frontier.Frontier(g)
    uses = applications(fr)
    for conv in ("connect_for_S16.conv.0.conv", "connect_for_S16.conv.1.conv"):
        assert uses[conv] == 2
        assert fr.grad_params.count(conv + ".weight") == 1
    assert sum(1 for n in uses.values() if n == 2) == 2 and max(uses.values()) == 2
    frozen = {nm for nm in _all_params(g) if nm.startswith("backbone.")}
    fz = frontier.Frontier(g, frozen)
    assert applications(fz)["connect_for_S16.conv.0.conv"] == 2  # both applications sit above the frontier
    first = next(nd for nd in g.nodes if nd.conv == "connect_for_S16.conv.0.conv")
    assert not fz.needs_grad(first.ins[0])                       # the first application reads the backbone: no input gradient
    second = [nd for nd in g.nodes if nd.conv == "connect_for_S16.conv.0.conv"][1]
    assert fz.needs_grad(second.ins[0])


def test_bn_mode_checks_name_the_module():
    g = _graphs()["mbv2_voc"]
    names = frontier.bn_names(g)
    frozen = {nm for nm in _all_params(g) if nm.startswith("backbone.")}
    fr = frontier.Frontier(g, frozen)
    backbone_bn = {nm for nm in names if nm.startswith("backbone.")}
    frontier.check_bn_modes(g, fr, backbone_bn)                  # (a) eval-mode BatchNorms below the frontier only
    frontier.check_bn_modes(g, fr, set())
    with pytest.raises(MnyError, match=r"connect_for_S32\.conv\.0\.bn"):
        frontier.check_bn_modes(g, fr, backbone_bn | {"connect_for_S32.conv.0.bn"})
    with pytest.raises(MnyError, match=r"backbone\.features\.3\.conv\.1 "):
        frontier.check_bn_modes(g, frontier.Frontier(g), {"backbone.features.3.conv.1"})          # backbone in eval but trainable
    frontier.check_fused_pair(["a.bn", "b.bn"], {"a.bn", "b.bn"}, "expand + depthwise")
    frontier.check_fused_pair(["a.bn", "b.bn"], set(), "expand + depthwise")
    with pytest.raises(MnyError, match=r"b\.bn is in eval mode.*a\.bn"):
        frontier.check_fused_pair(["a.bn", "b.bn"], {"b.bn"}, "expand + depthwise")


@pytest.mark.parametrize("archname", ["mbv2", "mbv3"])
def test_plan_key_follows_the_frozen_set_and_the_batchnorm_modes(archname):
    from mobilenet_yolo_pytorch_amd import mbv3, yolo
    m = (yolo if archname == "mbv2" else mbv3.yolo)(procedural.VOC_CONFIG).train()

    def key(mode=True):
        return m._plan_key(8, 352, 352, mode, 0, m.frozen_param_names(), m.bn_eval_names())
    base = key()
    assert base == (8, 352, 352, True)                           # nothing frozen, every BatchNorm training: the key of a plain training plan
    assert m.frozen_param_names() == () and m.bn_eval_names() == ()
    p = m.yolo_headS16[1].conv.weight
    p.requires_grad_(False)
    k1 = key()
    assert k1 != base and m.frozen_param_names() == ("yolo_headS16.1.conv.weight",)
    assert key("evalgrad") != m._plan_key(8, 352, 352, "evalgrad") and key("evalloss") == (8, 352, 352, "evalloss")
    p.requires_grad_(True)
    assert key() == base
    bn = m.yolo_headS16[1].bn
    bn.eval()
    k2 = key()
    assert k2 != base and k2 != k1 and m.bn_eval_names() == ("yolo_headS16.1.bn",)
    assert key("traindet") != (8, 352, 352, "traindet")
    bn.train()
    assert key() == base
    for q in m.backbone.parameters():
        q.requires_grad_(False)
    m.backbone.eval()
    k3 = key()
    assert k3 not in (base, k1, k2) and hash(k3) is not None
    assert m._plan_key(8, 352, 352, True, 1, m.frozen_param_names(), m.bn_eval_names()) != k3   # the second in-flight slot keeps its own plan
    assert set(m.frozen_param_names()) == {k for k, _ in m.named_parameters() if k.startswith("backbone.")}
    assert set(m.bn_eval_names()) == {k for k, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and k.startswith("backbone.")}
    m.train()
    for q in m.parameters():
        q.requires_grad_(True)
    assert key() == base


def test_frozen_names_are_the_graphs_parameter_names():
    from mobilenet_yolo_pytorch_amd import yolo
    m = yolo(procedural.VOC_CONFIG)
    for q in m.parameters():
        q.requires_grad_(False)
    assert sorted(m.frozen_param_names()) == sorted(set(_all_params(m.graph)))
    assert frontier.Frontier(m.graph, m.frozen_param_names()).order == []


def test_clip_grad_norm_waits_for_pending_all_reduces_however_the_parameters_arrive():
    from mobilenet_yolo_pytorch_amd import optim

    class Red:                                                  # stands in for the handle attach_data_parallel registers
        waits = 0

        def wait(self):
            self.waits += 1
    red = Red()
    dp._attached.add(red)
    try:
        lin = torch.nn.Linear(2, 2)                             # no .grad anywhere: the call ends after the wait
        optim.clip_grad_norm_(lin, 1.0)
        optim.clip_grad_norm_(lin.parameters(), 1.0)
        optim.clip_grad_norm_(lin.weight, 1.0)
        assert red.waits == 3
    finally:
        dp._attached.discard(red)


# ---- data-parallel: the buckets cover exactly the trainable slots ---------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_dp_cpu import FakePlan
        from mobilenet_yolo_pytorch_amd import yolo
        m = yolo(procedural.VOC_CONFIG)
        numel = {k: p.numel() for k, p in m.named_parameters()}
        frozen = {k for k in numel if k.startswith("backbone.")}
        fr = frontier.Frontier(m.graph, frozen)
        sizes = [numel[nm] for nm in fr.grad_params]
        plan = FakePlan(rank, sizes, slack={0: 76 * 1024, 1: 76})          # the padded S16 head's slots carry slack
        plan.names = list(fr.grad_params)
        red = dp.PlanReducer(plan, n_buckets=4)
        ext = dp.PlanReducer.slot_extents(plan)
        assert len(ext) == len(fr.grad_params) == len([k for k in numel if not k.startswith("backbone.") and not k.startswith("seg_")])
        assert red.buckets[0][0] == 0 and red.buckets[-1][1] == plan.gflat.numel() == sum(ext)
        assert all(red.buckets[i][1] == red.buckets[i + 1][0] for i in range(len(red.buckets) - 1))
        assert sum(sizes) <= sum(ext) and not any(nm in frozen for nm in fr.grad_params)
        red.run_backward()
        red.wait()
        for i, n in enumerate(plan.grad_params):
            assert torch.allclose(plan.gviews[n], torch.full((sizes[i],), 1.5 * (i + 1))), (rank, fr.grad_params[i])
        q.put((rank, "ok"))
    except Exception as e:                          # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_rank_buckets_cover_exactly_the_trainable_slots():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in procs]
    for p in procs:
        p.join(30)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res
