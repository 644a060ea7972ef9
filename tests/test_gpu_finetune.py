"""MI355X: fine-tuning plans — parameters with requires_grad == False take no gradient and cut the backward list at the frontier they
leave, BatchNorm modules in eval mode below it keep their statistics — and the fused gradient clipping (mny_grad_clip).

Oracle: oracle.net_ref.RefYolo (stock torch autograd) with the same requires_grad_ / eval() calls; procedural weights; the batch of
test_gpu_net.py::test_train_step_matches_oracle_bs8_352 (8 x 352 x 352, images seed 3, targets seed 4)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import net_ref, procedural

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _model(train=True, sync=True):
    from mobilenet_yolo_pytorch_amd import yolo
    torch.manual_seed(0)
    m = procedural.fill_state_dict_(yolo(procedural.VOC_CONFIG, sync_metrics=sync)).cuda()
    return m.train() if train else m.eval()


def _batch():
    return procedural.images(8, 352, 352, seed=3), procedural.targets(8, seed=4, empty_every=4)


def _freeze(m, prefix="backbone.", bn_eval=False):
    for k, p in m.named_parameters():
        if k.startswith(prefix):
            p.requires_grad_(False)
    if bn_eval:
        m.backbone.eval()
    return m


def _losses(res):
    return [float(r[0].detach()) for r in res]


def _step(m, x, tg, seg=None):
    """One step from cleared gradients -> (losses, {name: gradient clone}, {name: buffer clone})."""
    m.zero_grad(set_to_none=True)
    if seg is None:
        res = m(x, tg)
        sum(r[0] for r in res).backward()
        losses = _losses(res)
    else:
        res, so = m(x, tg, seg)
        (sum(r[0] for r in res) + so[0]).backward()
        losses = _losses(res) + [float(so[0].detach())]
    torch.cuda.synchronize()
    return (losses, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
            {k: b.clone() for k, b in m.named_buffers()})


@pytest.fixture(scope="module")
def full_step():
    """The unfrozen model's step on the batch: what every frozen variant must reproduce bit for bit on the parameters it still trains."""
    x, tg = _batch()
    return _step(_model(), x.cuda(), tg)


def _assert_bit_equal_to_full(got, full, trainable, what):
    assert got[0] == full[0], (what, got[0], full[0])
    assert sorted(got[1]) == sorted(trainable), (what, sorted(set(got[1]) ^ set(trainable))[:8])
    bad = [k for k in trainable if not torch.equal(got[1][k], full[1][k])]
    assert not bad, (what, len(bad), bad[:8])
    bad = [k for k in full[2] if not torch.equal(got[2][k], full[2][k])]
    assert not bad, (what, "buffers", bad[:8])


# ---- 4: fails without the feature -----------------------------------------------------------------------------------------------
def test_frozen_backbone_takes_no_gradient_and_no_optimizer_moves_it(full_step):
    from mobilenet_yolo_pytorch_amd import optim
    x, tg = _batch()
    for make in (lambda ps: optim.AdamW(ps, lr=1e-3, weight_decay=1e-2), lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2)):
        m = _freeze(_model())
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        res = m(x.cuda(), tg)
        (res[0][0] + res[1][0]).backward()
        for k, p in m.named_parameters():
            if k.startswith("backbone."):
                assert p.grad is None, k
            else:
                assert (p.grad is not None) == (k in full_step[1]), k       # every gradient the full step (and the oracle) has
        assert sum(p.grad is not None for p in m.parameters()) == 202 - sum(k.startswith("backbone.") for k in full_step[1])
        make(m.parameters()).step()
        torch.cuda.synchronize()
        for k, p in m.named_parameters():
            if k.startswith("backbone.") or p.grad is None:
                assert torch.equal(p.detach(), before[k]), k
            else:
                assert not torch.equal(p.detach(), before[k]), k             # the step is live: whatever has a gradient moves


# ---- 5: bit-equality with the full plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["backbone", "last_head_conv", "bn_affine"])
def test_trainable_gradients_equal_the_full_plans_bit_for_bit(full_step, case):
    """Train-mode BatchNorm everywhere, parameters frozen by requires_grad only: the trainable units run the same kernels on the same
    inputs, and the steps are bit-deterministic — so no tolerance."""
    m = _model()
    if case == "backbone":
        frozen = [k for k, _ in m.named_parameters() if k.startswith("backbone.")]
    elif case == "last_head_conv":
        frozen = [k for k, _ in m.named_parameters() if not k.startswith("yolo_headS32.3.")]
    else:
        frozen = [k for k, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) for k in (k + ".weight", k + ".bias")]
    P = dict(m.named_parameters())
    for k in frozen:
        P[k].requires_grad_(False)
    x, tg = _batch()
    got = _step(m, x.cuda(), tg)
    trainable = [k for k in full_step[1] if k not in set(frozen)]
    assert trainable and len(trainable) < 202
    _assert_bit_equal_to_full(got, full_step, trainable, case)
    plan = next(p for key, p in m._plans.items() if key[:4] == (8, 352, 352, True))
    assert plan.grad_params == [k for k in plan.frontier.grad_params] and set(plan.grad_params) == set(trainable)
    assert all(P[k].grad is None for k in frozen)
    if case == "last_head_conv":
        assert len(plan.bwd.calls) < 8


# ---- 6: frozen backbone with its BatchNorms in eval mode, against the oracle ----------------------------------------------------
def _assert_gradient_tensors_close(m, ref, tau):
    """test_gpu_net._assert_gradient_tensors_close's rule: ||g - g_ref|| <= tau * ||g_ref|| + 2e-5 per tensor -> (tensors compared, worst)."""
    rp = dict(ref.named_parameters())
    n_cmp, worst = 0, (0.0, None)
    for k, p in m.named_parameters():
        if rp[k].grad is None:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        a, b = p.grad.double().cpu(), rp[k].grad.double()
        d, nb = (a - b).norm().item(), b.norm().item()
        print("grad %-44s |g_ref| %.3e rel %.3e" % (k, nb, d / (nb + 1e-30)))
        assert d <= tau * nb + 2e-5, (k, d, nb, d / (nb + 1e-30))
        if nb > 1e-4 and d / nb > worst[0]:
            worst = (d / nb, k)
        n_cmp += 1
    return n_cmp, worst


def test_frozen_backbone_in_eval_mode_matches_the_oracle():
    """tau = 8e-2, the bound test_train_step_matches_oracle_bs8_352 holds the full step to at this batch (measured there: worst tensor
    3.1e-2, the fp32 reordering noise of ~55 training-mode BatchNorm layers over 8 images).  This configuration keeps 20 of those layers
    in training mode and feeds them from a backbone on running statistics, so its noise is a subset of the full step's.  The test prints
    every tensor's figure before it asserts; `python tools/grad_direction.py --freeze-backbone --bn-eval 8` measures the same (LAB_NOTES.md §10)."""
    ref = procedural.fill_state_dict_(net_ref.RefYolo(procedural.VOC_CONFIG)).train()
    m = _model()
    for net in (ref, m):
        _freeze(net, bn_eval=True)
    x, tg = _batch()
    before = {k: b.clone() for k, b in m.named_buffers()}
    rr = ref(x, tg)
    (rr[0][0] + rr[1][0]).backward()
    res = m(x.cuda(), tg)
    (res[0][0] + res[1][0]).backward()
    for i in range(2):
        np.testing.assert_allclose(np.array([float(v) for v in res[i]]), np.array([float(v) for v in rr[i]]), rtol=2e-3, atol=1e-5)
    n_cmp, worst = _assert_gradient_tensors_close(m, ref, 8e-2)
    print("worst tensor", worst)
    assert n_cmp == 202 - sum(k.startswith("backbone.") for k, _ in m.named_parameters())
    rb = dict(ref.named_buffers())
    moved = 0
    for k, b in m.named_buffers():
        if k.startswith("backbone."):
            assert torch.equal(b, before[k]), k                              # statistics and num_batches_tracked bit-unchanged
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(rb[k]), k
            moved += int(b) == 1
        else:
            assert not torch.equal(b, before[k]) or torch.equal(rb[k], before[k].cpu()), k
            np.testing.assert_allclose(b.cpu().numpy(), rb[k].numpy(), rtol=2e-3, atol=2e-5, err_msg=k)
    assert moved >= 14                                                       # the 14 neck / head BatchNorms a VOC loss depends on, at least


# ---- 7: every BatchNorm in eval mode under model.train() ------------------------------------------------------------------------
def test_all_batchnorms_in_eval_mode_under_train_is_the_eval_mode_differentiable_path():
    x, tg = _batch()
    a = _model(train=False)
    want = _step(a, x.cuda(), tg)
    b = _model(train=True)
    for mod in b.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    assert b.training
    before = {k: v.clone() for k, v in b.named_buffers()}
    got = _step(b, x.cuda(), tg)
    assert got[0] == want[0]
    assert sorted(got[1]) == sorted(want[1]) and len(got[1]) == 202
    assert not [k for k in want[1] if not torch.equal(got[1][k], want[1][k])]
    assert all(torch.equal(v, before[k]) for k, v in b.named_buffers())


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def test_unsupported_batchnorm_mixes_are_refused_before_anything_runs():
    from mobilenet_yolo_pytorch_amd import MnyError, _lib
    x, tg = _batch()
    x = x.cuda()
    m = _model()
    m.connect_for_S32.conv[0].bn.eval()
    before = {k: v.clone() for k, v in m.named_buffers()}
    with pytest.raises(MnyError, match=r"connect_for_S32\.conv\.0\.bn"):
        m(x, tg)
    assert not m._plans
    assert all(torch.equal(v, before[k]) for k, v in m.named_buffers())      # no statistic, no num_batches_tracked moved
    # a fused pair (expand + depthwise: backbone.features.2) with split modes, both members below the frontier
    assert _lib.query("mny_exdw_supported", 8, 176, 176, 16, 96, 2) == 1
    m = _freeze(_model(), bn_eval=True)
    m.backbone.features[2].conv[1].train()
    before = {k: v.clone() for k, v in m.named_buffers()}
    with pytest.raises(MnyError, match=r"backbone\.features\.2\.conv\.4 is in eval mode.*backbone\.features\.2\.conv\.1"):
        m(x, tg)
    assert not m._plans
    assert all(torch.equal(v, before[k]) for k, v in m.named_buffers())
    m.backbone.features[2].conv[1].eval()
    res = m(x, tg)                                                           # ... and the supported combination runs
    (res[0][0] + res[1][0]).backward()
    assert m.backbone.features[2].conv[0].weight.grad is None and m.yolo_headS16[3].weight.grad is not None


# ---- 9: unfreezing and freezing again mid-run -----------------------------------------------------------------------------------
def test_unfreezing_mid_run_builds_the_right_plans_and_keeps_the_step_counters(full_step):
    from mobilenet_yolo_pytorch_amd import optim
    x, tg = _batch()
    x = x.cuda()
    runs = {}
    for name, make in (("fused", lambda ps: optim.AdamW(ps, lr=0.0, weight_decay=0.0)), ("torch", lambda ps: torch.optim.AdamW(ps, lr=0.0, weight_decay=0.0))):
        m = _model()
        opt = make(m.parameters())                       # lr 0: the parameters stay put, so step 2 can be compared with a fresh model's
        _freeze(m)
        g1 = _step(m, x, tg)
        opt.step()
        for p in m.parameters():
            p.requires_grad_(True)
        g2 = _step(m, x, tg)
        opt.step()
        _freeze(m)
        g3 = _step(m, x, tg)
        opt.step()
        torch.cuda.synchronize()
        assert len(g2[1]) == 202 and not [k for k in g2[1] if not torch.equal(g2[1][k], full_step[1][k])]
        assert sorted(g1[1]) == sorted(g3[1]) and not [k for k in g1[1] if k.startswith("backbone.")]
        assert not [k for k in g1[1] if not torch.equal(g1[1][k], full_step[1][k])]
        assert not [k for k in g3[1] if not torch.equal(g3[1][k], full_step[1][k])]
        sd = opt.state_dict()["state"]
        names = [k for k, _ in m.named_parameters()]
        runs[name] = {names[i]: float(st["step"]) for i, st in sd.items()}
    assert runs["fused"] == runs["torch"]
    assert set(runs["fused"].values()) == {1.0, 3.0}
    assert all(v == 1.0 for k, v in runs["fused"].items() if k.startswith("backbone.")) and runs["fused"]["yolo_headS16.3.weight"] == 3.0


# ---- 10: other configurations ---------------------------------------------------------------------------------------------------
def test_mbv3_bf16_frozen_backbone_equals_the_full_plan_bit_for_bit():
    from mobilenet_yolo_pytorch_amd import mbv3
    x, tg = procedural.images(2, 256, 256, seed=7).cuda(), procedural.targets(2, seed=8, empty_every=0)

    def make():
        torch.manual_seed(0)
        return procedural.fill_state_dict_(mbv3.yolo(procedural.VOC_CONFIG, sync_metrics=True, act_dtype=torch.bfloat16)).cuda().train()
    full = _step(make(), x, tg)
    m = _freeze(make())
    got = _step(m, x, tg)
    trainable = [k for k in full[1] if not k.startswith("backbone.")]
    assert len(trainable) > 40
    _assert_bit_equal_to_full(got, full, trainable, "mbv3 bf16")
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("backbone."))


def test_bdd_seg_frozen_backbone_equals_the_full_plan_bit_for_bit():
    from mobilenet_yolo_pytorch_amd import yolo
    cfg = json.load(open(os.path.join(G, "state_keys_bdd100k.json")))["config"]

    def make():
        torch.manual_seed(0)
        return procedural.fill_state_dict_(yolo(cfg, sync_metrics=True)).cuda().train()
    x = procedural.images(4, 352, 352, seed=31).cuda()
    tg = procedural.targets(4, num_classes=cfg["yolo"]["num_classes"], seed=8, empty_every=3)
    r = np.random.RandomState(4)
    sm = torch.from_numpy((r.rand(4, 22, 22, 2) * (r.rand(4, 22, 22, 2) > 0.5)).astype(np.float32)).cuda()
    full = _step(make(), x, tg, sm)
    m = _freeze(make())
    got = _step(m, x, tg, sm)
    trainable = [k for k in full[1] if not k.startswith("backbone.")]
    assert any(k.startswith("seg_") for k in trainable)
    _assert_bit_equal_to_full(got, full, trainable, "bdd")
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("backbone."))


def test_nothing_trainable_returns_losses_without_a_graph(full_step):
    m = _model()
    for p in m.parameters():
        p.requires_grad_(False)
    x, tg = _batch()
    res = m(x.cuda(), tg)
    assert not res[0][0].requires_grad and _losses(res) == full_step[0]
    assert all(p.grad is None for p in m.parameters())
    assert all(torch.equal(b, full_step[2][k]) for k, b in m.named_buffers())            # the statistics still move, like torch's


def test_frozen_backbone_in_eval_mode_runs_under_no_grad_on_a_forward_only_plan():
    """model.train(), backbone.eval(), torch.no_grad(): no gradient path, so no BatchNorm mode to refuse and no backward list or arena;
    the losses are the grad-enabled frozen step's, the backbone's buffers stay and the neck / head statistics move once."""
    x, tg = _batch()
    x = x.cuda()
    a = _freeze(_model(), bn_eval=True)
    want = _step(a, x, tg)
    m = _freeze(_model(), bn_eval=True)
    before = {k: b.clone() for k, b in m.named_buffers()}
    with torch.no_grad():
        res = m(x, tg)
    torch.cuda.synchronize()
    assert not res[0][0].requires_grad and _losses(res) == want[0]
    assert len(m._plans) == 1 and all(p.bwd is None and not hasattr(p, "gflat") for p in m._plans.values())
    assert all(p.grad is None for p in m.parameters())
    for k, b in m.named_buffers():
        assert torch.equal(b, want[2][k]), k                                 # the grad-enabled step's buffers, bit for bit
        if k.startswith("backbone."):
            assert torch.equal(b, before[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(before[k]) + 1, k
    # not even the frozen flags are needed for it: every parameter trainable, grad mode off
    m = _model()
    m.backbone.eval()
    with torch.no_grad():
        res = m(x, tg)
    assert _losses(res) == want[0] and all(p.bwd is None for p in m._plans.values())
    # a refusal that does hold without a gradient path (split modes inside a fused forward unit) still moves nothing
    m.backbone.features[2].conv[1].train()
    before = {k: b.clone() for k, b in m.named_buffers()}
    from mobilenet_yolo_pytorch_amd import MnyError
    with torch.no_grad(), pytest.raises(MnyError, match=r"backbone\.features\.2\.conv\.4 is in eval mode"):
        m(x, tg)
    assert all(torch.equal(b, before[k]) for k, b in m.named_buffers())


# ---- 11: the clip kernel through the C ABI --------------------------------------------------------------------------------------
# Launch 1 sums a block of 8192 floats (the header's clip block) with 256 threads: a thread's fp32 accumulator takes the squares of at most 8
# float4 of the 16-byte aligned body plus one scalar each of the block's head and tail (include/mnyolo.h states the same count, 34), each
# added with one rounding (fma); everything across threads and blocks is fp64.  A sum of n non-negative terms accumulated in fp32 is
# within n * 2^-24 relative of the exact one, so the sum of squares is within 34 * 2^-24; the square root halves that and the result's
# rounding to fp32 adds 2^-24: the norm stays inside 34 * 2^-24 relative with room to spare.
CLIP_REL = 34 * 2.0 ** -24


def _clip(segments, max_norm):
    """segments: [(flat fp32 device tensor viewed at an offset)] -> (total_norm, coef) as python floats via mny_grad_clip."""
    from mobilenet_yolo_pytorch_amd import _lib, optim
    host, nblocks = optim.clip_segment_table([(t.data_ptr(), t.numel()) for t in segments])
    assert nblocks == sum((t.numel() + 8191) // 8192 for t in segments)
    table = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    ws = torch.empty(nblocks, device="cuda", dtype=torch.float64)
    out = torch.full((2,), -1.0, device="cuda")
    _lib.call("mny_grad_clip", ctypes.c_void_p(table.data_ptr()), len(segments), nblocks, float(max_norm), ctypes.c_void_p(ws.data_ptr()),
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return float(out[0]), float(out[1]), out


def _arena(lengths, offsets, fill=1e30, seed=0):
    """One flat buffer holding the segments at the given misalignments (floats past a 16-byte boundary), 1e30 in every gap."""
    gen = torch.Generator().manual_seed(seed)
    pos, spans = 0, []
    for n, o in zip(lengths, offsets):
        pos = (pos + 3) // 4 * 4 + 8 + o                      # a gap of at least 8 floats of slack, then the misalignment
        spans.append((pos, n))
        pos += n
    flat = torch.full((pos + 16,), fill)
    for b, n in spans:
        flat[b:b + n] = torch.randn(n, generator=gen) * 0.37
    flat = flat.cuda()
    assert flat.data_ptr() % 16 == 0
    return flat, spans


CLIP_LENGTHS = [1, 3, 4, 5, 65535, 65536, 65537]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_grad_clip_kernel_on_hand_built_segment_tables(shift):
    offsets = [(shift + i) % 4 if shift else 0 for i in range(len(CLIP_LENGTHS))]
    if shift:
        offsets[4:] = [shift, shift, shift]                   # the three long segments at this misalignment
    flat, spans = _arena(CLIP_LENGTHS, offsets, seed=shift)
    orig = flat.clone()
    segs = [flat[b:b + n] for b, n in spans]
    assert [(s.data_ptr() // 4) % 4 for s in segs] == offsets
    exact = float(torch.sqrt(sum((s.double() ** 2).sum() for s in segs)))
    assert 50.0 < exact < 1e3                                 # the 1e30 slack between the segments is not part of it
    tn, coef, _ = _clip(segs, 1.0)
    print("shift %d: norm %.9g exact %.9g rel %.3e (bound %.3e) coef %.9g" % (shift, tn, exact, abs(tn - exact) / exact, CLIP_REL, coef))
    assert abs(tn - exact) <= CLIP_REL * exact
    want_coef = np.float32(1.0) / (np.float32(tn) + np.float32(1e-6))
    assert coef == float(want_coef) and coef < 1.0
    c32 = torch.tensor(coef, dtype=torch.float32, device="cuda")
    keep = torch.ones_like(flat, dtype=torch.bool)
    for (b, n), s in zip(spans, segs):
        assert torch.equal(s, orig[b:b + n] * c32), (b, n)    # fp32(g * coef), bit for bit
        keep[b:b + n] = False
    assert torch.equal(flat[keep], orig[keep])                # nothing outside the segments was touched
    # two runs are bit-identical
    flat2 = orig.clone()
    tn2, coef2, _ = _clip([flat2[b:b + n] for b, n in spans], 1.0)
    assert (tn2, coef2) == (tn, coef) and torch.equal(flat2, flat)
    # max_norm above the norm: coefficient 1, data bit-unchanged
    flat3 = orig.clone()
    tn3, coef3, _ = _clip([flat3[b:b + n] for b, n in spans], 2.0 * exact)
    assert tn3 == tn and coef3 == 1.0 and torch.equal(flat3, orig)


def test_grad_clip_kernel_zero_table_and_non_finite_norm():
    flat = torch.zeros(70000, device="cuda")
    segs = [flat[1:6], flat[8:65545], flat[65548:65551]]
    tn, coef, _ = _clip(segs, 1.0)
    assert tn == 0.0 and coef == 1.0 and not flat.any()
    flat = torch.ones(9000, device="cuda")
    flat[4321] = float("nan")
    tn, coef, _ = _clip([flat[:8999]], 1.0)
    assert np.isnan(tn) and np.isnan(coef)
    assert bool(torch.isnan(flat[:8999]).all()) and float(flat[8999]) == 1.0          # torch's default: the NaN propagates
    flat = torch.ones(100, device="cuda")
    flat[7] = float("inf")
    tn, coef, _ = _clip([flat], 1.0)
    assert np.isinf(tn) and coef == 0.0 and bool(torch.isnan(flat[7])) and float(flat[8]) == 0.0


# ---- 12: clip_grad_norm_ on a real step -----------------------------------------------------------------------------------------
def test_clip_grad_norm_on_a_frozen_backbone_step():
    from mobilenet_yolo_pytorch_amd import MnyError, optim
    x, tg = _batch()
    m = _freeze(_model())
    stale = torch.full_like(m.backbone.features[0][0].weight, 3.0)
    m.backbone.features[0][0].weight.grad = stale.clone()                   # a stale .grad from before freezing: left alone
    res = m(x.cuda(), tg)
    (res[0][0] + res[1][0]).backward()
    torch.cuda.synchronize()
    ps = [p for p in m.parameters() if p.requires_grad and p.grad is not None]
    orig = [p.grad.clone() for p in ps]
    assert len(ps) == 46                                                     # the neck and the two heads; the seg branch of a VOC config is loss-dead
    clipped = orig + [stale]                                                 # torch clips whatever has a .grad, the stale one included
    clones = [torch.nn.Parameter(torch.zeros_like(g)) for g in clipped]
    for c, g in zip(clones, clipped):
        c.grad = g.clone()
    want = float(torch.nn.utils.clip_grad_norm_(clones, 1.0))
    exact = float(torch.sqrt(sum((g.double() ** 2).sum() for g in clipped)))
    total = optim.clip_grad_norm_(m.parameters(), 1.0)
    assert total.dim() == 0 and total.is_cuda
    got = float(total)
    print("norm %.9g torch %.9g exact %.9g" % (got, want, exact))
    assert exact > 1.0                                                       # the clip is active
    assert abs(got - exact) <= CLIP_REL * exact and abs(got - want) <= CLIP_REL * exact
    coef = torch.tensor(np.float32(1.0) / (np.float32(got) + np.float32(1e-6)), device="cuda")
    views = next(iter(m._plans.values())).gviews
    for k, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            assert p.grad.data_ptr() == views[k].data_ptr(), k               # the arena views were scaled in place
    for p, g in zip(ps, orig):
        assert torch.equal(p.grad, g * coef)
    assert torch.equal(m.backbone.features[0][0].weight.grad, stale * coef)  # it has a .grad, so it is clipped like torch clips it
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("backbone.") and k != "backbone.features.0.0.weight")
    # foreign gradients (not arena views), a module argument, and the refusals
    m.backbone.features[0][0].weight.grad = None
    for p, g in zip(ps, orig):
        p.grad = g.clone()
    got2 = float(optim.clip_grad_norm_(m, 1.0))
    exact2 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in orig)))
    assert abs(got2 - exact2) <= CLIP_REL * exact2
    coef2 = torch.tensor(min(np.float32(1.0), np.float32(1.0) / (np.float32(got2) + np.float32(1e-6))), device="cuda")
    for p, g in zip(ps, orig):
        assert torch.equal(p.grad, g * coef2)
    lin = torch.nn.Linear(3, 2)
    lin.weight.grad = torch.ones(2, 3)
    with pytest.raises(MnyError, match="fp32 CUDA"):
        optim.clip_grad_norm_(lin.parameters(), 1.0)
    dbl = torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64))
    dbl.grad = torch.ones(4, device="cuda", dtype=torch.float64)
    with pytest.raises(MnyError, match="fp32 CUDA"):
        optim.clip_grad_norm_([dbl], 1.0)
