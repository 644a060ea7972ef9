"""MI355X: fused SGD (mny_sgd_step) against torch.optim.SGD, the weight EMA (mny_ema_update) against torch.lerp_, the shadow swap
(mny_swap_chunks), and ModelEMA.applied() on the real module: same plans, same pointers, weights restored bit for bit.

Tolerance of the fp32-against-fp32 comparisons, per tensor T: max|a - b| <= tol_T = max(3e-6 * max|ref_T|, 2 * err_T), where err_T is
torch's own fp32 error on T against the same recurrence in float64 (plain tensor ops below).  Both fp32 sides evaluate one formula and
differ only in FMA contraction, so the fused error must be of the size of torch's own; the factor 2 covers the spread of the maximum of
two independent rounding sequences; 3e-6 relative (norm-wise, so elements crossing zero do not dominate) is what test_gpu_optim.py uses
for the AdamW twin.  The fused result is held to the same bound against the float64 run, so a formula error common to both fp32 sides
cannot hide.  Worst measured ratio error / bound: see LAB_NOTES.md ("SGD, EMA and swap launches")."""
import contextlib
import copy
import ctypes

import pytest
import torch

from oracle import procedural

pytestmark = pytest.mark.gpu

SHAPES = [(32, 3, 3, 3), (96,), (75, 512, 1, 1), (1,), (7,), (300, 1000), (1280, 320, 1, 1)]      # test_gpu_optim._params: odd sizes, several chunks, a ragged last chunk
ODD = (41, 37)                                                                                   # + a view 3 floats into a larger buffer: the non-vec4 path
LATE = 3                                                                                         # the parameter that gets no gradient in the first two steps


def _values(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in SHAPES + [ODD]]


def _params(seed):
    """(parameters, the larger buffer behind the last one): the last parameter starts 12 bytes into its storage."""
    vals = _values(seed)
    n = vals[-1].numel()
    big = torch.full((n + 16,), 7.0, device="cuda")
    big[3:3 + n].copy_(vals[-1].reshape(-1))
    ps = [torch.nn.Parameter(v.cuda()) for v in vals[:-1]] + [torch.nn.Parameter(big[3:3 + n].view(ODD))]
    assert ps[-1].data_ptr() % 16 == 12 and ps[0].data_ptr() % 16 == 0
    return ps, big


def _twin(seed):
    return [torch.nn.Parameter(v.cuda()) for v in _values(seed)]


def _grads(gen, it, late=True):
    """one gradient per tensor (None for the late one in the first two steps); the third tensor's is scaled x10"""
    out = []
    for i, s in enumerate(SHAPES + [ODD]):
        gr = torch.randn(*s, generator=gen).cuda() * (10.0 if i == 2 else 1.0)
        out.append(None if (late and i == LATE and it < 2) else gr)
    return out


def _bound(ref32, ref64):
    return max(3e-6 * float(ref32.abs().max()), 2.0 * float((ref32.double() - ref64).abs().max()))


def _check(tag, got, ref32, ref64, worst):
    """got against torch's fp32 result and against the float64 run, both within tol_T; records the ratios"""
    tol = _bound(ref32, ref64)
    e32 = float((got.double() - ref32.double()).abs().max())
    e64 = float((got.double() - ref64).abs().max())
    worst[0] = max(worst[0], e32 / tol)
    worst[1] = max(worst[1], e64 / tol)
    assert e32 <= tol, (tag, "vs torch", e32, tol)
    assert e64 <= tol, (tag, "vs float64", e64, tol)


SETTINGS = [dict(), dict(momentum=0.9), dict(momentum=0.9, nesterov=True, weight_decay=5e-4), dict(momentum=0.9, dampening=0.1)]


@pytest.mark.parametrize("kw", SETTINGS, ids=["plain", "momentum", "nesterov_wd", "dampening"])
def test_fused_sgd_matches_torch_and_float64(kw):
    from mobilenet_yolo_pytorch_amd.optim import SGD
    (pa, big), pb = _params(0), _twin(0)
    p64 = [p.detach().double() for p in pb]
    b64 = [None] * len(p64)
    lr, mu, damp, wd, nest = 1e-2, kw.get("momentum", 0.0), kw.get("dampening", 0.0), kw.get("weight_decay", 0.0), kw.get("nesterov", False)
    oa, ob = SGD(pa, lr=lr, **kw), torch.optim.SGD(pb, lr=lr, **kw)
    gen = torch.Generator().manual_seed(1)
    worst = [0.0, 0.0]
    for it in range(6):
        for i, gr in enumerate(_grads(gen, it)):
            pa[i].grad = None if gr is None else gr.clone()
            pb[i].grad = None if gr is None else gr.clone()
            if gr is None:
                continue
            d = gr.double()                                     # torch.optim.SGD's recurrence in float64
            if wd != 0:
                d = d + wd * p64[i]
            if mu != 0:
                b64[i] = d.clone() if b64[i] is None else mu * b64[i] + (1 - damp) * d
                d = d + mu * b64[i] if nest else b64[i]
            p64[i] = p64[i] - lr * d
        oa.step(); ob.step()
        for i, (a, b) in enumerate(zip(pa, pb)):
            _check(("p", it, i), a.detach(), b.detach(), p64[i], worst)
            if mu != 0 and b64[i] is not None:
                _check(("buf", it, i), oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"], b64[i], worst)
            elif mu != 0:
                assert "momentum_buffer" not in oa.state[a] and "momentum_buffer" not in ob.state[b]      # no gradient yet: no state, like torch
    print("sgd %s: worst error / bound  vs torch %.3f  vs float64 %.3f" % (kw, worst[0], worst[1]))
    n = pa[-1].numel()
    assert torch.all(big[:3] == 7.0) and torch.all(big[3 + n:] == 7.0)                     # nothing next to the misaligned view moved
    if mu != 0:
        assert all(oa.state[p]["momentum_buffer"].shape == p.shape for p in pa)
    else:
        assert len(oa.state_dict()["state"]) == 0


def test_sgd_tables_are_cached_on_the_pointer_signature():
    from mobilenet_yolo_pytorch_amd.optim import SGD
    pa, _big = _params(4)
    opt = SGD(pa, lr=1e-2, momentum=0.9)
    gen = torch.Generator().manual_seed(5)
    grads = _grads(gen, 9)
    for p, g in zip(pa, grads):
        p.grad = g
    opt.step()                                                  # every parameter on its first step: one table
    assert [s["first"] for s in opt._tables[0][1]] == [1]
    opt.step()
    tabs = opt._tables[0][1]
    assert [s["first"] for s in tabs] == [0]
    opt.step()
    assert opt._tables[0][1] is tabs                            # same pointers: nothing rebuilt
    pa[1].grad = pa[1].grad.clone()                             # a gradient moved
    opt.step()
    assert opt._tables[0][1] is not tabs


def test_sgd_state_dict_round_trip_with_torch_sgd():
    """torch -> fused and fused -> torch, one more step after loading; the late parameter (no state in one checkpoint, a None buffer in
    the other, as older torch checkpoints carry) takes the first-step form while the others run on.  Bound: 3e-6 * max|ref| per tensor,
    the relative tolerance of the AdamW twin taken norm-wise (three steps of a few roundings each stay two orders below it)."""
    from mobilenet_yolo_pytorch_amd.optim import SGD
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True)
    (pa, _big), pb = _params(2), _twin(2)
    oa, ob = SGD(pa, **kw), torch.optim.SGD(pb, **kw)
    gen = torch.Generator().manual_seed(3)

    def step(it, late=True):
        for a, b, gr in zip(pa, pb, _grads(gen, it, late)):
            a.grad = None if gr is None else gr.clone()
            b.grad = None if gr is None else gr.clone()
        oa.step(); ob.step()

    step(0); step(1)
    sa, sb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    assert sorted(sa["state"]) == sorted(sb["state"]) and LATE not in sa["state"]
    assert sa["param_groups"] == sb["param_groups"]
    sb["state"][LATE] = {"momentum_buffer": None}
    oa.load_state_dict(sb)                                      # the two optimizers trade checkpoints
    ob.load_state_dict(sa)
    step(2)                                                     # running form, except LATE: first step on both sides
    step(3)
    for i, (a, b) in enumerate(zip(pa, pb)):
        for got, ref in ((a.detach(), b.detach()), (oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"])):
            err, tol = float((got - ref).abs().max()), 3e-6 * float(ref.abs().max())
            assert err <= tol, (i, err, tol)


class _Bag(torch.nn.Module):
    """the tensor set as a module: parameters, a float buffer and an integer buffer"""

    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)
        self.register_buffer("stat", torch.linspace(-1, 1, 13).cuda())
        self.register_buffer("count", torch.tensor(5).cuda())


@pytest.mark.parametrize("tau", [2000, None])
def test_ema_update_matches_lerp_and_resumes(tau):
    from mobilenet_yolo_pytorch_amd.optim import ModelEMA
    import math
    pa, big = _params(6)
    bag = _Bag(pa)
    ema = ModelEMA(bag, decay=0.9, tau=tau)
    sd0 = bag.state_dict(keep_vars=True)
    names = [k for k, v in sd0.items() if v.is_floating_point()]                  # the shadow's entries: state_dict order, floats only
    live = [sd0[k] for k in names]
    assert list(ema.state_dict()["shadow"]) == names and "stat" in names and "count" not in names and len(names) == len(pa) + 1
    s32 = [t.detach().clone() for t in live]
    s64 = [t.detach().double() for t in live]
    gen = torch.Generator().manual_seed(7)
    worst = [0.0, 0.0]
    for u in range(1, 9):
        with torch.no_grad():
            for t in live:
                t.add_(torch.randn(*t.shape, generator=gen).cuda() * 0.1)
        ema.update()
        d = 0.9 * (1.0 - math.exp(-u / tau)) if tau else 0.9
        for i, t in enumerate(live):
            s32[i].lerp_(t.detach(), 1.0 - d)
            s64[i] = s64[i] + (1.0 - d) * (t.detach().double() - s64[i])
        got = ema.state_dict()["shadow"]
        for i, nm in enumerate(names):
            _check((nm, u), got[nm], s32[i], s64[i], worst)
    print("ema tau=%s: worst error / bound  vs lerp_ %.3f  vs float64 %.3f" % (tau, worst[0], worst[1]))
    assert ema.updates == 8 and int(bag.count) == 5
    n = pa[-1].numel()
    assert torch.all(big[:3] == 7.0) and torch.all(big[3 + n:] == 7.0)
    # resume: a second EMA over a copy of the module, loaded from the checkpoint, continues bit for bit
    sd = copy.deepcopy(ema.state_dict())
    bag2 = _Bag([torch.nn.Parameter(p.detach().clone()) for p in pa])
    bag2.stat.copy_(bag.stat)
    ema2 = ModelEMA(bag2, decay=0.5, tau=7)
    ema2.load_state_dict(sd)
    assert (ema2.updates, ema2.decay, ema2.tau) == (8, 0.9, tau)
    ema.update(); ema2.update()
    a, b = ema.state_dict(), ema2.state_dict()
    assert a["updates"] == b["updates"] == 9
    for nm in names:
        assert torch.equal(a["shadow"][nm], b["shadow"][nm]), nm


def test_swap_chunks_exchanges_exactly_and_twice_is_the_identity():
    from mobilenet_yolo_pytorch_amd import _lib, optim
    pa, big = _params(8)
    flat = torch.randn(sum((p.numel() + 3) // 4 * 4 for p in pa) + 4, generator=torch.Generator().manual_seed(9)).cuda()
    rows, views, off = [], [], 0
    for p in pa:
        n = p.numel()
        views.append(flat[off:off + n])
        rows += optim._chunk_rows((p.data_ptr(), 0, views[-1].data_ptr(), 0), n, optim.STREAM_CHUNK)
        off += (n + 3) // 4 * 4
    assert any(r[5] == 0 for r in rows) and any(r[5] == 1 for r in rows)           # both the scalar and the float4 path
    assert any(r[4] % 4 for r in rows) and max(r[4] for r in rows) == optim.STREAM_CHUNK and len(rows) > len(pa)
    table = optim._device_table(rows, "cuda")
    p0, f0, b0 = [p.detach().clone() for p in pa], flat.clone(), big.clone()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("mny_swap_chunks", ctypes.c_void_p(table.data_ptr()), len(rows), st)
    off = 0
    for p, v, was in zip(pa, views, p0):
        n = p.numel()
        assert torch.equal(p.detach().reshape(-1), f0[off:off + n]) and torch.equal(v, was.reshape(-1))
        pad = (n + 3) // 4 * 4
        assert torch.equal(flat[off + n:off + pad], f0[off + n:off + pad])           # the padding between shadows is not touched
        off += pad
    n = pa[-1].numel()
    assert torch.equal(big[:3], b0[:3]) and torch.equal(big[3 + n:], b0[3 + n:])
    _lib.call("mny_swap_chunks", ctypes.c_void_p(table.data_ptr()), len(rows), st)
    assert torch.equal(flat, f0) and torch.equal(big, b0)
    assert all(torch.equal(p.detach(), was) for p, was in zip(pa, p0))


def _train_three(cls, act_dtype, n, size, enter, fill, val_conf):
    """Three SGD(+Nesterov) steps with ema.update(), an eval pass (inside ema.applied() when `enter`), one more training step.
    Returns what the tests look at.  `fill`: the oracle's procedural weights, else the constructor's own initialisation (seeded)."""
    from mobilenet_yolo_pytorch_amd.optim import SGD, ModelEMA
    torch.manual_seed(0)
    m = cls(procedural.VOC_CONFIG, act_dtype=act_dtype)
    if fill:
        procedural.fill_state_dict_(m)
    m = m.cuda().train()
    for hs in m.yolo_losses:
        hs.val_conf = val_conf
    x = procedural.images(n, size, size, seed=3).cuda()
    tg = procedural.targets(n, seed=4, empty_every=0)
    opt = SGD(m.parameters(), lr=1e-4, momentum=0.9, nesterov=True)
    ema = ModelEMA(m, decay=0.9, tau=None)

    def step():
        opt.zero_grad()
        res = m(x, tg)
        loss = res[0][0] + res[1][0]
        loss.backward()
        opt.step()
        return float(loss.detach())

    for _ in range(3):
        step()
        ema.update()
    m.eval()
    raw = m(x)                                                  # the eval plan exists from here on
    out = dict(model=m, ema=ema, x=x, tg=tg, raw=raw)
    out["plans_before"] = dict(m._plans)
    out["state_before"] = {k: v.clone() for k, v in m.state_dict().items()}
    out["shadow_before"] = ema.state_dict()["shadow"]
    out["shadow_sd"] = ema.shadow_state_dict()
    with (ema.applied() if enter else contextlib.nullcontext()):
        out["det"] = m(x)
        out["plans_inside"] = dict(m._plans)
        out["state_inside"] = {k: v.clone() for k, v in m.state_dict().items()}
    out["plans_after"] = dict(m._plans)
    out["state_after"] = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    out["next_loss"] = step()
    return out


def _check_applied(cls, act_dtype, n, size, fill, val_conf):
    r = _train_three(cls, act_dtype, n, size, True, fill, val_conf)
    # plans: the same objects before, inside and after — nothing was rebuilt
    for other in (r["plans_inside"], r["plans_after"]):
        assert set(other) == set(r["plans_before"]) and all(other[k] is r["plans_before"][k] for k in other)
    # inside the block the live tensors hold the shadow (BN running statistics included), integer buffers stay
    floats = list(r["shadow_before"])
    assert any("running_mean" in k for k in floats) and any("running_var" in k for k in floats)
    for k, v in r["state_inside"].items():
        assert torch.equal(v, r["shadow_before"][k] if k in r["shadow_before"] else r["state_before"][k]), k
    assert any(not torch.equal(r["state_inside"][k], r["state_before"][k]) for k in floats)
    # ... and the detections are those of a fresh module loaded with the shadow
    fresh = cls(procedural.VOC_CONFIG, act_dtype=act_dtype)
    fresh.load_state_dict(r["shadow_sd"])
    fresh = fresh.cuda().eval()
    for hs in fresh.yolo_losses:
        hs.val_conf = val_conf
    want = fresh(r["x"])
    assert len(want) == len(r["det"]) == n and sum(len(d) for d in want) > 0
    for a, b in zip(r["det"], want):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    # after the block every parameter and buffer is what it was
    for k, v in r["state_after"].items():
        assert torch.equal(v, r["state_before"][k]), k
    return r


def test_applied_on_the_real_module_keeps_plans_and_restores_weights():
    from mobilenet_yolo_pytorch_amd import MnyError, yolo
    r = _check_applied(yolo, torch.float32, 4, 160, True, 0.3)
    # a further training step equals that of a twin that never entered applied()
    twin = _train_three(yolo, torch.float32, 4, 160, False, True, 0.3)
    assert all(torch.equal(a, b) for a, b in zip(twin["det"], twin["raw"]))
    assert r["next_loss"] == twin["next_loss"], (r["next_loss"], twin["next_loss"])
    # guards
    m, ema = r["model"], r["ema"]
    with ema.applied():
        for what in (ema.update, ema.copy_to_model, lambda: ema.applied().__enter__()):
            with pytest.raises(MnyError, match="applied"):
                what()
    res = m(r["x"], r["tg"])                                    # a differentiable forward that still awaits its backward
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(MnyError, match="awaits its backward"):
        with ema.applied():
            pass
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    (res[0][0] + res[1][0]).backward()
    with ema.applied():                                         # settled: allowed again
        pass
    ema.copy_to_model()
    sd = m.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ema.state_dict()["shadow"].items())


def test_applied_on_bf16_storage():
    """the weight shadows (bf16 copies, gate cuts) are re-cut from the live tensors on every pass, so the swap reaches them too
    (MobileNetV3 at 8 x 160 x 160 like test_bf16_training_reduces_loss, and like it from the constructor's initialisation: under the
    procedural weights this network's eval-mode heads are not finite, and rows with NaN compare unequal to themselves)"""
    from mobilenet_yolo_pytorch_amd import mbv3
    _check_applied(mbv3.yolo, torch.bfloat16, 8, 160, False, 0.1)


def test_fused_sgd_on_the_model_gradient_arena():
    """Three steps on the same arena-view gradients (the seg-branch parameters have none) against torch.optim.SGD on detached copies
    and the float64 recurrence, with the bound of the module docstring; then the plan keeps working and the loss has fallen."""
    from mobilenet_yolo_pytorch_amd import yolo
    from mobilenet_yolo_pytorch_amd.optim import SGD
    torch.manual_seed(0)
    m = yolo(dict(procedural.VOC_CONFIG)).cuda().train()
    x = procedural.images(4, 160, 160, seed=3).cuda()
    tg = procedural.targets(4, seed=4, empty_every=0)
    res = m(x, tg)
    (res[0][0] + res[1][0]).backward()
    live = list(m.parameters())
    ref = [torch.nn.Parameter(p.detach().clone()) for p in live]
    for r, p in zip(ref, live):
        r.grad = None if p.grad is None else p.grad.detach().clone()
    lr, mu, wd = 1e-4, 0.9, 5e-4
    fused, stock = SGD(live, lr=lr, momentum=mu, weight_decay=wd), torch.optim.SGD(ref, lr=lr, momentum=mu, weight_decay=wd)
    p64 = [p.detach().double() for p in live]
    b64 = [None] * len(live)
    for _ in range(3):
        fused.step(); stock.step()
        for i, p in enumerate(live):
            if p.grad is None:
                continue
            d = p.grad.double() + wd * p64[i]
            b64[i] = d.clone() if b64[i] is None else mu * b64[i] + d
            p64[i] = p64[i] - lr * b64[i]
    worst, n_live = [0.0, 0.0], 0
    for i, (r, p) in enumerate(zip(ref, live)):
        if p.grad is None:
            assert torch.equal(p.detach(), r.detach()) and len(fused.state[p]) == 0
            continue
        n_live += 1
        _check(("p", i), p.detach(), r.detach(), p64[i], worst)
        _check(("buf", i), fused.state[p]["momentum_buffer"], stock.state[r]["momentum_buffer"], b64[i], worst)
    print("sgd on the arena: worst error / bound  vs torch %.3f  vs float64 %.3f" % (worst[0], worst[1]))
    assert n_live >= 200
    res2 = m(x, tg)
    l0, l1 = float((res[0][0] + res[1][0]).detach()), float((res2[0][0] + res2[1][0]).detach())
    print("loss %.6f -> %.6f" % (l0, l1))
    assert l1 < l0
