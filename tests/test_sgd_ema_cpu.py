"""CPU: the argument checks of mny_sgd_step / mny_ema_update / mny_swap_chunks (they run before any launch), the constructor
validation of optim.SGD against torch.optim.SGD, ModelEMA's decay schedule against the formula in double, and the state-dict
layouts of both on CPU-constructed objects.  Whatever would launch a kernel on CPU tensors raises MnyError: there is no fallback."""
import copy
import ctypes
import math

import pytest
import torch


@pytest.fixture(scope="module")
def lib_path():
    import mobilenet_yolo_pytorch_amd.build as b
    return b.build()


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Conv2d(5, 7, 1, bias=False))


def test_argument_errors_do_not_need_a_gpu(lib_path):
    from mobilenet_yolo_pytorch_amd import _lib
    row = ctypes.create_string_buffer(40)                     # a non-null table: every check below fails before anything reads it
    t, null = ctypes.c_void_p(ctypes.addressof(row)), None
    with pytest.raises(_lib.MnyError, match="sgd_step: bad arguments"):
        _lib.call("mny_sgd_step", null, 1, 1e-2, 0.0, 0.0, 0.0, 0, 0, None)
    with pytest.raises(_lib.MnyError, match="sgd_step: bad arguments"):
        _lib.call("mny_sgd_step", t, 0, 1e-2, 0.0, 0.0, 0.0, 0, 0, None)
    for lr, mu, wd in ((-1e-2, 0.0, 0.0), (1e-2, -0.9, 0.0), (1e-2, 0.9, -5e-4), (float("nan"), 0.0, 0.0)):
        with pytest.raises(_lib.MnyError, match="must be >= 0"):
            _lib.call("mny_sgd_step", t, 1, lr, mu, 0.0, wd, 0, 0, None)
    for mu, damp in ((0.0, 0.0), (0.9, 0.1)):                 # torch's own ValueError
        with pytest.raises(_lib.MnyError, match="requires a momentum and zero dampening"):
            _lib.call("mny_sgd_step", t, 1, 1e-2, mu, damp, 0.0, 1, 0, None)
    with pytest.raises(_lib.MnyError, match="ema_update: bad arguments"):
        _lib.call("mny_ema_update", null, 1, 0.5, None)
    with pytest.raises(_lib.MnyError, match="ema_update: bad arguments"):
        _lib.call("mny_ema_update", t, -3, 0.5, None)
    for decay in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(_lib.MnyError, match=r"decay must be in \[0,1\]"):
            _lib.call("mny_ema_update", t, 1, decay, None)
    with pytest.raises(_lib.MnyError, match="swap_chunks: bad arguments"):
        _lib.call("mny_swap_chunks", null, 1, None)
    with pytest.raises(_lib.MnyError, match="swap_chunks: bad arguments"):
        _lib.call("mny_swap_chunks", t, 0, None)


def test_sgd_constructor_validation_matches_torch():
    from mobilenet_yolo_pytorch_amd import _lib
    from mobilenet_yolo_pytorch_amd.optim import SGD
    for kw in (dict(lr=-1e-2), dict(lr=1e-2, momentum=-0.5), dict(lr=1e-2, weight_decay=-1.0), dict(lr=1e-2, nesterov=True),
               dict(lr=1e-2, momentum=0.9, dampening=0.1, nesterov=True)):
        msgs = []
        for cls in (torch.optim.SGD, SGD):
            with pytest.raises(ValueError) as e:
                cls([torch.nn.Parameter(torch.zeros(3))], **kw)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], kw
    with pytest.raises(_lib.MnyError, match="maximize"):
        SGD([torch.nn.Parameter(torch.zeros(3))], lr=1e-2, maximize=True)


def test_sgd_state_dict_layout_and_no_cpu_fallback():
    from mobilenet_yolo_pytorch_amd import _lib
    from mobilenet_yolo_pytorch_amd.optim import SGD
    pa = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4, nesterov=True)
    ours, stock = SGD(pa, **kw), torch.optim.SGD(pb, **kw)
    assert ours.state_dict()["param_groups"] == stock.state_dict()["param_groups"]
    assert ours.state_dict()["state"] == {}
    for p in pb:
        p.grad = torch.ones_like(p)
    stock.step()
    ours.load_state_dict(copy.deepcopy(stock.state_dict()))                    # torch -> fused
    for a, b in zip(pa, pb):
        assert torch.equal(ours.state[a]["momentum_buffer"], stock.state[b]["momentum_buffer"])
    fresh = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in pa], lr=1.0)
    fresh.load_state_dict(copy.deepcopy(ours.state_dict()))                    # fused -> torch
    assert fresh.param_groups[0]["momentum"] == 0.9 and fresh.param_groups[0]["nesterov"] is True
    assert len(fresh.state_dict()["state"]) == 2
    for p in pa:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in pa]
    with pytest.raises(_lib.MnyError, match="no CPU fallback"):
        ours.step()
    assert all(torch.equal(a, b) for a, b in zip(pa, before))
    ours.param_groups[0]["maximize"] = True
    with pytest.raises(_lib.MnyError, match="maximize"):
        ours.step()


@pytest.mark.parametrize("tau", [2000, None])
def test_ema_decay_schedule(tau):
    from mobilenet_yolo_pytorch_amd.optim import ModelEMA
    ema = ModelEMA(_net(), decay=0.9998, tau=tau)
    for u in (1, 2, 10, 500, 2000, 20000, 10 ** 6):
        want = 0.9998 * (1.0 - math.exp(-u / 2000.0)) if tau else 0.9998
        assert ema.decay_at(u) == want
        assert 0.0 <= ema.decay_at(u) <= 0.9998
    if tau:
        assert ema.decay_at(1) < 1e-3 and abs(ema.decay_at(10 ** 6) - 0.9998) < 1e-15
    assert ModelEMA(_net(), decay=0.5, tau=0).decay_at(3) == 0.5
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ModelEMA(_net(), decay=bad)


def test_ema_layout_and_no_cpu_fallback():
    from mobilenet_yolo_pytorch_amd import _lib
    from mobilenet_yolo_pytorch_amd.optim import ModelEMA
    net = _net()
    net[1].running_mean.add_(0.25)
    net[1].num_batches_tracked.add_(7)
    ema = ModelEMA(net, decay=0.99, tau=100)
    sd = ema.state_dict()
    assert sorted(sd) == ["decay", "shadow", "tau", "updates"] and (sd["updates"], sd["decay"], sd["tau"]) == (0, 0.99, 100)
    floats = [k for k, v in net.state_dict().items() if v.is_floating_point()]
    assert list(sd["shadow"]) == floats and "1.running_mean" in floats and "1.num_batches_tracked" not in floats
    for k in floats:
        assert torch.equal(sd["shadow"][k], net.state_dict()[k]) and sd["shadow"][k].dtype == torch.float32
    with torch.no_grad():                                      # the live weights move on; the shadow is a copy, not a view
        for p in net.parameters():
            p.add_(1.0)
    ssd = ema.shadow_state_dict()
    assert list(ssd) == list(net.state_dict())
    assert int(ssd["1.num_batches_tracked"]) == 7             # integer entries: the model's, at call time
    assert not torch.equal(ssd["0.weight"], net.state_dict()["0.weight"]) and torch.equal(ssd["0.weight"], sd["shadow"]["0.weight"])
    twin = _net()
    twin.load_state_dict(ssd)
    # update / applied would launch: CPU tensors are refused, and nothing moved
    for what in (ema.update, lambda: ema.applied().__enter__()):
        with pytest.raises(_lib.MnyError, match="no CPU fallback"):
            what()
    assert ema.updates == 0
    # resume: counters and shadow come back exactly
    other = ModelEMA(_net(), decay=0.5, tau=None)
    sd["updates"] = 41
    other.load_state_dict(sd)
    assert (other.updates, other.decay, other.tau) == (41, 0.99, 100)
    for k in floats:
        assert torch.equal(other.state_dict()["shadow"][k], sd["shadow"][k])
    bad = dict(sd, shadow={k: v for k, v in list(sd["shadow"].items())[1:]})
    with pytest.raises(_lib.MnyError, match="do not match"):
        other.load_state_dict(bad)
    ema.copy_to_model()                                        # a plain copy, no kernel: the live weights become the average
    assert torch.equal(net.state_dict()["0.weight"], sd["shadow"]["0.weight"])
