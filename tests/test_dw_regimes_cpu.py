"""CPU: the Python restatement of the depthwise launch geometry (tests/dw_regimes.py) agrees with the library's own part-count queries (host
functions: no GPU needed), the rows of its table are in the regime they claim, and the fp64 reference of tests/dw_trips_ref.py agrees with
F.conv2d(groups=C) and autograd."""
import ast
import os

import pytest
import torch
import torch.nn.functional as F

import dw_regimes as dr
import dw_trips_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def _regime(r):
    return dr.regime(r.op, r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16, r.red)


def _agree(lib, op, N, H, W, C, K, s, bf, red):
    g = dr.regime(op, N, H, W, C, K, s, bf, red)
    qs = dr.query_args(op, N, H, W, C, K, s, bf, red)
    for name, args in qs:
        assert lib.query(name, *args) == g.gx, (name, args, g)
    return len(qs)


def test_every_table_row_has_the_grid_the_library_reports(lib):
    names = set()
    for r in dr.TABLE:
        _agree(lib, r.op, r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16, r.red)
        names |= {q[0] for q in dr.query_args(r.op, r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16, r.red)}
    assert names == {"mny_dw_stat_parts", "mny_dw_stat_parts_x", "mny_dw_wgrad_parts", "mny_dw_bnbwd_parts", "mny_dw_bnbwd_parts_k",
                     "mny_dw_bnbwd_s2_parts", "mny_dw_bnbwd_s2k5_parts"}


def _parametrized(test_name):
    """(argnames, rows) of the parametrize decorator of a test of test_gpu_kernels.py"""
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_kernels.py")).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == test_name:
            for d in node.decorator_list:
                if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize":
                    return [n.strip() for n in ast.literal_eval(d.args[0]).split(",")], ast.literal_eval(d.args[1])
    raise KeyError(test_name)


# test of test_gpu_kernels.py -> the depthwise calls it makes with its (N, H, W, C, ...) rows
_EXISTING = {
    "test_dw_forward_backward": lambda p: [("fwd", p["K"], p["s"], False, False), ("bwd_data", p["K"], p["s"], False, False), ("bwd_weight", p["K"], p["s"], False, False)],
    "test_dw_forward_odd_shapes_and_views": lambda p: [("fwd", 3, p["s"], False, False)],
    "test_dw_forward_tile_form_bf16": lambda p: [("fwd", p["k"], 1, True, False)],
    "test_fused_dw_unit_backward": lambda p: [("bnbwd", p["k"], 1, p["dtype"] == "bf16", False)],
    "test_fused_dw_unit_backward_with_producer_bn_sums": lambda p: [("bnbwd", p["k"], 1, p["dtype"] == "bf16", False), ("bnbwd", p["k"], 1, p["dtype"] == "bf16", True)],
    "test_fused_dw_stride2_unit_backward": lambda p: [("bnbwd_s2", 3, 2, p["dtype"] == "bf16", False), ("bwd_data", 3, 2, p["dtype"] == "bf16", False),
                                                      ("bwd_weight", 3, 2, p["dtype"] == "bf16", False)],
    "test_fused_dw5_stride2_unit_backward": lambda p: [("bnbwd_s2k5", 5, 2, p["dtype"] == "bf16", False), ("bwd_data", 5, 2, p["dtype"] == "bf16", False),
                                                       ("bwd_weight", 5, 2, p["dtype"] == "bf16", False)],
}


def _existing_calls():
    for test, calls in _EXISTING.items():
        names, rows = _parametrized(test)
        for row in rows:
            p = dict(zip(names, row))
            for op, K, s, bf, red in calls(p):
                yield test, op, p["N"], p["H"], p["W"], p["C"], K, s, bf, red


def test_the_shapes_the_kernel_tests_already_use_agree_too_and_take_one_trip(lib):
    """The same agreement at every depthwise shape parametrized in test_gpu_kernels.py — and the reason for test_gpu_dw_trips.py: none of them
    has a workgroup take a second trip of its loop."""
    n = 0
    for test, op, N, H, W, C, K, s, bf, red in _existing_calls():
        n += _agree(lib, op, N, H, W, C, K, s, bf, red)
        assert dr.regime(op, N, H, W, C, K, s, bf, red).trips == 1, (test, op, N, H, W, C, K, s, bf, red)
    assert n > 100


def test_table_rows_are_in_the_regime_they_claim():
    assert len({r.id for r in dr.TABLE}) == len(dr.TABLE)
    for r in dr.TABLE:
        g = _regime(r)
        if r.kind == "trips":
            assert g.gx == g.cap, r.id
            assert g.units > 2 * g.units_per_trip and g.trips >= 3, (r.id, g)         # a third trip starts
            assert g.units % g.units_per_trip != 0 and g.ragged, (r.id, g)            # and the last one is ragged
        elif r.kind == "tall":
            assert g.form == "tile" and g.TH >= 2 * (r.K + 1) and g.units > g.gx and g.gx == g.cap, (r.id, g)
        else:
            assert r.kind == "small" and g.trips == 1 and g.gx <= 8, (r.id, g)
    by_kernel = {}
    for r in dr.TABLE:
        g = _regime(r)
        by_kernel.setdefault(g.kernel, []).append(g)
    assert sorted(by_kernel) == ["dw3_fwd_kernel", "dw5_fwd_kernel", "dw5_wgrad_kernel", "dw_bnbwd_s1k3_kernel", "dw_bnbwd_s2k3_kernel", "dw_bnbwd_s2k5_kernel",
                                 "dw_bwd_data_s2k3_kernel", "dw_bwd_data_s2k5_kernel", "dw_slide_kernel", "dwb_tile_kernel", "dwf_tile_kernel"]
    for kernel, gs in by_kernel.items():
        assert any(g.gx % 8 == 0 and g.trips >= 3 for g in gs), kernel + ": no row with the XCD renumbering on a multi-trip grid"
        assert any(g.gx % 8 != 0 for g in gs), kernel + ": no row without the XCD renumbering"
    tile = [(r, _regime(r)) for r in dr.TABLE if _regime(r).form == "tile"]
    for kernel in ("dwb_tile_kernel", "dwf_tile_kernel"):
        assert any(r.kind == "tall" for r, g in tile if g.kernel == kernel), kernel
        assert any(r.kind == "trips" and g.nWT > 1 and g.last_tile_w < g.PT * (2 if r.K == 5 else 1) and g.last_strip_h < g.TH for r, g in tile if g.kernel == kernel), kernel
    assert {g.CG for r, g in tile} >= {16, 18}


def test_what_the_docstring_of_the_stride2_5x5_test_says_about_its_largest_case():
    """40 x 64 x 64 x 72 on dw_bnbwd_s2k5: 36 channel pairs, 7 strips per workgroup, 366 workgroups' worth of strips (368 launched) under a cap of 768: one trip."""
    g = dr.regime("bnbwd_s2k5", 40, 64, 64, 72, 5, 2, True)
    assert (g.units, g.ppb, g.gx, g.cap, g.trips, g.TH) == (2560, 7, 368, 768, 1, 16)


@pytest.mark.parametrize("N,H,W,C,K,s", [(2, 5, 7, 8, 3, 1), (2, 6, 7, 8, 3, 2), (1, 7, 6, 4, 5, 1), (2, 7, 9, 4, 5, 2), (1, 1, 2, 4, 5, 2), (1, 2, 1, 4, 3, 1)])
def test_reference_is_conv2d_and_its_autograd(N, H, W, C, K, s):
    g = torch.Generator().manual_seed(N + 10 * H + 100 * K)
    a = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, K, K, generator=g, dtype=torch.float64)
    an = a.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wn = w.view(C, 1, K, K).clone().requires_grad_(True)
    y = F.conv2d(an, wn, None, s, K // 2, 1, C)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    dyh = dy.permute(0, 2, 3, 1).contiguous()
    assert ref.out_hw(H, W, K, s) == tuple(y.shape[2:])
    assert (ref.conv(a, w, s) - y.detach().permute(0, 2, 3, 1)).abs().max() < 1e-12
    assert (ref.conv_dx(dyh, w, s, H, W) - an.grad.permute(0, 2, 3, 1)).abs().max() < 1e-12
    assert (ref.conv_dw(a, dyh, K, s) - wn.grad.view(C, K, K)).abs().max() < 1e-12


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4])
def test_reference_activation_derivatives_are_autograd(code):
    z = (torch.arange(-40, 41, dtype=torch.float64) / 4 + 0.01).requires_grad_(True)
    ref.act(z, code).sum().backward()
    assert (ref.dact(z.detach(), code) - z.grad).abs().max() < 1e-12
