"""CPU: the Python restatement of the gate / bf16 project launch geometry (tests/gate_regimes.py) agrees with the library's own part-count queries
(host functions: no GPU needed); the rows of its table are in the regime they claim; the existing kernel tests never ran those regimes; the fp64
reference of tests/gate_exact_ref.py agrees with torch autograd; its exact inputs keep every fp32 value exact and every partial sum below 2^24 units;
and the faults that tests/test_gpu_gate_exact.py exists for — stale LDS columns, an unmasked tail, a dropped trip, a zeroed padding-tile group — each
change an output of every row they apply to.  The last test measures what the 1e-2 * max bound of tests/test_gpu_gate.py sees of the first two on
that test's own data: less hides there than was assumed, see its docstring."""
import ast
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gate_exact_ref as ge
import gate_regimes as gr

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def _ids(rows):
    return [pytest.param(r, id=r.id) for r in rows]


# ---- the rows of the older tests ------------------------------------------------------------------------------------------------------------------------
def _lit(node):
    if isinstance(node, (ast.Tuple, ast.List)):
        return tuple(_lit(e) for e in node.elts)
    return eval(compile(ast.Expression(node), "<row>", "eval"), {"__builtins__": {}})      # constants and arithmetic on them (16 * 37 + 5)


def _parametrized(path, test_name, arg):
    """(argnames, rows) of the parametrize decorator of a test that carries the argument `arg`"""
    tree = ast.parse(open(os.path.join(HERE, path)).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == test_name:
            for d in node.decorator_list:
                if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize":
                    names = [n.strip() for n in ast.literal_eval(d.args[0]).split(",")]
                    if arg in names:
                        return names, _lit(d.args[1])
    raise KeyError(test_name)


# the rows this change added to the existing tests (exempt from the claims below: they are the first to leave the old regimes)
ADDED_GATE_M = {169, 32915}
ADDED_PJ = {(65683, 16, 16, 3), (65683, 64, 24, 1), (65683, 72, 40, 4)}


def _old_gate_m(with_added=False):
    ms = set()
    for test in ("test_gate_forward_matches_torch", "test_gate_backward_matches_autograd"):
        names, rows = _parametrized("test_gpu_gate.py", test, "M")
        got = {(row[names.index("M")] if isinstance(row, tuple) else row) for row in rows}
        assert ADDED_GATE_M <= got, (test, got)
        ms |= got
    return sorted(ms if with_added else ms - ADDED_GATE_M)


def _old_pj_rows(with_added=False):
    names, rows = _parametrized("test_gpu_pjbwd.py", "test_project_unit_backward_in_one_pass_bf16_storage", "M")
    assert names == ["M", "Ki", "No", "act"] and ADDED_PJ <= set(rows)
    return [r for r in rows if with_added or r not in ADDED_PJ]


def test_every_row_has_the_grid_the_library_reports(lib):
    names = set()
    for r in gr.TABLE:
        for name, args, want in gr.queries(r):
            assert lib.query(name, *args) == want, (r.id, name, args, want)
            names.add(name)
    assert names == {"mny_gate_parts", "mny_gate_bwd_parts", "mny_pj_bwd_parts_bf16"}
    for M in _old_gate_m(with_added=True) + [1, 15, 16, 17, 64, 65, 128, 129, 32768, 32769, 65536, 65537, 1 << 22]:
        assert lib.query("mny_gate_parts", M) == gr.gate_grid(M).gx and lib.query("mny_gate_bwd_parts", M) == gr.gate_bwd_grid(M).gx, M
    for (M, Ki, No, act) in _old_pj_rows(with_added=True):
        assert lib.query("mny_pj_bwd_parts_bf16", M, Ki, No) == gr.pj16_grid(M, Ki, No).gx, (M, Ki, No)
    for (C, R) in gr.GATE_SHAPES:
        assert lib.query("mny_gate_supported", 5, C, R) == 1
    for (Ki, No) in gr.PJ16_SHAPES:
        assert lib.query("mny_pj_bwd_supported_bf16", 16, Ki, No, gr.ACT_RELU) == 1 and lib.query("mny_pj_bwd_supported_bf16", 15, Ki, No, gr.ACT_RELU) == 0
        assert not gr.pj16_ok(15, Ki, No)
        with pytest.raises(lib.MnyError):
            lib.query("mny_pj_bwd_parts_bf16", 15, Ki, No)
    for r in gr.PJ_TABLE:
        assert lib.query("mny_pj_bwd_supported_bf16", r.M, r.Ki, r.No, r.act) == 1, r.id


def test_table_rows_are_in_the_regime_they_claim():
    assert len({r.id for r in gr.TABLE}) == len(gr.TABLE)
    for r in gr.TABLE:
        gr.check_regime(r)
    # gate: every M at every shape
    assert {(r.M, r.C, r.R) for r in gr.GATE_TABLE} == {(M, C, R) for M in (5, 169, 32915, 65557) for (C, R) in gr.GATE_SHAPES}
    # pj16: M = 16, 169, 65683 for all five instantiations; the third trip for the store from the accumulators and for the staged one
    pj = {(r.M, r.Ki, r.No) for r in gr.PJ_TABLE}
    assert pj == {(M, Ki, No) for M in (16, 169, 65683) for (Ki, No) in gr.PJ16_SHAPES} | {(131093, 16, 16), (131093, 72, 24)}
    assert not gr.pj16_flat(16) and gr.pj16_flat(72)
    for (Ki, No) in gr.PJ16_SHAPES:
        acts = {r.act for r in gr.PJ_TABLE if (r.Ki, r.No) == (Ki, No)}
        assert len(acts) >= 2 and gr.ACT_LEAKY not in acts, (Ki, No, acts)
    assert {r.act for r in gr.PJ_TABLE} == {gr.ACT_NONE, gr.ACT_RELU6, gr.ACT_RELU, gr.ACT_HSWISH}
    # the second trip of pj16 leaves workgroups that request rows past the last iteration
    g = gr.pj16_grid(65683, 16, 16)
    assert g.iters + g.gx - 1 - (g.iters - 1) % g.gx > g.iters


def test_the_older_tests_never_ran_these_regimes():
    ms = _old_gate_m()
    assert len(ms) >= 5 and min(ms) >= 16                              # no gate row below one full tile
    for M in ms:
        if M < 65557:
            assert not gr.gate_bwd_grid(M).stale_possible and gr.gate_grid(M).trips == 1, M
    rows = _old_pj_rows()
    assert len(rows) >= 10
    for (M, Ki, No, act) in rows:
        g = gr.pj16_grid(M, Ki, No)
        if M < 65557:
            assert not g.stale_possible, (M, Ki, No)
        if (Ki, No) in ((16, 16), (64, 24), (72, 40)):
            assert g.trips == 1, (M, Ki, No)                          # ... nor a request past the last iteration
    # the rows added with this table are the first to get there
    assert gr.gate_bwd_grid(32915).stale_possible
    for (M, Ki, No, act) in ADDED_PJ:
        assert gr.pj16_grid(M, Ki, No).stale_possible


def test_the_fp32_facts_the_recipe_rests_on():
    sixth, third = np.float32(1.0) / np.float32(6.0), np.float32(1.0) / np.float32(3.0)
    k = np.arange(-2001, 2002, 2, dtype=np.float32)
    assert ((np.float32(0.75) * k) * sixth == k / np.float32(8.0)).all()           # an odd multiple of 0.75 times fl(1 / 6): an odd eighth
    n = np.arange(-4096, 4097, dtype=np.float32)
    assert ((np.float32(6.0) * n) * sixth == n).all()
    assert np.float32(6.0) * sixth == np.float32(1.0)                              # the saturated gate is 1
    assert float(third) == (1.0 + 2.0 ** -25) / 3.0
    fma = lambda z: float(np.float32(np.float64(z) * np.float64(third) + 0.5))     # noqa: E731  (the fp64 expression is exact: one rounding)
    assert fma(-0.75) == 0.25 and fma(2.25) == 1.25 and fma(-2.25) == -(0.25 + 2.0 ** -25)


# ---- the reference against autograd ---------------------------------------------------------------------------------------------------------------------
def _bn_consts(x, gamma, beta):
    m, v = x.mean(0), x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(v + EPS)
    return m, invstd, gamma * invstd, beta - m * gamma * invstd


def _bn_coef(red, M, gamma, mean, invstd):
    """dx = ca dz + cb x + cc of a training-mode BatchNorm from its sums (sum dz, sum dz x_hat)"""
    s1, s2 = red[0], red[1]
    return torch.stack((gamma * invstd, -gamma * invstd ** 2 * s2 / M, -gamma * invstd * s1 / M + gamma * invstd ** 2 * mean * s2 / M))


def gate_case_with_batchnorm(y3, s3, b3, w1, w2, g1, be1, g2, be2, dout, round_grads=True):
    """a case dict whose constants are those of training-mode BatchNorm on the data itself: what mny_bn_finalize / mny_bn_bwd_finalize hand the passes"""
    M, C = y3.shape
    R = w1.shape[0]
    z = lambda n: torch.zeros(n, dtype=F64)  # noqa: E731
    c = dict(M=M, C=C, R=R, y3=y3, s3=s3, b3=b3, w1=w1, w2=w2, dout=dout, sc1=z(R), sh1=z(R), sc2=z(C), sh2=z(C), mean1=z(R), invstd1=z(R),
             mean2=z(C), invstd2=z(C), mean3=z(C), invstd3=z(C), coef1=torch.zeros(3, R, dtype=F64), coef2=torch.zeros(3, C, dtype=F64),
             add_x=torch.zeros(M, C, dtype=F64), add_scale=z(C), add_shift=z(C))
    c["mean1"], c["invstd1"], c["sc1"], c["sh1"] = _bn_consts(ge.gate_ref(c)[1]["hr"], g1, be1)
    c["mean2"], c["invstd2"], c["sc2"], c["sh2"] = _bn_consts(ge.gate_ref(c)[1]["g"], g2, be2)
    c["coef2"] = _bn_coef(ge.gate_ref(c, round_grads=round_grads)[0]["red2"], M, g2, c["mean2"], c["invstd2"])
    c["coef1"] = _bn_coef(ge.gate_ref(c, round_grads=round_grads)[0]["red1"], M, g1, c["mean1"], c["invstd1"])
    return c


def _st(v):
    """straight-through bf16 rounding"""
    return v + (v.detach().float().to(torch.bfloat16).to(F64) - v.detach())


@pytest.mark.parametrize("C,R", gr.GATE_SHAPES)
def test_gate_reference_agrees_with_autograd(C, R):
    M = 200
    g = torch.Generator().manual_seed(C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    y3, s3, b3 = rn(M, C) * 1.5 + 0.3, torch.rand(C, generator=g, dtype=F64) + 0.5, rn(C) * 0.4
    w1, w2 = rn(R, C) * (2.0 / C) ** 0.5, rn(C, R) * (2.0 / R) ** 0.5
    g1, be1, g2, be2 = torch.rand(R, generator=g, dtype=F64) + 0.5, rn(R) * 0.3, torch.rand(C, generator=g, dtype=F64) + 0.5, rn(C) * 0.8
    dout = rn(M, C) * 0.7
    c = gate_case_with_batchnorm(y3, s3, b3, w1, w2, g1, be1, g2, be2, dout, round_grads=False)
    out, mid, _, _ = ge.gate_ref(c, round_grads=False)
    t = (y3 * s3 + b3).requires_grad_(True)
    W1, W2, G1, B1, G2, B2 = (v.clone().requires_grad_(True) for v in (w1, w2, g1, be1, g2, be2))
    hr = _st(t) @ _st(W1).t()
    z1 = (hr - hr.mean(0)) / torch.sqrt(hr.var(0, unbiased=False) + EPS) * G1 + B1
    gg = _st(torch.relu(z1)) @ _st(W2).t()
    z2 = (gg - gg.mean(0)) / torch.sqrt(gg.var(0, unbiased=False) + EPS) * G2 + B2
    o = t * (torch.clamp(z2 + 3.0, 0.0, 6.0) / 6.0)
    o.backward(dout)
    assert ((z2.detach() > -3) & (z2.detach() < 3)).double().mean() > 0.3          # the case exercises the gate's slope
    # the reference rounds the gate, dO t / 6 and dO gate to fp32 (2^-24 each); everything else is fp64 on both sides
    for name, got, want in (("out", mid["out_f32:None"], o.detach()), ("dt", mid["dt32"], t.grad), ("dW1", out["dw1"], W1.grad), ("dW2", out["dw2"], W2.grad),
                            ("dbeta2", out["red2"][0], B2.grad), ("dgamma2", out["red2"][1], G2.grad), ("dbeta1", out["red1"][0], B1.grad),
                            ("dgamma1", out["red1"][1], G1.grad)):
        err = (got - want).abs().max().item()
        assert err <= 2e-6 * want.abs().max().item(), (name, err, want.abs().max().item())
    # the residual operand: scale, shift and activation
    c["add_x"], c["add_scale"], c["add_shift"] = rn(M, C), rn(C), rn(C)
    mid = ge.gate_ref(c)[1]
    a = c["add_x"] * c["add_scale"] + c["add_shift"]
    for kind, want in ((None, o.detach()), ("plain", o.detach() + c["add_x"]), ("view", o.detach() + a), ("view-relu", o.detach() + torch.relu(a))):
        assert (mid["out_f32:%s" % kind] - want).abs().max().item() <= 2e-6 * want.abs().max().item(), kind
    # red3: the BN-backward sums of the project unit over the stored gradient
    c["mean3"], c["invstd3"] = rn(C), torch.rand(C, generator=g, dtype=F64) + 0.5
    out = ge.gate_ref(c)[0]
    assert torch.equal(out["red3"][0], out["dt"].sum(0)) and torch.allclose(out["red3"][1], (out["dt"] * (y3 - c["mean3"]) * c["invstd3"]).sum(0), rtol=1e-12, atol=1e-12)
    assert torch.equal(out["dt"], ge.bf(out["dt"])) and torch.equal(out["st1"][0], mid["hr"].sum(0)) and torch.equal(out["st2"][1], (mid["g"] ** 2).sum(0))


@pytest.mark.parametrize("Ki,No", gr.PJ16_SHAPES)
@pytest.mark.parametrize("act", [gr.ACT_NONE, gr.ACT_RELU6, gr.ACT_RELU, gr.ACT_HSWISH])
def test_pj16_reference_agrees_with_autograd(Ki, No, act):
    M = 150
    g = torch.Generator().manual_seed(Ki + No + act)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    c = dict(M=M, Ki=Ki, No=No, act=act, G=rn(M, No), Y=rn(M, No), coef=torch.stack((rn(No), rn(No) * 0.1, rn(No) * 0.1)), W=rn(No, Ki) * Ki ** -0.5,
             D=rn(M, Ki) * 2.0, d_scale=torch.rand(Ki, generator=g, dtype=F64) + 0.5, d_shift=rn(Ki) * 0.5 + 1.0, d_mean=rn(Ki) * 0.2,
             d_invstd=torch.rand(Ki, generator=g, dtype=F64) + 0.5)
    out, mid, _, _ = ge.pj_ref(c)
    dYb = ge.bf(c["coef"][0] * c["G"] + c["coef"][1] * c["Y"] + c["coef"][2])
    D, W = c["D"].clone().requires_grad_(True), c["W"].clone().requires_grad_(True)
    z = D * c["d_scale"] + c["d_shift"]
    a = {gr.ACT_NONE: lambda v: v, gr.ACT_RELU6: F.relu6, gr.ACT_RELU: torch.relu, gr.ACT_HSWISH: F.hardswish}[act](z)
    a.retain_grad()
    (_st(a) @ _st(W).t()).backward(dYb)
    for name, got, want in (("gd", mid["gd32"], a.grad), ("dW", out["dw"], W.grad), ("dz", mid["gd32"] * mid["slope"], D.grad / c["d_scale"])):
        err = (got - want).abs().max().item()
        assert err <= 2e-6 * want.abs().max().item(), (name, err)
    assert torch.equal(out["gd"], ge.bf(mid["gd32"]))
    dz = ge.f32(out["gd"] * mid["slope"])                                         # over the STORED gradient
    assert torch.equal(out["red"][0], dz.sum(0)) and torch.allclose(out["red"][1], (dz * (c["D"] - c["d_mean"]) * c["d_invstd"]).sum(0), rtol=1e-12, atol=1e-12)


# ---- the exact rows ---------------------------------------------------------------------------------------------------------------------------------
def _fp32_exact(mid, what):
    for k, v in mid.items():
        assert torch.equal(v.to(torch.float32).to(F64), v), "%s: %s is not exact in fp32" % (what, k)


def _budget(terms, pixels, what):
    """(most pixels one workgroup accumulates) x (largest |term| in units of its accumulator) / 2^24, per reduced output; all must stay below 1"""
    use = {k: pixels * ge.worst_units(t) / 2.0 ** 24 for k, t in terms.items()}
    for k, u in use.items():
        assert u < 1.0, "%s: %s can reach %.2f of 2^24 units in one partial row" % (what, k, u)
    return use


def _differs(a, b):
    return bool((a != b).any())


def _head(c, n):
    """the first n pixels of a case"""
    return {k: (v[:n] if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == c["M"] else (n if k == "M" else v)) for k, v in c.items()}


@pytest.mark.parametrize("r", _ids(gr.GATE_TABLE))
def test_gate_row_is_exact_and_every_fault_shows(r):
    t0 = time.time()
    gs = gr.check_regime(r)
    gf, gb = gs["fwd"], gs["bwd"]
    c = ge.gate_case(r.M, r.C, r.R)
    out, mid, terms, reduce = ge.gate_ref(c)
    _fp32_exact(mid, r.id)
    _fp32_exact({k: v for k, v in c.items() if torch.is_tensor(v)}, r.id + " input")
    for k in ("y3", "dout", "add_x"):
        assert torch.equal(ge.bf(c[k]), c[k]), k                                  # stored as bf16
    assert torch.equal(ge.bf(c["w1"]), c["w1"]) and torch.equal(ge.bf(c["w2"]), c["w2"])
    # no pre-activation on a kink; both sides of ReLU and all three pieces of the hard sigmoid are populated
    z1, z2 = mid["z1"], mid["z2"]
    assert not (z1 == 0).any() and not (z2.abs() == 3).any()
    pos = (z1 > 0).double().mean().item()
    inside, lo, hi = ((z2 > -3) & (z2 < 3)).double().mean().item(), (z2 < -3).double().mean().item(), (z2 > 3).double().mean().item()
    assert 0.25 <= pos <= 0.75, (r.id, pos)
    assert inside >= 0.05 and lo >= 0.20 and hi >= 0.20, (r.id, inside, lo, hi)
    eighths = mid["gate"][(z2 > -3) & (z2 < 3)] * 8
    assert bool((eighths == eighths.round()).all() and (eighths % 2 == 1).all())
    # every partial row stays exact: forward sums by the forward grid, the rest by the backward grid
    use = _budget({k: terms[k] for k in ("st1", "st2")}, gf.max_pixels, r.id)
    use.update(_budget({k: terms[k] for k in ("red2", "red1", "red3", "dw2", "dw1")}, gb.max_pixels, r.id))
    for k in ("st1", "st2", "red2", "red1", "red3", "dw1", "dw2"):                # ... and so does their total, which the GPU test forms in fp64
        assert out[k].abs().max().item() < 2.0 ** 52
    # mutations
    reduced = ("st1", "st2", "red2", "red1", "red3", "dw2", "dw1")
    stale = gr.stale_pixels(gb)
    assert (stale.stop - stale.start == 16 * gb.last_idle) == gb.stale_possible
    if gb.stale_possible:
        d = reduce(stale)
        assert _differs(d["dw1"], torch.zeros_like(d["dw1"])) and _differs(d["dw2"], torch.zeros_like(d["dw2"])), r.id + ": stale columns would not show"
    if gb.last_pixels < 16:                                                   # (16 - last_pixels) more copies of pixel 0
        d = reduce(slice(0, 1))
        assert all(_differs(d[k], torch.zeros_like(d[k])) for k in ("st1", "st2", "red1", "red3", "dw2", "dw1")), r.id + ": an unmasked tail would not show"
        o = ge.gate_ref(_head(c, 1))[0]
        assert _differs(o["dt"], torch.zeros_like(o["dt"]))
    for g_, keys in ((gf, ("st1", "st2")), (gb, ("red2", "red1", "red3", "dw2", "dw1"))):
        if g_.trips >= 2:
            d = reduce(slice(gr.last_trip_start(g_), r.M))
            assert all(_differs(d[k], torch.zeros_like(d[k])) for k in keys), r.id + ": a dropped last trip would not show"
    grp = gr.padding_group(r.R)
    assert grp is not None and grp.stop == r.R
    n = min(r.M, 64)
    o0, o1 = ge.gate_ref(_head(c, n))[0], ge.gate_ref(_head(c, n), zero_hidden=grp)[0]
    assert _differs(o0["out:None"], o1["out:None"]) and _differs(o0["dt"], o1["dt"]) and _differs(o0["dw2"][:, grp], o1["dw2"][:, grp]), r.id + ": a zeroed padding group would not show"
    assert set(reduced) == set(terms)
    print("%s: interior %.3f, saturated low %.3f / high %.3f, z1 > 0 %.3f; |hr| <= %g, |g| <= %g, |dt| <= %g; largest partial row uses %.4f of 2^24; %.1f s"
          % (r.id, inside, lo, hi, pos, mid["hr"].abs().max().item(), mid["g"].abs().max().item(), mid["dt32"].abs().max().item(), max(use.values()), time.time() - t0))


@pytest.mark.parametrize("r", _ids(gr.PJ_TABLE))
def test_pj16_row_is_exact_and_every_fault_shows(r):
    t0 = time.time()
    g = gr.check_regime(r)["bwd"]
    c = ge.pj_case(r.M, r.Ki, r.No, r.act)
    out, mid, terms, reduce = ge.pj_ref(c)
    _fp32_exact(mid, r.id)
    _fp32_exact({k: v for k, v in c.items() if torch.is_tensor(v)}, r.id + " input")
    for k in ("G", "Y", "D", "W"):
        assert torch.equal(ge.bf(c[k]), c[k]), k
    assert torch.equal(ge.bf(mid["dY"]), mid["dY"]) and torch.equal(ge.bf(mid["a"]), mid["a"])       # the operands are exact in bf16 too
    z = mid["z"]
    if r.act in (gr.ACT_RELU, gr.ACT_RELU6):
        assert not (z == 0).any() and not (z == 6).any() and 0.25 <= (z > 0).double().mean().item() <= 0.9
    if r.act == gr.ACT_RELU6:
        assert (z > 6).double().mean().item() >= 0.05
    if r.act == gr.ACT_HSWISH:
        assert not (z.abs() == 3).any()
        mid_z = z[(z > -3) & (z < 3)]
        assert set(mid_z.unique().tolist()) == {-0.75, 2.25} and set(mid["slope"].unique().tolist()) == {0.0, 0.25, 1.0, 1.25}
        assert mid_z.numel() >= 0.05 * z.numel() and (z < -3).double().mean().item() >= 0.2 and (z > 3).double().mean().item() >= 0.2
    use = _budget(terms, g.max_pixels, r.id)
    assert out["dw"].abs().max().item() < 2.0 ** 52 * float(ge.unit_of(out["dw"].reshape(1, -1)).min())       # the fp64 combine of the rows is exact: dW is its one rounding to fp32
    stale = gr.stale_pixels(g)
    if g.stale_possible:
        assert stale.stop - stale.start == 16 * g.last_idle == 96
        assert _differs(reduce(stale)["dw"], torch.zeros_like(out["dw"])), r.id + ": stale columns would not show"
    if g.last_pixels < 16:
        d = reduce(slice(0, 1))
        assert _differs(d["dw"], torch.zeros_like(d["dw"])) and _differs(d["red"], torch.zeros_like(d["red"])), r.id + ": an unmasked tail would not show"
    if g.trips >= 2:
        d = reduce(slice(gr.last_trip_start(g), r.M))
        assert _differs(d["dw"], torch.zeros_like(d["dw"])) and _differs(d["red"][0], torch.zeros_like(d["red"][0])) and _differs(d["red"][1], torch.zeros_like(d["red"][1]))
    thin, wide = gr.padding_group(r.No), gr.padding_group(r.Ki)
    assert (thin is None) == (r.No == 16) and (wide is None) == (r.Ki in (16, 64))
    h = _head(c, 16)
    o0 = ge.pj_ref(h)[0]
    if thin is not None:
        assert _differs(o0["gd"], ge.pj_ref(h, zero_thin=thin)[0]["gd"]), r.id + ": a zeroed padding group of dY would not show"
    if wide is not None:
        hh = _head(c, min(r.M, 64))
        assert _differs(ge.pj_ref(hh)[0]["dw"][:, wide], ge.pj_ref(hh, zero_wide=wide)[0]["dw"][:, wide]), r.id + ": a zeroed padding group of a_d would not show"
    print("%s (act %d): |gd| <= %g, largest partial row uses %.4f of 2^24; %.1f s" % (r.id, r.act, mid["gd32"].abs().max().item(), max(use.values()), time.time() - t0))


# ---- what the older test's bound sees of these faults -----------------------------------------------------------------------------------------------
def test_what_the_older_bound_sees_of_stale_columns_and_an_unmasked_tail(lib):
    """tests/test_gpu_gate.py's own random case (make_case, C = 40, M = 65557, the seeds of test_gate_backward_matches_autograd) with the constants of
    training-mode BatchNorm, as mny_bn_finalize / mny_bn_bwd_finalize hand them over: dW1 / dW2 with the 96 stale columns of iteration 256 added once
    more, and with the 11 masked lanes of the last tile carrying pixel 0, against that test's 1e-2 * max|ref|.

    The expectation this file was asked to put on record — both faults stay inside the bound — does NOT hold for the stale columns.  A prototype at
    M = 4000 moved dW1 by 2-3 % of its maximum, and the estimate scaled that down in proportion to M.  But BatchNorm's backward makes dg and dhr
    orthogonal to the constant and to the normalised activations, so the weight gradients are sums of nearly centred terms: max|dW| grows like
    sqrt(M), not like M, and 96 pixels out of 65 557 still move dW1 by 4.1e-2 and dW2 by 8.5e-2 of the maximum (measured here) — four to eight times the
    bound.  The older test would fail on that fault at this size.  The unmasked tail moves dW1 by 3.5e-2 (seen) and dW2 by 3.5e-3 of the maximum: that
    one hides, at a third of the bound.  What the older bounds cannot see is therefore narrower than assumed: a fault of a few pixels in dW2, a wrong tile
    of small entries (every bound is relative to the global maximum), and the cases that test never runs; those are what tests/test_gpu_gate_exact.py
    adds.  The assertions below hold the measured relations, in both directions, so that this record stays true."""
    import test_gpu_gate as tg
    M, C, R = 32768 * 2 + 21, 40, 10
    names, rows = _parametrized("test_gpu_gate.py", "test_gate_backward_matches_autograd", "M")
    assert M in rows
    y3, s3, b3, w1, w2, g1, be1, g2, be2, add = tg.make_case(M, C, R, seed=3 * C + M, residual=None)
    dout = (torch.randn(M, C, generator=torch.Generator().manual_seed(C * 7 + M)) * 0.7).to(torch.bfloat16)
    d = lambda v: v.to(F64)  # noqa: E731
    c = gate_case_with_batchnorm(d(y3), d(s3), d(b3), d(w1), d(w2), d(g1), d(be1), d(g2), d(be2), d(dout))
    out, _, _, reduce = ge.gate_ref(c)
    g = gr.gate_bwd_grid(M)
    assert g.stale_possible and (g.last_live, g.last_idle, g.last_pixels) == (2, 6, 5)
    stale, tail = reduce(gr.stale_pixels(g)), reduce(slice(0, 1))
    ratio = {}
    for k in ("dw1", "dw2"):
        bound = 1e-2 * out[k].abs().max().item()
        for what, delta in (("stale", stale[k]), ("tail", (16 - g.last_pixels) * tail[k])):
            moved = delta.abs().max().item()
            ratio[k, what] = bound / moved
            print("%s, %s at M = %d: moves by %.3e = %.2e of max|ref|; the older bound is %.2f times that" % (k, what, M, moved, moved / out[k].abs().max().item(), bound / moved))
    assert ratio["dw2", "tail"] > 2.0                                           # hides
    assert ratio["dw1", "stale"] < 0.5 and ratio["dw2", "stale"] < 0.5 and ratio["dw1", "tail"] < 0.5      # would be seen
