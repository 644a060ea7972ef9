"""Every instantiation of the three weight-gradient tile kernels behind mny_pw_wgrad / mny_pw_wgrad_bf16 (csrc/pwwgrad.hip: pw_wgrad_kernel,
pw_wgrad_dma_kernel, pw_wgrad_bf16_kernel — 113 compiled kernels) held to EQUALITY with an fp64 reference.

The older direct tests launch 45 of the 113 (tests/test_wgrad_regimes_cpu.py prints which), each at one or two row counts, on seeded normal data
against a bound relative to the result's global maximum.  Here every instantiation runs the ring's short prologues (one chunk, two chunks), one steady
trip, several splits with a last split of one row, and — where its plan has more than one workgroup per split — the plain 3-D grid and the XCD
order with dead workgroups; at channel counts ragged in K and N; behind every view of its template; with a bias gradient and as the deferred
combine.  tests/wgrad_regimes.py lists the rows and restates the plan; every test asserts its row's regime first, from the restatement and from
mny_pw_wgrad_kernel, and after the call that mny_pw_wgrad_last_kernel reports the predicted kernel.

The inputs of tests/wgrad_exact_ref.py make every product and every sum exact in fp32 (asserted on the CPU), so the fp64 sum of the partial rows, dw
and dbias are EQUAL to the reference whatever the order of summation, on the fp32 MFMA, the six-product form and the bf16 MFMA.  X and dY are the
first M rows of allocations 64 rows longer that hold 2^12 behind them; dw, dbias, the workspace (mny_pw_wgrad_ws_floats, and one more row) and the
partial rows of the deferred form (one more than counted) are pre-filled with NaN: exactly the counted rows are written.
"""
import ctypes
import time

import pytest
import torch

import wgrad_exact_ref as we
import wgrad_regimes as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def _ids(rows):
    return [pytest.param(r, id=r.id) for r in rows]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _host(t):
    return t.cpu().double()


def _same(got, want, what):
    """got, want [N, K]: equal, or the first bad (co, ci) and its 32 x 32 block"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)                                  # (a NaN left in `got` is unequal too)
    if bad.any():
        idx = bad.nonzero()
        first = idx[0].tolist()
        msg = "%s: %d of %d elements differ; first at %s: got %r, want %r" % (what, idx.shape[0], got.numel(), first, got[tuple(idx[0])].item(), want[tuple(idx[0])].item())
        if got.dim() == 2:
            co, ci = first[0] // 32 * 32, first[1] // 32 * 32
            blk = bad[co:co + 32, ci:ci + 32]
            msg += "; 32 x 32 block (co %d.., ci %d..): %d of %d differ, rows %s, columns %s; blocks with a difference: %s" % (
                co, ci, int(blk.sum()), blk.numel(), sorted(set((idx[:, 0] % 32).tolist()))[:8], sorted(set((idx[:, 1] % 32).tolist()))[:8],
                sorted({(int(a) // 32, int(b) // 32) for a, b in idx.tolist()})[:12])
        raise AssertionError(msg)


def _regime(lib, row):
    r, g = wr.check_regime(row)
    act, view = wr.VIEWS[row.view]
    assert lib.query("mny_pw_wgrad_kernel", row.bf16, row.M, row.K, row.N, act, int(view), int(row.bias)) == r.code, row.id
    assert lib.query("mny_pw_wgrad_kernel", row.bf16, row.M, row.K, row.N, act, int(view), 0) == r.code, row.id
    assert lib.query("mny_pw_wgrad_splits" + ("_bf16" if row.bf16 else ""), row.M, row.K, row.N) == g.splits, row.id
    return r, g


class _Call:
    """the device buffers of one table row and one input class; run() launches the direct or the deferred form"""

    def __init__(self, lib, row, r, g, c):
        self.lib, self.row, self.r, self.g = lib, row, r, g
        self.act = c["act"]
        self.X = we.padded(c["X"], row.bf16).cuda()            # (the allocation: the call reads its first M rows)
        self.dY = we.padded(c["dY"], row.bf16).cuda()
        self.scale = None if c["scale"] is None else c["scale"].float().cuda()
        self.shift = None if c["shift"] is None else c["shift"].float().cuda()
        self.fn = "mny_pw_wgrad_bf16" if row.bf16 else "mny_pw_wgrad"
        self.n = row.N * row.K

    def run(self, deferred, bias):
        row, g = self.row, self.g
        if deferred:
            ws, dw, db = _nan((g.splits + 1) * self.n), None, None
        else:
            floats = int(self.lib.query("mny_pw_wgrad_ws_floats", row.M, row.K, row.N))
            assert floats >= g.splits * self.n + (min(wr.cdiv(row.M, 256), 512) * row.N if bias else 0)
            ws, dw, db = _nan(floats + self.n), _nan(row.N, row.K), (_nan(row.N) if bias else None)
        self.lib.call(self.fn, _p(self.X), _p(self.scale), _p(self.shift), self.act, _p(self.dY), _p(dw), _p(db), _p(ws), row.M, row.K, row.N, _st())
        assert self.lib.query("mny_pw_wgrad_last_kernel") == self.r.code and self.lib.query("mny_pw_last_route") == self.r.family, row.id
        return ws, dw, db

    def partial_sum(self, ws, bias, what):
        """exactly the counted partial rows are written (and, behind them, the column sums of a bias gradient): their fp64 sum"""
        g, h = self.g, _host(ws)
        rows = h[:g.splits * self.n].view(g.splits, self.n)
        assert not torch.isnan(rows).any(), what + ": a counted partial row was not (wholly) written"
        rest = h[g.splits * self.n:]
        if bias:
            rest = rest[min(wr.cdiv(self.row.M, 256), 512) * self.row.N:]
        assert rest.numel() >= self.n and torch.isnan(rest).all(), what + ": the workspace was written past the counted rows"
        return rows.sum(0).view(self.row.N, self.row.K)


def _kinds(row):
    """the 16-bit input classes run without a view: only where that call launches the row's own instantiation"""
    if row.bf16 or row.view == "leaky" or wr.route(0, row.M, row.K, row.N).inst != row.inst:
        return ["small"]
    return ["small", "wide16", "wide16-swapped"]


@pytest.mark.parametrize("row", _ids(wr.EXACT_TABLE))
def test_weight_gradient_is_exact(lib, row):
    t0 = time.time()
    r, g = _regime(lib, row)
    runs = []
    for kind in _kinds(row):
        c = we.case(row, kind)
        want = we.ref(c)
        rr = r if kind == "small" else wr.route(0, row.M, row.K, row.N)
        call = _Call(lib, row, rr, g, c)
        if kind == "small":
            runs.append((kind, call, want, call.run(False, row.bias), call.run(True, False)))
        else:
            runs.append((kind, call, want, call.run(False, False), None))
    torch.cuda.synchronize()
    t1 = time.time()
    for kind, call, want, (ws, dw, db), deferred in runs:
        bias = row.bias and kind == "small"
        _same(call.partial_sum(ws, bias, kind), want["dw"], "%s: fp64 sum of the partial rows (%s inputs)" % (row.id, kind))
        _same(_host(dw), we.f32(want["dw"]), "%s: dW (%s inputs)" % (row.id, kind))
        if bias:
            _same(_host(db), we.f32(want["dbias"]), "%s: dbias" % row.id)
        if deferred is not None:
            _same(call.partial_sum(deferred[0], False, "deferred"), want["dw"], "%s: fp64 sum of the partial rows, deferred combine (dw == NULL)" % row.id)
    print("%s: %s, %d splits x %s chunks of %d rows (last chunk %d rows, last split %d rows), grid %d x %d%s, %d workgroups: equal (%s); GPU %.2f s, total %.2f s" % (
        row.id, wr.inst_name(row.inst), g.splits, g.total, g.kc, g.last_rows[-1], g.last_split_rows, r.plan.gx, r.plan.gy,
        " in XCD order, %d dead" % g.dead if g.xcd else "", g.blocks, ", ".join(k for k, *_ in runs), t1 - t0, time.time() - t0))


@pytest.mark.parametrize("row", _ids(wr.LEAKY_TABLE))
def test_leaky_view_shares_the_clamp_path(lib, row):
    """0.1f z is not exact: the tolerances of tests/test_gpu_kernels.py (fp32: 2e-4 + 2e-4 |ref| per element) and tests/test_gpu_bf16.py (3e-4 max(1,
    max|ref|) + 3e-4 |ref|, against the activated operand rounded to bf16 where the LDS-DMA kernel rounds it)"""
    r, g = _regime(lib, row)
    c = we.case(row)
    ref = we.leaky_ref(c)
    a = we.bf(ref["a"]) if r.inst.template == wr.T_BF16 else ref["a"]
    want = c["dY"].t() @ a
    call = _Call(lib, row, r, g, c)
    ws, dw, db = call.run(False, row.bias)
    wsd, _, _ = call.run(True, False)
    torch.cuda.synchronize()
    tol = (3e-4 * max(1.0, float(want.abs().max())) + 3e-4 * want.abs()) if row.bf16 else (2e-4 + 2e-4 * want.abs())
    for what, got in (("dW", _host(dw)), ("partial rows", call.partial_sum(ws, row.bias, "direct")), ("deferred partial rows", call.partial_sum(wsd, False, "deferred"))):
        err = (got - want).abs()
        print("%s %s: max err %.3e, tolerance there %.3e, max|ref| %.3e" % (row.id, what, float(err.max()), float(tol.flatten()[err.argmax()]), float(want.abs().max())))
        assert bool((err <= tol).all()), (row.id, what)
    if row.bias:
        _same(_host(db), we.f32(ref["dbias"]), "%s: dbias" % row.id)
