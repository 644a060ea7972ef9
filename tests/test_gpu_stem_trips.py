"""The kernels at the two ends of a block — csrc/stem.hip, csrc/stemdw.hip and the fp32 csrc/pjbwd.hip — at odd image sizes and past the first trip of
their persistent loops.

With stride 2 and pad 1 an even size never reads the bottom or right zero padding; every stem-side shape of the older tests is even.  stemdw_bwd_kernel
(grid capped at 512) and pj_bwd_kernel (1024 / 512 workgroups of 64 pixels) never took a second trip there either, so the accumulators, the double
buffers, the prefetch and the XCD renumbering they carry across trips were never exercised, and stem_tile_kernel<T, 1> / <T, 2> and seven of the twelve
pj instantiations were never launched (tests/test_stem_regimes_cpu.py asserts all of that).  The rows of stem_regimes.TABLE close those gaps.  Every
test first asserts its row's regime from the restated geometry AND the library's own part-count query, so that a retuned cap cannot quietly turn it back
into a one-trip case.

The reference is the plain operation in fp64 on the CPU (tests/stem_trips_ref.py).  Two modes per row:

exact  inputs, taps and coefficients are small integers, invstd a power of two, pre-activations odd integers (never on a kink of ReLU / ReLU6), so every
       product and every partial sum is an integer below 2^24 (asserted on the reference on the CPU: sum |terms| < 2^24 per output, whatever the order)
       and every stored value has magnitude <= 256 (exact in bf16).  Outputs and partial rows are pre-filled with NaN, each partial-row buffer one row
       longer than the query says: exactly the counted rows are written, and every output is asserted EQUAL to the reference, element for element.
       A skipped, repeated or stale tile, or an accumulator reset between trips, cannot hide behind a tolerance.
real   seeded normal data with a non-zero mean on the image and the gradients (coherent sums), every activation the kernel accepts (leaky included,
       h-swish for mny_stem_bnwgrad), elements within 1e-3 of a kink moved off it.  Element-wise outputs at the tolerances of the older test of the same
       operation; reductions bounded by k 2^-24 sum |terms| per element, k derived from the accumulation order in each test's docstring
       (stem_trips_ref.stem_k / sd_k / pj_k).  tests/test_stem_regimes_cpu.py checks that dropping the last unit, or the last trip, moves a reduced
       output of every row by more than four times that bound.
"""
import ctypes
import time

import pytest
import torch

import stem_regimes as sr
import stem_trips_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
MODES = ["exact", "real"]


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


def _nan(*shape, bf=False):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device="cuda")


def _dev(t, bf=False):
    return t.to(torch.bfloat16 if bf else torch.float32).cuda().contiguous()


def _host(t):
    return t.cpu().double()


def _regime(lib, r):
    gs = sr.check_regime(r)
    for name, args, want in sr.queries(r):
        assert lib.query(name, *args) == want, (r.id, name, args, want)
    return gs


def _rows_written(buf, gx, what):
    """buf [gx + 1, ...] pre-filled with NaN: the gx counted rows are written, the extra one is not; returns the fp64 sum of the rows"""
    h = _host(buf)
    assert not torch.isnan(h[:gx]).any(), what + ": a counted partial row was not written"
    assert torch.isnan(h[gx]).all(), what + ": a row past the counted ones was written"
    return h[:gx].sum(0)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)                                  # (a NaN left in `got` is unequal too)
    if bad.any():
        idx = bad.nonzero()
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            what, idx.shape[0], got.numel(), idx[0].tolist(), got[tuple(idx[0])].item(), want[tuple(idx[0])].item()))


def _close(got, want, rtol, atol, what):
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    assert not torch.isnan(got).any(), what + ": NaN left in the output"
    assert (err <= tol).all(), "%s: max err %.3e (tol %.3e there), max|ref| %.3e" % (what, err.max().item(), tol.flatten()[err.argmax()].item(), want.abs().max().item())


def _bounded(got, want, terms, k, what):
    """|got - want| <= k 2^-24 sum|terms| per entry; prints the worst ratio to the bound"""
    bound = k * U * terms
    err = (got - want).abs()
    assert not torch.isnan(got).any(), what + ": NaN"
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print("%s: k = %d, worst |err| / (k 2^-24 sum|terms|) = %.3f" % (what, k, ratio))
    assert (err <= bound).all(), "%s: worst ratio %.3f of the bound (k = %d)" % (what, ratio, k)


def _timed(what, t0):
    print("%s: %.2f s" % (what, time.time() - t0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("r", _ids(sr.ST_TABLE))
def test_stem_forward_and_weight_gradients(lib, r, bf, mode):
    """mny_stem_fwd, mny_stem_wgrad and mny_stem_bnwgrad (fp32 and bf16 storage of y / dy / g) on stem_tile_kernel<T, 0 / 1 / 2>, stem_wgrad_mfma_kernel
    (Cout 16 / 32) and stem_kernel (Cout 12), at odd H and W and past the first trip.
    Real mode, y: 1e-4 relative + 1e-5 (test_stem); bf16: one rounding of the stored value, 2^-8 of the maximum.  The statistics are taken over the STORED
    output, so they are held against the fp64 sums of the kernel's own y (itself checked element-wise): a thread of the tile form adds one value per
    pixel pass, cgn = Cout / 4 passes per tile, to its accumulator over all its trips (sum y^2 by fma: one rounding per step too), then one thread adds
    the 256 / cgn accumulators of its channel group: k = trips cgn + 256 / cgn; stem_kernel: one pixel per trip, ppb = 256 / cgn (rounded down)
    accumulators: k = trips + ppb.  The rows are combined in fp64 here.
    Weight gradients, vector-ALU forms: the same chain with one fma per pixel (the product is exact inside the fma) and the same fold: the same k on
    sum |x| |dY|; dW itself is the library's fp64 combine of the rows rounded once (+ 1).  Matrix cores: a wave issues 16 instructions of 4 products per
    tile into one accumulator (at most 4 roundings each, whatever the order inside the instruction), over all trips, and the four waves are added in
    order: k = 64 trips + 4.  The fused form rebuilds dY = ca g act'(sc y + sh) + cb y + cc in fp32: z (1), act' (at most 2: h-swish's z / 3 + 1 / 2),
    g act' (1), the two fmas (2), the fp32 value of leaky's 0.1 / h-swish's 1 / 3 (1) — 7 more roundings relative to |ca g act'| + |cb y| + |cc|:
    k + 7 on sum |x| (|ca g act'| + |cb y| + |cc|).
    Worst measured ratio to the bound: 0.010 on the multi-trip rows (st-valu64, k = 48 .. 56), 0.048 on the one-trip ones (st-oddH1, k = 32 .. 40)."""
    t0 = time.time()
    gs = _regime(lib, r)
    N, H, W, C = r.N, r.H, r.W, r.Cout
    Ho, Wo = sr.out_hw(H, W)
    c = ref.stem_case(r, mode, bf)
    out, terms = ref.stem_ref(c)
    sfx = "_bf16" if bf else ""
    xd, wd = _dev(c["x"]), _dev(c["w"])
    gf = gs["fwd"]
    y, stats = _nan(N, Ho, Wo, C, bf=bf), _nan(gf.gx + 1, 2, C)
    lib.call("mny_stem_fwd" + sfx, _p(xd), _p(wd), _p(y), _p(stats), N, H, W, C, _st())
    gw = gs["wgrad"]
    dyd = _dev(c["dy"], bf)
    dw, ws = _nan(C, 3, 3, 3), _nan(gw.gx + 1, C * 27)
    lib.call("mny_stem_wgrad" + sfx, _p(xd), _p(dyd), _p(dw), _p(ws), N, H, W, C, _st())
    fused = "bnwgrad" in gs
    if fused:
        gd, yd, sc, sh, cf = _dev(c["g"], bf), _dev(c["yraw"], bf), _dev(c["scale"]), _dev(c["shift"]), _dev(c["coef"])
        dwb, wsb = _nan(C, 3, 3, 3), _nan(gs["bnwgrad"].gx + 1, C * 27)
        lib.call("mny_stem_bnwgrad" + sfx, _p(xd), _p(gd), _p(yd), _p(sc), _p(sh), c["act"], _p(cf), _p(dwb), _p(wsb), N, H, W, C, _st())
    torch.cuda.synchronize()
    got_y, st = _host(y), _rows_written(stats, gf.gx, "stem statistics")
    got_dw, rows = _host(dw), _rows_written(ws, gw.gx, "stem wgrad").view(C, 3, 3, 3)
    if fused:
        got_dwb, rowsb = _host(dwb), _rows_written(wsb, gs["bnwgrad"].gx, "stem bnwgrad").view(C, 3, 3, 3)
    if mode == "exact":
        _same(got_y, out["y"], "y")
        _same(st[0], out["s1"], "sum y")
        _same(st[1], out["s2"], "sum y^2")
        _same(rows, out["dw"], "dW partial rows")
        _same(got_dw, out["dw"], "dW")
        if fused:
            _same(rowsb, out["dwb"], "fused dW partial rows")
            _same(got_dwb, out["dwb"], "fused dW")
        _timed(r.id, t0)
        return
    if bf:
        _close(got_y, out["y"], 0.0, 2.0 ** -8 * out["y"].abs().max().item(), "y")
    else:
        _close(got_y, out["y"], 1e-4, 1e-5, "y")
    k = ref.stem_k(gf, "fwd")
    _bounded(st[0], got_y.sum((0, 1, 2)), got_y.abs().sum((0, 1, 2)), k, r.id + " sum y")
    _bounded(st[1], (got_y ** 2).sum((0, 1, 2)), (got_y ** 2).sum((0, 1, 2)), k, r.id + " sum y^2")
    k = ref.stem_k(gw, "wgrad")
    _bounded(rows, out["dw"], terms["dw"], k, r.id + " dW partial rows")
    _bounded(got_dw, out["dw"], terms["dw"], k + 1, r.id + " dW")
    if fused:
        k = ref.stem_k(gs["bnwgrad"], "bnwgrad")
        _bounded(rowsb, out["dwb"], terms["dwb"], k, r.id + " fused dW partial rows (act %d)" % c["act"])
        _bounded(got_dwb, out["dwb"], terms["dwb"], k + 1, r.id + " fused dW")
    _timed(r.id, t0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _ids(sr.SD_TABLE))
def test_stem_and_first_depthwise_backward(lib, r, mode):
    """mny_stemdw_bwd on independent inputs (gd, d, s, x and every coefficient vector are inputs of the kernel; it does not recompute s from x).
    Exact: the depthwise dW and its partial rows, and the five blocks [P1 | Gram | s1 | s2 | colsum] of the first gx rows of the workspace summed in
    fp64, are equal to the reference; the final dW_s, dgamma_s, dbeta_s go through pw_bnbwd_finalize_kernel's fp64 division by M and are held to 1e-6
    of the tensor's maximum (with exact sums the finalize is the only rounding).
    Real: a workgroup walks TH rows per tile and `trips` tiles.  Depthwise dW: a tap's accumulator takes one fma per row, TH + 1 of them per tile, then
    the 32 column slots are added in order; a term a dY carries 3 roundings of the activated view (z, the leaky product, fp32 0.1) and 5 of dY (z, g act', two
    fmas, fp32 0.1): k = trips (TH + 1) + 32 + 8 on sum |z_s| (|ca g act'| + |cb d| + |cc|).  s1: one addition per owned row, the 32 slots; dz_s carries the 5
    roundings of dY, the 9 fmas of the scatter and the mask product with its 0.1 (2): k = trips TH + 32 + 16 on sum over the taps of |w| (|ca g act'| + |cb d| + |cc|);
    s2: + 3 (s - mean, invstd, the fma) on the same times |s_hat|.  Matrix cores: per row and tile a wave issues two instructions of 4 products into
    an accumulator (at most 4 roundings each), then the four waves are added in order: k = 8 trips TH + 4, + 16 for P1 (dz_s), on sum |dz terms| |p|
    and sum |p_i p_j|; colsum: two additions per row and tile, two shuffles, the four waves: k = 2 trips TH + 6.  The final dW_s is held against the
    fp64 finalize of the kernel's own sums: the reduced row is the fp64 combine rounded to fp32 (1), the coefficients inherit that (1), the result is
    rounded (1): k = 4 on |ca P1| + |cb| |W| |Gram| + (|ca s1 / M| + |cb mean|) |colsum|; dgamma_s and dbeta_s are s2 and s1 rounded once (k = 1).
    Worst measured ratio of a sum: 0.007 on sd-trips / sd-strips (k up to 140 / 292), 0.078 on the smallest grids (colsum of sd-min-8x9, k = 14); dW_s
    0.41 of its k = 4; dgamma_s / dbeta_s up to 0.99 of the single rounding they are allowed."""
    t0 = time.time()
    g = _regime(lib, r)["bwd"]
    N, H, W, C = r.N, r.H, r.W, sr.SD_C
    c = ref.sd_case(r, mode)
    assert lib.query("mny_stemdw_supported", N, H, W, C, c["s_act"], c["d_act"]) == 1
    out, terms = ref.sd_ref(c)
    names = ("gd", "d", "d_scale", "d_shift", "d_coef", "s", "s_scale", "s_shift", "s_mean", "s_invstd", "s_gamma", "x", "w_stem", "w_dw")
    t = {n: _dev(c[n]) for n in names}
    nws = int(lib.query("mny_stemdw_bwd_ws_floats", N, H, W, C))
    stride = sr.SD_STRIDE
    ws = _nan(nws + stride)
    dwws = _nan(g.gx + 1, C * 9)
    dws, dgs, dbs, dwd = _nan(C, 27), _nan(C), _nan(C), _nan(C, 3, 3)
    lib.call("mny_stemdw_bwd", _p(t["gd"]), _p(t["d"]), _p(t["d_scale"]), _p(t["d_shift"]), c["d_act"], _p(t["d_coef"]), _p(t["s"]), _p(t["s_scale"]),
             _p(t["s_shift"]), _p(t["s_mean"]), _p(t["s_invstd"]), _p(t["s_gamma"]), c["s_act"], _p(t["x"]), _p(t["w_stem"]), _p(t["w_dw"]),
             _p(dws), _p(dgs), _p(dbs), _p(dwd), _p(dwws), _p(ws), N, H, W, C, _st())
    torch.cuda.synchronize()
    rows_dw = _rows_written(dwws, g.gx, "depthwise dW").view(C, 3, 3)
    wsh = _host(ws)
    assert torch.isnan(wsh[nws:]).all(), "the workspace was written past the size the library asks for"
    parts = wsh[: g.gx * stride].view(g.gx, stride)
    assert not torch.isnan(parts).any(), "a counted partial row of the workspace was not written"
    idle = [b for b in range(g.gx) if sr.sd_first_tile(b, g.gx) >= g.units]
    assert len(idle) == max(g.gx - g.units, 0)
    if idle:                                              # workgroups without a tile write zero rows
        assert (parts[idle] == 0).all() and (_host(dwws)[idle] == 0).all()
    red = parts.sum(0)
    o = [C * 27, C * 27 + 27 * 27, C * 27 + 27 * 27 + C, C * 27 + 27 * 27 + 2 * C]
    got = dict(P1=red[:o[0]].view(C, 27), gram=red[o[0]:o[1]].view(27, 27), s1=red[o[1]:o[2]], s2=red[o[2]:o[3]], colsum=red[o[3]:], dw_dw=rows_dw)
    fin = (_host(dws), _host(dgs), _host(dbs))
    for v, n in zip(fin, ("dW_s", "dgamma_s", "dbeta_s")):
        assert not torch.isnan(v).any(), n
    if mode == "exact":
        for n in ("dw_dw", "P1", "gram", "s1", "s2", "colsum"):
            _same(got[n], out[n], n)
        _same(_host(dwd), out["dw_dw"], "depthwise dW (combined)")
        for v, w, n in zip(fin, ref.sd_finalize(out, c)[:3], ("dW_s", "dgamma_s", "dbeta_s")):
            assert (v - w).abs().max().item() <= 1e-6 * w.abs().max().item(), (n, (v - w).abs().max().item(), w.abs().max().item())
        _timed(r.id, t0)
        return
    ks = ref.sd_k(g)
    for n in ("dw_dw", "P1", "gram", "s1", "s2", "colsum"):
        _bounded(got[n], out[n], terms[n], ks[n], "%s %s (acts %d / %d)" % (r.id, n, c["s_act"], c["d_act"]))
    _bounded(_host(dwd), out["dw_dw"], terms["dw_dw"], ks["dw_dw"] + 1, r.id + " depthwise dW (combined)")
    dW, dgamma, dbeta, mag = ref.sd_finalize(got, c)
    _bounded(fin[0], dW, mag, 4, r.id + " dW_s against the finalize of the kernel's own sums")
    _bounded(fin[1], dgamma, got["s2"].abs(), 1, r.id + " dgamma_s")
    _bounded(fin[2], dbeta, got["s1"].abs(), 1, r.id + " dbeta_s")
    _timed(r.id, t0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _ids(sr.PJ_TABLE))
def test_project_unit_backward(lib, r, mode):
    """mny_pj_bwd (fp32), all twelve (No, Ki) instantiations on three trips with six tiles in the last trip and three pixels in the last tile — the
    next-tile prefetch of D (Ki 32, 96) and the non-prefetching form (Ki 144, 192) both with a next tile to take.
    Exact: gd, dW and its partial rows, the two sums: equal.  Real: gd at 2e-5 max + 1e-5 (test_project_unit_backward_in_one_pass).  dW: a wave takes
    one 16-pixel tile per trip: 4 instructions of 4 products per accumulator and tile (at most 4 roundings each), then the four waves are added in
    order; a term dY a carries 2 roundings of dY (two fmas) and 3 of a (z, the leaky product, fp32 0.1): k = 16 trips + 4 + 5 on sum (|ca g| + |cb y| + |cc|) |z|,
    + 1 for the combined dW.  Sums: a lane adds 4 pixels per tile, two shuffles, the four waves; dz = gd act' carries the 2 roundings of dY, the No
    products of the data-gradient chain and the mask product with its 0.1 (2): k = 4 trips + 6 + No + 4 on sum (|dY terms| |W|); s2: + 3 (d - mean, invstd, the fma)
    on the same times |d_hat|.
    Worst measured ratio: 0.010 (the combined dW of pj-32-192, k = 58); the sums stay below 0.003."""
    t0 = time.time()
    g = _regime(lib, r)["bwd"]
    M, Ki, No = r.M, r.Ki, r.No
    c = ref.pj_case(r, mode)
    assert lib.query("mny_pj_bwd_supported", M, Ki, No, c["act"]) == 1
    out, terms = ref.pj_ref(c)
    names = ("G", "Y", "coef", "D", "d_scale", "d_shift", "d_mean", "d_invstd", "W")
    t = {n: _dev(c[n]) for n in names}
    gd, dw, dws, red = _nan(M, Ki), _nan(No, Ki), _nan(g.gx + 1, No * Ki), _nan(g.gx + 1, 2, Ki)
    lib.call("mny_pj_bwd", _p(t["G"]), _p(t["Y"]), _p(t["coef"]), _p(t["D"]), _p(t["d_scale"]), _p(t["d_shift"]), _p(t["d_mean"]), _p(t["d_invstd"]), c["act"],
             _p(t["W"]), _p(gd), _p(dw), _p(dws), _p(red), M, Ki, No, _st())
    torch.cuda.synchronize()
    got_gd, got_dw = _host(gd), _host(dw)
    rows, sums = _rows_written(dws, g.gx, "pj dW").view(No, Ki), _rows_written(red, g.gx, "pj sums")
    if mode == "exact":
        _same(got_gd, out["gd"], "gd")
        _same(rows, out["dw"], "dW partial rows")
        _same(got_dw, out["dw"], "dW")
        _same(sums[0], out["s1"], "sum dz")
        _same(sums[1], out["s2"], "sum dz d_hat")
        _timed(r.id, t0)
        return
    _close(got_gd, out["gd"], 0.0, 2e-5 * out["gd"].abs().max().item() + 1e-5, "gd")
    ks = ref.pj_k(g, No)
    _bounded(rows, out["dw"], terms["dw"], ks["dw"], r.id + " dW partial rows (act %d)" % c["act"])
    _bounded(got_dw, out["dw"], terms["dw"], ks["dw"] + 1, r.id + " dW")
    _bounded(sums[0], out["s1"], terms["s1"], ks["s1"], r.id + " sum dz")
    _bounded(sums[1], out["s2"], terms["s2"], ks["s2"], r.id + " sum dz d_hat")
    _timed(r.id, t0)
