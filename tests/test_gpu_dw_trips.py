"""The persistent loops of the depthwise kernels (csrc/dwconv.hip, csrc/dwbwd.hip, csrc/dwtile.hip) past their first trip.

Every depthwise kernel launches a capped grid and each workgroup walks `for (strip = lb * ppb + pix; strip < nstrips; strip += gx * ppb)` (register
forms) or `for (tile = lb; tile < ntiles; tile += gx)` (tile forms), carrying the weight-gradient accumulators, the BN partial sums, the producer's
sums, the XCD renumbering of the workgroup and — tile forms — the LDS ring and the halo-duty rotation across trips.  No shape of
test_gpu_kernels.py takes a second trip (tests/test_dw_regimes_cpu.py asserts that); the rows of dw_regimes.TABLE take a third, ragged one
("trips"), run strips tall enough for the ring to wrap twice on more tiles than workgroups ("tall"), or run the few-workgroup grid that is not
renumbered ("small").  Every test first asserts its regime from the restated geometry AND the library's own part-count query, so that a retuned
cap cannot quietly turn it back into a one-trip case.

The reference is the plain operation in fp64 on the CPU (tests/dw_trips_ref.py).  Two modes per row:

exact  inputs, taps and coefficients are small integers, pre-activations odd integers (never on a kink of ReLU / ReLU6), so every product and every
       partial sum is an integer below 2^24 (asserted on the reference: sum |terms| < 2^24 per output, whatever the order) and every stored value
       an integer of magnitude <= 256 (exact in bf16).  Every output — y, dX, dW and its partial rows, the BN partial sums, the producer's sums — is
       asserted EQUAL to the reference, every element of it, with outputs and partial rows pre-filled with NaN.  A skipped, repeated or stale strip,
       or an accumulator reset between trips, cannot hide behind a tolerance.
real   seeded normal data, h-swish on both sides (the activation with a continuous derivative: an fp32 pre-activation cannot fall on the other side
       of a jump than the fp64 one).  Element-wise outputs at the tolerances test_gpu_kernels.py applies to the same operation; reductions bounded by
       k 2^-24 sum |terms| with k derived from the accumulation order in each test's docstring.
"""
import ctypes

import pytest
import torch

import dw_regimes as dr
import dw_trips_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MODES = ["exact", "real"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


def _rows(*ops):
    return [pytest.param(r, id=r.id) for r in dr.TABLE if r.op in ops]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape, bf=False):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device="cuda")


def _dev(t, bf=False):
    return None if t is None else t.to(torch.bfloat16 if bf else torch.float32).cuda().contiguous()


def _host(t):
    return t.cpu().double()


class Data:
    """seeded inputs as fp64 tensors that hold exactly the values the kernel is given (fp32- or bf16-representable)"""

    def __init__(self, r, mode):
        self.g = torch.Generator().manual_seed(1000 + dr.TABLE.index(r))
        self.exact, self.bf = mode == "exact", r.bf16

    def ints(self, shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=self.g, dtype=torch.int8).double()

    def act(self, shape, lo=-2, hi=2):                   # a stored activation tensor
        if self.exact:
            return self.ints(shape, lo, hi)
        t = torch.randn(shape, generator=self.g, dtype=torch.float32)
        return (t.to(torch.bfloat16) if self.bf else t).double()

    def taps(self, C, K):
        if self.exact:
            return self.ints((C, K, K), -2, 2) if K == 3 else self.ints((C, K, K), -1, 1)
        return (torch.randn(C, K, K, generator=self.g, dtype=torch.float32) * (0.4 if K == 3 else 0.25)).double()

    def chan(self, C, a, b):                             # per-channel fp32 vector a + b * normal
        return (a + b * torch.randn(C, generator=self.g, dtype=torch.float32)).double()

    def odd(self, C):
        return 2 * self.ints((C,), -1, 1) + 1

    def view(self, C, code):
        """(scale, shift) of an input view: exact mode 2 x + odd = an odd integer, off the kinks at 0 and 6"""
        if self.exact:
            return (None, None) if code == 0 else (torch.full((C,), 2.0, dtype=torch.float64), self.odd(C))
        return self.chan(C, 1.0, 0.2), self.chan(C, 0.0, 0.3)


def _acts(r, mode):
    """(activation of the unit, activation of the input view): exact mode rotates through none / ReLU6 / ReLU; the producer's sums need a view"""
    if mode == "real":
        return 4, 4
    i = dr.TABLE.index(r)
    return (1, 3, 0)[i % 3], ((1, 3)[i % 2] if r.red else (1, 3, 0)[(i // 3) % 3])


def _regime(lib, r):
    g = dr.regime(r.op, r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16, r.red)
    for name, args in dr.query_args(r.op, r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16, r.red):
        assert lib.query(name, *args) == g.gx, (name, args, g.gx)
    if r.kind == "trips":
        assert g.gx == g.cap and g.units > 2 * g.units_per_trip, g
    elif r.kind == "tall":
        assert g.gx == g.cap and g.units > g.gx and g.TH >= 2 * (r.K + 1), g
    else:
        assert g.gx % 8 != 0 and g.trips == 1, g
    return g


def _depth(g, r):
    """(longest chain of fp32 additions one thread makes into an accumulator over all its trips — rows of a strip, K more for the halo steps, times the
    columns a tile-form thread owns —, number of thread accumulators the workgroup then adds up in a fixed order)"""
    return g.trips * (g.TH + r.K) * (2 if g.form == "tile" and r.K == 5 else 1), (g.PT if g.form == "tile" else g.ppb)


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


def _exact_ok(terms, what):
    assert terms.max().item() < 2 ** 24, "%s: sum|terms| %.0f is not below 2^24: the exact-mode data is too large" % (what, terms.max().item())


def _tol(bf, ref_max, kind):
    if kind == "fwd":
        return (2.0 ** -7, 2.0 ** -7 * 0.25 * max(1.0, ref_max)) if bf else (1e-4, 1e-5)
    if kind == "data":
        return (2.0 ** -7, 4e-3 * max(1.0, ref_max)) if bf else (1e-4, 1e-5)
    return (2.0 ** -7, 4e-3 * max(1.0, ref_max)) if bf else (2e-4, 2e-5 * max(1.0, ref_max))      # dX of the fused kernels


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("fwd"))
def test_forward_and_bn_partial_sums(lib, r, mode):
    """mny_dw_fwd on dw3_fwd_kernel / dw5_fwd_kernel (strides 1 and 2, fp32 and bf16 storage) and on the tile form (5x5, bf16).
    Real mode: y at 1e-4 / 1e-5 (fp32), 2^-7 (bf16: the tolerances of test_dw_forward_backward / test_dw_forward_tile_form_bf16).  The partial sums
    are taken over the STORED output, so they are held against the fp64 sums of the kernel's own y (itself checked element-wise): a thread adds one
    value per output row and owned column to its accumulator, trips (TH + K) [x 2 columns, 5x5 tile form] additions at the most (sum y^2 by fma: one
    rounding per step as well), then one thread adds the ppb (tile form: PT) accumulators of the workgroup; the rows are combined in fp64 here.
    k = that depth + that width.  Worst measured ratio to the bound: 0.014 on the multi-trip rows (sum y^2, fwd-k3s1-bf16, k = 28), 0.17 on the small
    ones (small-dw3_fwd, k = 13)."""
    g = _regime(lib, r)
    N, H, W, C, K, s, bf = r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16
    d = Data(r, mode)
    _, code = _acts(r, mode)
    x, w = d.act((N, H, W, C)), d.taps(C, K)
    xs, xh = d.view(C, code)
    y_ref = ref.conv(ref.act(ref.preact(x, xs, xh), code), w, s)
    Ho, Wo = ref.out_hw(H, W, K, s)
    y, stats = _nan(N, Ho, Wo, C, bf=bf), _nan(g.gx, 2, C)
    xd, wd, xsd, xhd = _dev(x, bf), _dev(w.view(C, 1, K, K)), _dev(xs), _dev(xh)
    lib.call("mny_dw_fwd" + ("_bf16" if bf else ""), _p(xd), _p(xsd), _p(xhd), code, _p(wd), _p(y), _p(stats), N, H, W, C, K, s, _st())
    torch.cuda.synchronize()
    got, st = _host(y), _host(stats)
    assert not torch.isnan(st).any(), "a partial row was not written"
    st = st.sum(0)
    if mode == "exact":
        assert y_ref.abs().max().item() <= 256
        _exact_ok((y_ref ** 2).sum((0, 1, 2)), "sum y^2")
        _same(got, y_ref, "y")
        _same(st[0], y_ref.sum((0, 1, 2)), "sum y")
        _same(st[1], (y_ref ** 2).sum((0, 1, 2)), "sum y^2")
        return
    _close(got, y_ref, *_tol(bf, y_ref.abs().max().item(), "fwd"), "y")
    n1, n2 = _depth(g, r)
    _bounded(st[0], got.sum((0, 1, 2)), got.abs().sum((0, 1, 2)), n1 + n2, r.id + " sum y")
    _bounded(st[1], (got ** 2).sum((0, 1, 2)), (got ** 2).sum((0, 1, 2)), n1 + n2, r.id + " sum y^2")


def _big(r):
    return r.N * r.H * r.W * r.C > 40e6


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("bwd_data"))
def test_backward_data(lib, r, mode):
    """mny_dw_bwd_data.  Stride 1 is the forward kernel over dY with the flipped filter and an addend (dw3_fwd_kernel / dw5_fwd_kernel: the XCD
    renumbering and the strip walk of the forward, the ADD instantiation).  Stride 2 is one thread per input quad on a grid capped at 8192 workgroups:
    a third trip needs more than 2 x 8192 x 256 quads (4 channels: 67 M elements of dX, the one large case of this file; its real mode runs without
    the 67 M-element addend, the exact mode with it).  No reductions: dX equal (exact), 1e-4 / 1e-5 or 2^-7 (real)."""
    g = _regime(lib, r)
    N, H, W, C, K, s, bf = r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16
    d = Data(r, mode)
    Ho, Wo = ref.out_hw(H, W, K, s)
    dy, w = d.act((N, Ho, Wo, C)), d.taps(C, K)
    add = None if (_big(r) and mode == "real") else d.act((N, H, W, C), -3, 3)
    dx = _nan(N, H, W, C, bf=bf)
    dyd, wd, addd = _dev(dy, bf), _dev(w.view(C, 1, K, K)), _dev(add, bf)
    lib.call("mny_dw_bwd_data" + ("_bf16" if bf else ""), _p(dyd), _p(wd), _p(addd), _p(dx), N, H, W, C, K, s, _st())
    torch.cuda.synchronize()
    want = ref.conv_dx(dy, w, s, H, W)
    del dy
    if add is not None:
        want += add
    del add
    got = _host(dx)
    if mode == "exact":
        assert want.abs().max().item() <= 256
        _same(got, want, "dX")
    else:
        _close(got, want, *_tol(bf, want.abs().max().item(), "data"), "dX")
    assert g.trips >= (3 if r.kind == "trips" else 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("bwd_weight"))
def test_backward_weight(lib, r, mode):
    """mny_dw_bwd_weight: 3x3 on the sliding-window kernel (dw_slide_kernel, MODE 1), 5x5 on dw5_wgrad_kernel (strides 1 and 2), the tap accumulators
    carried over three trips.  Exact: dW and the fp64 sum of its partial rows equal.  Real: a tap's accumulator takes one fma per row step, at most
    trips (TH + K) of them, then ppb accumulators are added per workgroup and the rows combined in fp64 and rounded once (+ 1); a term a dy carries
    the rounding of the h-swish view in fp32 (z = fma(x, s, h), z + 3, the clip, two products: 5 roundings, each at most 2^-24 |z| since |a| <= |z|) and
    of the product inside the fma (+ 1): k = depth + ppb + 7 on sum |z| |dy|.  Worst measured ratio: 0.004 on the multi-trip rows (bwd_weight-k5, k = 40),
    0.09 on the small ones (small-dw5_wgrad, k = 21)."""
    g = _regime(lib, r)
    N, H, W, C, K, s, bf = r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16
    d = Data(r, mode)
    _, code = _acts(r, mode)
    Ho, Wo = ref.out_hw(H, W, K, s)
    x, dy = d.act((N, H, W, C)), d.act((N, Ho, Wo, C))
    xs, xh = d.view(C, code)
    dw, ws = _nan(C, 1, K, K), _nan(g.gx, C * K * K)
    xd, dyd, xsd, xhd = _dev(x, bf), _dev(dy, bf), _dev(xs), _dev(xh)
    lib.call("mny_dw_bwd_weight" + ("_bf16" if bf else ""), _p(xd), _p(xsd), _p(xhd), code, _p(dyd), _p(dw), _p(ws), N, H, W, C, K, s, _st())
    torch.cuda.synchronize()
    z = ref.preact(x, xs, xh)
    want = ref.conv_dw(ref.act(z, code), dy, K, s)
    terms = ref.conv_dw(z.abs(), dy.abs(), K, s)
    got, rows = _host(dw).view(C, K, K), _host(ws)
    assert not torch.isnan(rows).any(), "a partial row was not written"
    rows = rows.sum(0).view(C, K, K)
    if mode == "exact":
        _exact_ok(terms, "dW")
        _same(got, want, "dW")
        _same(rows, want, "dW partial rows")
        return
    n1, n2 = _depth(g, r)
    _bounded(got, want, terms, n1 + n2 + 7, r.id + " dW")
    _bounded(rows, want, terms, n1 + n2 + 6, r.id + " dW partial rows")


def _fused(lib, r, mode):
    g = _regime(lib, r)
    N, H, W, C, K, s, bf = r.N, r.H, r.W, r.C, r.K, r.stride, r.bf16
    d = Data(r, mode)
    act, xact = _acts(r, mode)
    Ho, Wo = ref.out_hw(H, W, K, s)
    x, add = d.act((N, H, W, C)), d.act((N, H, W, C), -3, 3)
    gg, y, w = d.act((N, Ho, Wo, C)), d.act((N, Ho, Wo, C)), d.taps(C, K)
    xs, xh = d.view(C, xact)
    if mode == "exact":
        scale, shift = torch.full((C,), 2.0, dtype=torch.float64), d.odd(C)
        coef = torch.stack((d.ints((C,), 1, 2), d.ints((C,), -1, 1), d.ints((C,), -1, 1)))
        mean, invstd = d.ints((C,), -1, 1), d.ints((C,), 1, 2)
    else:
        scale, shift = d.chan(C, 1.0, 0.2), d.chan(C, 0.0, 0.3)
        coef = torch.stack((d.chan(C, 1.0, 0.2), d.chan(C, 0.0, 0.05), d.chan(C, 0.0, 0.05)))
        mean, invstd = d.chan(C, 0.0, 0.2), d.chan(C, 1.0, 0.1).abs()
    dx, dw, ws = _nan(N, H, W, C, bf=bf), _nan(C, 1, K, K), _nan(g.gx, C * K * K)
    red = _nan(g.gx, 2, C) if r.red else None
    t = [_dev(gg, bf), _dev(y, bf), _dev(scale), _dev(shift), _dev(coef), _dev(x, bf), _dev(xs), _dev(xh), _dev(mean), _dev(invstd), _dev(w.view(C, 1, K, K)),
         _dev(add, bf)]
    gd, yd, sc, sh, cf, xd, xsd, xhd, mu, istd, wd, addd = [_p(v) for v in t]
    sfx = "_bf16" if bf else ""
    if r.op == "bnbwd" and r.red:
        lib.call("mny_dw_bnbwd_red" + sfx, gd, yd, sc, sh, act, cf, xd, xsd, xhd, xact, mu, istd, wd, addd, _p(dx), _p(dw), _p(ws), _p(red), N, H, W, C, K, 1, _st())
    elif r.op == "bnbwd":
        lib.call("mny_dw_bnbwd" + sfx, gd, yd, sc, sh, act, cf, xd, xsd, xhd, xact, wd, addd, _p(dx), _p(dw), _p(ws), N, H, W, C, K, 1, _st())
    elif r.op == "bnbwd_s2":
        lib.call("mny_dw_bnbwd_s2" + sfx, gd, yd, sc, sh, act, cf, xd, xsd, xhd, xact, wd, addd, _p(dx), _p(dw), _p(ws), N, H, W, C, _st())
    else:
        lib.call("mny_dw_bnbwd_s2k5" + sfx, gd, yd, sc, sh, act, cf, xd, xsd, xhd, xact, mu if r.red else None, istd if r.red else None, wd, addd,
                 _p(dx), _p(dw), _p(ws), _p(red), N, H, W, C, _st())
    torch.cuda.synchronize()
    dY = ref.bn_dy(gg, y, scale, shift, act, coef)
    dX = ref.conv_dx(dY, w, s, H, W) + add
    z = ref.preact(x, xs, xh)
    dW = ref.conv_dw(ref.act(z, xact), dY, K, s)
    got_dx, got_dw, rows = _host(dx), _host(dw).view(C, K, K), _host(ws)
    assert not torch.isnan(rows).any(), "a weight-gradient partial row was not written"
    rows = rows.sum(0).view(C, K, K)
    sums = None
    if r.red:
        sums = _host(red)
        assert not torch.isnan(sums).any(), "a partial row of the producer's sums was not written"
        sums = sums.sum(0)
    xhat = (x - mean) * invstd
    if mode == "exact":
        assert dX.abs().max().item() <= 256
        _exact_ok(ref.conv_dw(z.abs(), dY.abs(), K, s), "dW")
        _exact_ok(dX.abs().sum((0, 1, 2)), "sum dz")
        _exact_ok((dX * xhat).abs().sum((0, 1, 2)), "sum dz xhat")
        _same(got_dx, dX, "dX")
        _same(got_dw, dW, "dW")
        _same(rows, dW, "dW partial rows")
        if r.red:
            _same(sums, ref.producer_sums(dX, x, xs, xh, xact, mean, invstd), "producer's sums")
        return
    _close(got_dx, dX, *_tol(bf, dX.abs().max().item(), "fused"), "dX")
    n1, n2 = _depth(g, r)
    terms = ref.conv_dw(z.abs(), ref.bn_dy_mag(gg, y, scale, shift, act, coef), K, s)
    _bounded(got_dw, dW, terms, n1 + n2 + 13, r.id + " dW")
    _bounded(rows, dW, terms, n1 + n2 + 12, r.id + " dW partial rows")
    if r.red:                                            # over the STORED dX, as the producer's own backward reads it
        want = ref.producer_sums(got_dx, x, xs, xh, xact, mean, invstd)
        _bounded(sums[0], want[0], got_dx.abs().sum((0, 1, 2)), n1 + n2 + 4, r.id + " sum dz")
        _bounded(sums[1], want[1], (got_dx * xhat).abs().sum((0, 1, 2)), n1 + n2 + 8, r.id + " sum dz xhat")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("bnbwd"))
def test_fused_unit_backward(lib, r, mode):
    """mny_dw_bnbwd / mny_dw_bnbwd_red: the register form (dw_bnbwd_s1k3_kernel: 3x3 fp32 with and without the producer's sums, bf16 with them) and the
    tile form (dwb_tile_kernel: 5x5 fp32 / bf16 / with the producer's sums, 3x3 bf16 at 16 and at 18 channel groups per workgroup; two column tiles
    with a narrower last one, several strips with a shorter last one; "tall" rows whose strips wrap the (K + 1)-row ring more than twice).
    dY = ca g act'(scale y + shift) + cb y + cc, dX = its data gradient + addend, dW against the activated view, the producer's sums over the stored dX.
    Exact: all equal.  Real: dX at 2e-4 / 2e-5 max|dX| (fp32), 2^-7 / 4e-3 max|dX| (bf16) as test_fused_dw_unit_backward.  dW: a tap's accumulator takes
    at most trips (TH + K) [x 2 columns per thread, 5x5 tile form] fmas, ppb (tile form: PT) accumulators are added per workgroup, the rows combined in
    fp64 and rounded once (+ 1); a term a dY carries 5 roundings of the h-swish view (each <= 2^-24 |z|), 6 of dY (z, act', g act', two fmas, the
    mask product — relative to |ca g act'| + |cb y| + |cc|) and the product's (+ 1): k = depth + width + 13 on sum |z| (|ca g act'| + |cb y| + |cc|).
    Producer's sums: one addition per output element of the thread; dz = dX act'(z) carries 3 roundings of act' and the product's (k = depth + width
    + 4 on sum |dX|), dz xhat four more (xhat: 2, product, fma; + 8 on sum |dX xhat|).  Worst measured ratios on the multi-trip rows: dW 0.006
    (bnbwd-k3, k = 41), sum dz 0.002, sum dz xhat 0.003; on small-bnbwd-k3: 0.074, 0.042, 0.061 (k = 25, 17, 21)."""
    _fused(lib, r, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("bnbwd_s2"))
def test_fused_stride2_unit_backward(lib, r, mode):
    """mny_dw_bnbwd_s2 (dw_bnbwd_s2k3_kernel, fp32 and bf16 storage): same reference, tolerances and k as test_fused_unit_backward (a thread walks quad
    rows: TH + K bounds its steps per strip).  Worst measured ratio: dW 0.006 (bnbwd_s2, k = 36), 0.11 on small-bnbwd_s2 (k = 24)."""
    _fused(lib, r, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", _rows("bnbwd_s2k5"))
def test_fused_5x5_stride2_unit_backward(lib, r, mode):
    """mny_dw_bnbwd_s2k5 (dw_bnbwd_s2k5_kernel: channel pairs), with and without the producer's sums, fp32 and bf16: same reference, tolerances and k as
    test_fused_unit_backward.  Worst measured ratios: dW 0.007 (bnbwd_s2k5-red, k = 41), sum dz 0.002, sum dz xhat 0.002; on small-bnbwd_s2k5: 0.11, 0.028,
    0.039 (k = 25, 16, 20)."""
    _fused(lib, r, mode)
