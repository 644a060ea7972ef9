"""Exact inputs and the fp64 reference for the rows of gate_regimes.TABLE: the per-pixel gate's three forward and three backward passes and the
one-pass bf16 project backward (csrc/gate.hip), as the plain operation on the CPU with bf16 round-to-nearest-even applied exactly where the kernels
apply it — the matrix operands tb, hb, dg, dhr (pj16: dY, a_d, W), the stored out / dt / gd, and the red3 / pj16 sums, taken over the STORED gradient.

The kernels take every BatchNorm constant as a pointer, so the generator supplies constants that keep every fp32 value EXACT: it then does not matter
whether the compiler contracts a multiply and an add, or in which order a sum is taken, and the GPU test asserts equality.

Gate recipe
  y3 integers in [-2, 2], s3 = +-1, b3 in {-1, 0, 1}: t is an integer, |t| <= 3 (with y3 in [-3, 3] and s3 = 2 allowed, |t| <= 7, the terms of the BN1 sums
  reach 0.94 of the 2^24 budget below at C = 160, M = 65557; this range leaves a factor of four).
  W1: six nonzeros of {+-1, +-2} per row; W2: three nonzeros of +-1 per row.
  sc1 = +-1, sh1 in {+-0.5, +-1.5}: z1 is a half-integer and never on ReLU's kink.
  sc2 = +-3, sh2 = 0.75 + 1.5 k: z2 + 3 is an ODD multiple of 0.75, so z2 is never +-3, and inside (0, 6) fl((z2 + 3) * fl(1 / 6)) is exactly an
  odd eighth ((0.75 k) * float32(1 / 6) == k / 8 in fp32 for every odd |k| <= 2001, asserted by the CPU test): the gate, out and dO * gate are exact.
  dO in 6 * {-2 .. 2}: dO * t * fl(1 / 6) is an exact integer ((6 n) * float32(1 / 6) == n for |n| <= 4096, asserted too).
  mean rows small integers, invstd rows and the ca / cb rows of coef1 / coef2 powers of two, cc small integers.
  Residual operand: integers in [-4, 4], scale in {1, -1, 2}, shift in {-1, 0, 1}.

pj16 recipe
  G, Y integers in [-3, 3]; ca, cb in {+-1, +-2, +-0.5}, cc integer: dY is a half-integer, exact in bf16.  W: four nonzeros of {+-1, +-2} per input
  channel.  D integers, d_scale = +-1, d_shift a half-odd: z is never on a kink of ReLU / ReLU6.
  h-swish rows: D in 4 * {-2 .. 2}, d_scale = +-0.75, d_shift = 0.75 (4 i + 3): z = 0.75 k with k = 3 (mod 4).  z is then never +-3, act_fwd is exact
  (an odd eighth times z), and the interior z are -0.75 and 2.25 only.  That last restriction is needed: act_bwd is ONE fma, fmaf(z, fl(1 / 3), 0.5), and
  fl(1 / 3) = (1 + 2^-25) / 3, so at z = -2.25 its correctly rounded value is -(0.25 + 2^-25), and gd times that is no longer a short dyadic number
  — the sums would depend on their order.  At z = -0.75 (a tie, to even) and z = 2.25 the fma gives 0.25 and 1.25 exactly.  The reference still
  evaluates the fma in fp64 from float32(1 / 3) and rounds once.

Every reduction's terms are returned next to its value: the CPU test finds their common power-of-two unit and asserts that (most pixels one workgroup
accumulates) x (largest |term|) stays below 2^24 units of its accumulator, so that every fp32 partial sum is exact whatever its order.
"""
import numpy as np
import torch

import gate_regimes as gr

F64 = torch.float64
SIXTH = float(np.float32(1.0) / np.float32(6.0))
THIRD = float(np.float32(1.0) / np.float32(3.0))
RESIDUALS = (None, "plain", "view", "view-relu")


def bf(v):
    """fp64 -> fp32 (must already be exact) -> bf16 round-to-nearest-even -> fp64"""
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


def f32(v):
    """one fp32 rounding of an fp64 value"""
    return v.to(torch.float32).to(F64)


def _pick(g, values, *shape):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _sparse_rows(g, rows, cols, nnz, values):
    w = torch.zeros(rows, cols, dtype=F64)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nnz]
        w[r, idx] = _pick(g, values, nnz)
    return w


def gate_case(M, C, R, seed=0):
    """exact inputs of one gate row; the four residual operands of RESIDUALS share everything else"""
    g = torch.Generator().manual_seed(1000 * C + seed)
    c = dict(M=M, C=C, R=R)
    c["y3"] = _ints(g, -2, 2, M, C)
    c["s3"], c["b3"] = _pick(g, [1.0, -1.0], C), _pick(g, [-1.0, 0.0, 1.0], C)
    c["w1"] = _sparse_rows(g, R, C, 6, [1.0, -1.0, 2.0, -2.0])
    c["w2"] = _sparse_rows(g, C, R, 3, [1.0, -1.0])
    c["sc1"], c["sh1"] = _pick(g, [1.0, -1.0], R), _pick(g, [0.5, -0.5, 1.5, -1.5], R)
    c["sc2"], c["sh2"] = _pick(g, [3.0, -3.0], C), 0.75 + 1.5 * _ints(g, -2, 1, C)
    c["dout"] = 6.0 * _ints(g, -2, 2, M, C)
    c["mean1"], c["invstd1"] = _ints(g, -2, 2, R), _pick(g, [0.5, 1.0, 2.0], R)
    c["mean2"], c["invstd2"] = _ints(g, -2, 2, C), _pick(g, [0.5, 1.0, 2.0], C)
    c["mean3"], c["invstd3"] = _ints(g, -2, 2, C), _pick(g, [0.5, 1.0, 2.0], C)
    c["coef2"] = torch.stack((_pick(g, [1.0, -1.0, 2.0, -2.0], C), _pick(g, [0.5, -0.5, 0.25, -0.25], C), _ints(g, -2, 2, C)))
    c["coef1"] = torch.stack((_pick(g, [1.0, -1.0, 0.5, -0.5], R), _pick(g, [0.5, -0.5, 0.25, -0.25], R), _ints(g, -2, 2, R)))
    c["add_x"] = _ints(g, -4, 4, M, C)
    c["add_scale"], c["add_shift"] = _pick(g, [1.0, -1.0, 2.0], C), _pick(g, [-1.0, 0.0, 1.0], C)
    return c


def residual(c, kind):
    """(add_x, add_scale, add_shift, add_act) of mny_gate_fwd_bf16 for a residual kind"""
    if kind is None:
        return None, None, None, gr.ACT_NONE
    if kind == "plain":
        return c["add_x"], None, None, gr.ACT_NONE
    return c["add_x"], c["add_scale"], c["add_shift"], gr.ACT_RELU if kind == "view-relu" else gr.ACT_NONE


def _pair(x, y, idx):
    return torch.stack((x[idx].sum(0), y[idx].sum(0)))


def _products(a, b):
    """the terms of a weight gradient sum_px a[px, i] b[px, j] are not formed: worst_units() bounds them from the operands"""
    return dict(a=a, b=b)


def gate_ref(c, zero_hidden=None, round_grads=True):
    """-> (outputs, intermediates, terms, reduce).  `outputs` holds the element-wise results and the reductions over all M pixels; reduce(idx) gives
    the reductions over the pixels `idx` alone (they are sums over pixels, so the CPU test's mutations — pixels counted twice, a trip dropped — are
    sums and differences of such calls).  `zero_hidden`: hidden channels whose operand hb is replaced by zero (a mutation too);
    round_grads=False leaves the gradient operands dg, dhr and the stored dt unrounded, which is what autograd with straight-through roundings computes."""
    gbf = bf if round_grads else (lambda v: v)
    t = c["y3"] * c["s3"] + c["b3"]
    tb = bf(t)
    hr = tb @ bf(c["w1"]).t()
    z1 = hr * c["sc1"] + c["sh1"]
    hb = bf(torch.relu(z1))
    if zero_hidden is not None:
        hb[:, zero_hidden] = 0.0
    gg = hb @ bf(c["w2"]).t()
    z2 = gg * c["sc2"] + c["sh2"]
    gate = f32(torch.clamp(z2 + 3.0, 0.0, 6.0) * SIXTH)
    tg = t * gate
    out = {}
    mid = dict(t=t, hr=hr, z1=z1, g=gg, z2=z2, gate=gate, tg=tg)
    for kind in RESIDUALS:
        ax, asc, ash, aact = residual(c, kind)
        o = tg
        if ax is not None:
            a = ax * asc + ash if asc is not None else ax
            o = tg + (torch.relu(a) if aact == gr.ACT_RELU else a)
        mid["out_f32:%s" % kind] = o
        out["out:%s" % kind] = bf(o)
    # backward
    dO = c["dout"]
    inside = (z2 > -3.0) & (z2 < 3.0)
    dz2 = f32(f32(dO * t) * torch.where(inside, torch.full_like(z2, SIXTH), torch.zeros_like(z2)))
    ca2, cb2, cc2 = c["coef2"]
    dg = ca2 * dz2 + (cb2 * gg + cc2)
    dgb = gbf(dg)
    dh = dgb @ bf(c["w2"])
    dz1 = torch.where(z1 > 0, dh, torch.zeros_like(dh))
    ca1, cb1, cc1 = c["coef1"]
    dhr = ca1 * dz1 + (cb1 * hr + cc1)
    dhrb = gbf(dhr)
    dog = f32(dO * gate)
    dt32 = dog + dhrb @ bf(c["w1"])
    dt = gbf(dt32)
    out["dt"] = dt
    mid.update(dz2=dz2, dg=dg, dh=dh, dhr=dhr, dog=dog, dt32=dt32)
    terms = dict(st1=(hr, hr * hr), st2=(gg, gg * gg), red2=(dz2, dz2 * ((gg - c["mean2"]) * c["invstd2"])), red1=(dz1, dz1 * ((hr - c["mean1"]) * c["invstd1"])),
                 red3=(dt, dt * ((c["y3"] - c["mean3"]) * c["invstd3"])), dw2=_products(dgb, hb), dw1=_products(dhrb, tb))

    def reduce(idx):
        r = {k: _pair(terms[k][0], terms[k][1], idx) for k in ("st1", "st2", "red2", "red1", "red3")}
        r["dw2"] = dgb[idx].t() @ hb[idx]
        r["dw1"] = dhrb[idx].t() @ tb[idx]
        return r

    out.update(reduce(slice(None)))
    return out, mid, terms, reduce


def pj_case(M, Ki, No, act, seed=0):
    g = torch.Generator().manual_seed(1000 * Ki + No + seed)
    c = dict(M=M, Ki=Ki, No=No, act=act)
    c["G"], c["Y"] = _ints(g, -3, 3, M, No), _ints(g, -3, 3, M, No)
    c["coef"] = torch.stack((_pick(g, [1.0, -1.0, 2.0, -2.0, 0.5, -0.5], No), _pick(g, [1.0, -1.0, 2.0, -2.0, 0.5, -0.5], No), _ints(g, -2, 2, No)))
    c["W"] = _sparse_rows(g, Ki, No, 4, [1.0, -1.0, 2.0, -2.0]).t().contiguous()                    # [No, Ki]
    if act == gr.ACT_HSWISH:
        c["D"] = 4.0 * _ints(g, -2, 2, M, Ki)
        c["d_scale"], c["d_shift"] = _pick(g, [0.75, -0.75], Ki), 0.75 * (4.0 * _ints(g, -2, 1, Ki) + 3.0)
    else:
        c["D"] = _ints(g, -8, 8, M, Ki)
        c["d_scale"], c["d_shift"] = _pick(g, [1.0, -1.0], Ki), _ints(g, -2, 3, Ki) + 0.5
    c["d_mean"], c["d_invstd"] = _ints(g, -2, 2, Ki), _pick(g, [0.5, 1.0, 2.0], Ki)
    return c


def act_fwd(z, act):
    if act == gr.ACT_NONE:
        return z
    if act == gr.ACT_RELU:
        return torch.relu(z)
    if act == gr.ACT_RELU6:
        return torch.clamp(z, 0.0, 6.0)
    assert act == gr.ACT_HSWISH
    return f32(z * f32(torch.clamp(z + 3.0, 0.0, 6.0) * SIXTH))


def act_bwd(z, act):
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if act == gr.ACT_NONE:
        return one
    if act == gr.ACT_RELU:
        return torch.where(z > 0, one, zero)
    if act == gr.ACT_RELU6:
        return torch.where((z > 0) & (z < 6.0), one, zero)
    assert act == gr.ACT_HSWISH
    return torch.where(z <= -3.0, zero, torch.where(z >= 3.0, one, f32(z * THIRD + 0.5)))         # one fma: a single rounding


def pj_ref(c, zero_thin=None, zero_wide=None):
    """-> (outputs, intermediates, terms, reduce) as gate_ref; `zero_thin`: channels of the operand dY, `zero_wide`: of a_d, replaced by zero"""
    ca, cb, cc = c["coef"]
    dY = ca * c["G"] + (cb * c["Y"] + cc)
    dYb = bf(dY)
    if zero_thin is not None:
        dYb[:, zero_thin] = 0.0
    gd32 = dYb @ bf(c["W"])
    gd = bf(gd32)
    z = c["D"] * c["d_scale"] + c["d_shift"]
    a = act_fwd(z, c["act"])
    ab = bf(a)
    if zero_wide is not None:
        ab[:, zero_wide] = 0.0
    slope = act_bwd(z, c["act"])
    dz = f32(gd * slope)
    mid = dict(dY=dY, gd32=gd32, z=z, a=a, slope=slope, dz=dz)
    terms = dict(red=(dz, dz * ((c["D"] - c["d_mean"]) * c["d_invstd"])), dw=_products(dYb, ab))

    def reduce(idx):
        return dict(red=_pair(terms["red"][0], terms["red"][1], idx), dw=dYb[idx].t() @ ab[idx])

    out = dict(gd=gd)
    out.update(reduce(slice(None)))
    return out, mid, terms, reduce


def unit_of(v):
    """per column of v [pixels, n]: the largest power of two 2^-k (k >= 0) of which every value of the column is a multiple -> [n]"""
    unit = torch.zeros(v.shape[1], dtype=F64)
    for k in range(0, 40):
        s = 2.0 ** k
        ok = ((v * s) == torch.round(v * s)).all(0) & (unit == 0)
        unit[ok] = 2.0 ** -k
        if bool((unit > 0).all()):
            return unit
    raise AssertionError("values are no short dyadic numbers")


def worst_units(terms):
    """terms of a reduction -> the largest |term| of any one accumulator, in units of that accumulator's own power of two"""
    if isinstance(terms, dict):                                     # a weight gradient: operands a [pixels, i], b [pixels, j]
        a, b = terms["a"], terms["b"]
        return float(((a.abs().amax(0) / unit_of(a))[:, None] * (b.abs().amax(0) / unit_of(b))[None, :]).max())
    return max(float((t.abs().amax(0) / unit_of(t)).max()) for t in terms)
