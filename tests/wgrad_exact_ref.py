"""Inputs on which the weight gradient dW[N, K] = sum_m dY[m, n] act(scale X + shift)[m, k] is EXACT in fp32 whatever the order of summation, and
its plain fp64 reference.

Class "small" (every row of tests/wgrad_regimes.py): dY small integers, X small integers or half-integers, scale from {+-0.5, +-1, +-2, 3}, shift
from a few half-integers, the views none / ReLU6 / ReLU.  The h-swish views take scale 3, shift 0 on integer X ("hs3"), or no scale / shift on X in
multiples of 3 ("hs"): every z is <= -3, 0 or >= 3, where z * med3(z + 3, 0, 6) * (1/6f) — and z * (min(max(z + 3, 0), 6) * (1/6f)) of the
register-staged kernel — round to exactly 0 or z (6 * (1/6f) = 1 + 2^-25: a quarter of an ulp of z).  Every activated operand is a multiple of 1/4
below 32: bf16-representable, so the bf16 MFMA, the six-product cut (whose mid and lo pieces are zero) and the fp32 MFMA form the same products, and
every sum of products over the rows of a split is an integer multiple of 1/4 far below 2^24 units.

Class "wide16" (fp32 storage, no view): X odd integers of exactly 16 significant bits, dY from {+-1}; and "wide16-swapped" with the roles exchanged.  The
six-product form cuts such an operand into a hi and a NON-ZERO mid piece of 8 bits each (lo = 0): dropping a mid product changes dW.  At most 256 rows
per split keep every sum below 2^24.  (The lo piece cannot be made exact this way: it stays with the rms test of tests/test_gpu_kernels.py.)

The leaky view multiplies by 0.1f: not exact; leaky_ref() is the fp64 product on the fp32-evaluated view, for a tolerance.

The kernels round nothing but the bf16 kernel's activated operand (to bf16, exact here); reduce_parts_kernel sums the partial rows in fp64 and rounds
once to fp32: f32() of the fp64 sum.
"""
import numpy as np
import torch

import wgrad_regimes as wr

F64 = torch.float64
PAD_VALUE = 4096.0          # the rows behind M of the X and dY allocations
PAD_ROWS = 64
SCALES = [0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0]
SHIFTS = [-1.5, -0.5, 0.0, 0.5, 1.5]
LIMIT = float(2 ** 24)


def f32(v):
    """one fp32 rounding of an fp64 value"""
    return v.to(torch.float32).to(F64)


def bf(v):
    """fp64 -> fp32 -> bf16 round-to-nearest-even -> fp64"""
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


def _pick(g, values, *shape):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def act_fwd(z, act):
    if act == wr.ACT_NONE:
        return z
    if act == wr.ACT_RELU:
        return torch.relu(z)
    if act == wr.ACT_RELU6:
        return z.clamp(0.0, 6.0)
    if act == wr.ACT_HSWISH:
        return z * (z + 3.0).clamp(0.0, 6.0) / 6.0
    assert act == wr.ACT_LEAKY
    return torch.where(z > 0, z, z * float(np.float32(0.1)))


def blocks(n):
    """the 32-channel blocks an instantiation covers of n channels: slices (the last one may be short)"""
    return [slice(b, min(b + 32, n)) for b in range(0, n, 32)]


def case(row, kind="small"):
    """-> dict(X [M, K], dY [M, N], scale, shift ([K] or None), act, unit): fp64 tensors holding the exact inputs of a table row"""
    M, K, N = row.M, row.K, row.N
    g = torch.Generator().manual_seed(100003 * K + 1009 * N + M)
    act, view = wr.VIEWS[row.view]
    if kind != "small":
        wide = (torch.randint(2 ** 14, 2 ** 15, (M, max(K, N)), generator=g).to(F64) * 2 + 1) * _pick(g, [1.0, -1.0], M, max(K, N))
        ones = _pick(g, [1.0, -1.0], M, max(K, N))
        X, dY = (wide[:, :K], ones[:, :N]) if kind == "wide16" else (ones[:, :K], wide[:, :N])
        return dict(X=X.contiguous(), dY=dY.contiguous(), scale=None, shift=None, act=wr.ACT_NONE, unit=1.0, kind=kind)
    assert kind == "small"
    dY = torch.randint(-3, 4, (M, N), generator=g).to(F64)
    scale = shift = None
    if row.view == "hs":
        X = torch.randint(-2, 3, (M, K), generator=g).to(F64) * 3.0
    elif row.view == "hs3":
        X = torch.randint(-4, 5, (M, K), generator=g).to(F64)
        scale, shift = torch.full((K,), 3.0, dtype=F64), torch.zeros(K, dtype=F64)
    else:
        X = torch.randint(-12, 13, (M, K), generator=g).to(F64) * 0.5
        if view:
            scale, shift = _pick(g, SCALES, K), _pick(g, SHIFTS, K)
    # no row of dY and no row of the activated X is all zero inside a 32-channel block: row m gets a live entry in channel (m mod width) of each block
    m = torch.arange(M)
    for s in blocks(N):
        c = s.start + m % (s.stop - s.start)
        dY[m, c] = torch.where(dY[m, c] == 0, torch.ones(M, dtype=F64), dY[m, c])
    for s in blocks(K):
        c = s.start + m % (s.stop - s.start)
        if row.view == "hs":
            X[m, c] = 3.0
        elif row.view == "hs3":
            X[m, c] = 2.0
        else:                 # z = |scale| * 4 + shift >= 0.5 (and < 6 only where the scale is small: ReLU6 clamps the rest to 6, live as well)
            X[m, c] = 4.0 * (torch.sign(scale[c]) if scale is not None else torch.ones(M, dtype=F64))
    return dict(X=X, dY=dY, scale=scale, shift=shift, act=act, unit=0.25, kind=kind)


def activated(c):
    """act(scale X + shift), fp64 (exact for the exact classes)"""
    z = c["X"] if c["scale"] is None else c["X"] * c["scale"] + c["shift"]
    return act_fwd(z, c["act"])


def ref(c, rows=None):
    """-> dict(dw [N, K] fp64 sum, dbias [N]) over all rows, or over the rows `rows` (a slice / index tensor)"""
    a, dy = activated(c), c["dY"]
    if rows is not None:
        a, dy = a[rows], dy[rows]
    return dict(dw=dy.t() @ a, dbias=dy.sum(0))


def split_slices(g, M):
    """the rows of every split of a launch (g: wgrad_regimes.Regime; its plan's rows per split are those of split 0)"""
    rpb = M if g.splits == 1 else (M - g.last_split_rows) // (g.splits - 1)
    return [slice(s * rpb, min(M, (s + 1) * rpb)) for s in range(g.splits)]


def worst_units(c, g, M):
    """the largest sum over a split's rows of |dY| |act(X)|, in units of c['unit']: below 2^24, every partial sum of every order is exact in fp32"""
    a, dy = activated(c).abs(), c["dY"].abs()
    return max(float((dy[s].t() @ a[s]).max()) for s in split_slices(g, M)) / c["unit"]


def leaky_ref(c):
    """the leaky row: the view evaluated in fp32 as the kernels do (one fma, one multiply by 0.1f), the product in fp64"""
    x = c["X"].to(torch.float32)
    z = x if c["scale"] is None else torch.addcmul(c["shift"].to(torch.float32), x, c["scale"].to(torch.float32))
    a = torch.where(z > 0, z, z * np.float32(0.1)).to(F64)
    return dict(dw=c["dY"].t() @ a, dbias=c["dY"].sum(0), a=a)


def padded(t, bf16=False):
    """an allocation PAD_ROWS rows longer than t whose extra rows hold PAD_VALUE (CPU tensor; a call reads its first M rows)"""
    full = torch.full((t.shape[0] + PAD_ROWS, t.shape[1]), PAD_VALUE, dtype=torch.bfloat16 if bf16 else torch.float32)
    full[:t.shape[0]] = t.to(full.dtype)
    return full
