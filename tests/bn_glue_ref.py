"""fp64 references of the BatchNorm and glue operations of include/mnyolo.h (torch CPU / numpy only).

Every function restates the OPERATION (what nn.BatchNorm2d, the activations, nn.Upsample, torch.add / torch.cat of the reference
model compute), in double precision and without any of the kernels' thread layouts, partial rows or operation order.  Activation
tensors are channels-last: [M, C] or [N, H, W, C]; per-channel parameters are [C].  tests/test_bn_glue_ref_cpu.py holds these
functions against torch autograd; tests/test_gpu_bn_glue.py holds the kernels against them."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
N_ACTS = 6                                  # MNY_ACT_NONE, RELU6, LEAKY(0.1), RELU, HSWISH, HSIGMOID
# pre-activations at which the derivative of act jumps, and the largest jump there
KINKS = {0: (), 1: (0.0, 6.0), 2: (0.0,), 3: (0.0,), 4: (-3.0, 3.0), 5: (-3.0, 3.0)}


def d(x):
    """Any tensor / array / scalar as an fp64 CPU tensor (exact for fp32 and bf16 inputs)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(F64)
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def act_fn(z, act):
    if act == 0:
        return z
    if act == 1:
        return F.relu6(z)
    if act == 2:
        return F.leaky_relu(z, 0.1)
    if act == 3:
        return F.relu(z)
    if act == 4:
        return z * F.relu6(z + 3) / 6          # the reference model's h-swish
    if act == 5:
        return F.relu6(z + 3) / 6              # ... and h-sigmoid
    raise ValueError("act %r" % (act,))


def view(x, scale, shift, act):
    """The activated view act(scale * x + shift) a consumer reads; scale = None: no affine part."""
    x = d(x)
    z = x if scale is None else x * d(scale) + d(shift)
    return act_fn(z, act)


def act_grad(z, act):
    """d act / dz at z, from torch autograd in fp64 (torch's subgradient choices at the kinks)."""
    zz = d(z).clone().requires_grad_(True)
    (act_fn(zz, act) * 1.0).sum().backward()
    return zz.grad.detach()


def act_grad_mag(z, act):
    """Sum of the magnitudes of the terms that form act_grad (h-swish: relu6(z+3)/6 + z/6 cancels around z = -1.5)."""
    z = d(z)
    if act == 4:
        return act_fn(z, 5).abs() + (z.abs() / 6) * ((z > -3) & (z < 3))
    return act_grad(z, act).abs()


def view_mag(x, scale, shift, act):
    """What a rounding bound of view() refers to: |act(z)| for the roundings inside the activation plus |z| * |act'(z)| (by terms) for
    the rounding of z itself — h-swish and h-sigmoid do not pass through the origin, so the second is not covered by the first."""
    x = d(x)
    z = x if scale is None else x * d(scale) + d(shift)
    return act_fn(z, act).abs() + z.abs() * act_grad_mag(z, act)


def kink_ambiguous(z, act):
    """Elements whose fp64 pre-activation is so close to a non-zero kink that its fp32 rounding may land on the other side (a
    correctly rounded fp32 value never changes sign, so the kink at 0 cannot be crossed)."""
    z = d(z)
    m = torch.zeros_like(z, dtype=torch.bool)
    for k in KINKS[act]:
        if k != 0.0:
            m |= (z - k).abs() <= 2.0 ** -23 * abs(k)
    return m


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
def bn_finalize_ref(stats_rows, count, gamma, beta, eps, momentum, rm=None, rv=None):
    """stats_rows [parts, 2, C] = partial (sum x, sum x^2).  Returns scale, shift, mean, invstd, rm', rv' (the last two None without rm)."""
    rows = d(stats_rows)
    s, q = rows[:, 0].sum(0), rows[:, 1].sum(0)
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)          # biased; a negative difference of rounded sums is no variance
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = d(gamma) * invstd
    shift = d(beta) - mean * scale
    rm2 = rv2 = None
    if rm is not None:
        unbiased = var * count / (count - 1) if count > 1 else var
        rm2 = (1 - momentum) * d(rm) + momentum * mean
        rv2 = (1 - momentum) * d(rv) + momentum * unbiased
    return scale, shift, mean, invstd, rm2, rv2


def bn_bwd_sums_ref(g, y, scale, shift, act, mean, invstd):
    """(sum dz, sum dz * yhat, sum |dz|, sum |dz * yhat|) per channel over the rows of g, y [M, C]."""
    g, y = d(g), d(y)
    z = y * d(scale) + d(shift)
    dz = g * act_grad(z, act)
    t = dz * ((y - d(mean)) * d(invstd))
    return dz.sum(0), t.sum(0), dz.abs().sum(0), t.abs().sum(0)


def bn_bwd_coef_ref(s, q, count, gamma, mean, invstd, frozen=False):
    """Rows (ca, cb, cc) of dy = ca * dz + cb * y + cc.
    training: dy = gamma * invstd * (dz - mean(dz) - yhat * mean(dz * yhat)), yhat = (y - mean) * invstd, written out in y;
    frozen  : the statistics are constants, dy = gamma * invstd * dz."""
    gamma, mean, invstd = d(gamma), d(mean), d(invstd)
    a = gamma * invstd
    if frozen:
        return torch.stack((a, torch.zeros_like(a), torch.zeros_like(a)))
    mdz, mdzy = d(s) / count, d(q) / count
    cb = -a * mdzy * invstd
    cc = -a * mdz + a * mdzy * invstd * mean
    return torch.stack((a, cb, cc))


def bn_bwd_coef_mag(s, q, count, gamma, mean, invstd):
    """Sum of term magnitudes per coefficient row (what a relative rounding bound refers to)."""
    gamma, mean, invstd = d(gamma), d(mean), d(invstd)
    a = (gamma * invstd).abs()
    mdz, mdzy = d(s).abs() / count, d(q).abs() / count
    return torch.stack((a, a * mdzy * invstd, a * mdz + a * mdzy * invstd * mean.abs()))


def bn_bwd_apply_ref(g, y, scale, shift, act, coef):
    """dy = ca * dz + cb * y + cc with dz = g * act'(scale * y + shift); scale = None: z = y; coef = None: dy = dz."""
    g, y = d(g), d(y)
    z = y if scale is None else y * d(scale) + d(shift)
    dz = g * act_grad(z, act)
    if coef is None:
        return dz
    c = d(coef)
    return c[0] * dz + c[1] * y + c[2]


def bn_bwd_apply_mag(g, y, scale, shift, act, coef):
    g, y = d(g), d(y)
    z = y if scale is None else y * d(scale) + d(shift)
    m = g.abs() * act_grad_mag(z, act)
    if coef is None:
        return m
    c = d(coef).abs()
    return c[0] * m + c[1] * y.abs() + c[2]


# ---- glue ------------------------------------------------------------------------------------------------------------------------
def upsample2x(u):
    """nn.Upsample(scale_factor=2, mode='nearest') on [N, h, w, C]."""
    return d(u).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def add_views_ref(a, av, b=None, bv=None, up=None):
    """view(a) + view(b) + upsample2x(up); av / bv = (scale, shift, act)."""
    o = view(a, *av)
    if b is not None:
        o = o + view(b, *bv)
    if up is not None:
        o = o + upsample2x(up)
    return o


def upsample_bwd_ref(src, dst0=None):
    """Gradient of upsample2x: every coarse pixel collects its 2x2 fine pixels (+ what dst held when accumulating)."""
    s = d(src)
    N, H, W, C = s.shape
    o = s.view(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))
    return o if dst0 is None else o + d(dst0)


def mul_views_ref(a, av, b, bv):
    return view(a, *av) * view(b, *bv)


def mul_views_bwd_ref(g, o, ov, addend=None):
    """Gradient of a product wrt one operand: g times the OTHER operand's view (+ addend)."""
    r = d(g) * view(o, *ov)
    return r if addend is None else r + d(addend)


def partadd_up_ref(a, av, up):
    """PartAdd: upsample2x(up) [.., Cb] with view(a) [.., Ca] added onto its first Ca channels."""
    o = upsample2x(up).clone()
    Ca = a.shape[-1]
    o[..., :Ca] += view(a, *av)
    return o


def slice_channels_ref(src, Ca, dst0=None):
    o = d(src)[..., :Ca]
    return o if dst0 is None else o + d(dst0)


def axpy_ref(src, alpha=None, dst0=None):
    o = d(src) * (1.0 if alpha is None else float(alpha))
    return o if dst0 is None else o + d(dst0)


def pad_rows_ref(src, alpha, Cp):
    s = d(src)
    o = torch.zeros(s.shape[0], Cp, dtype=F64)
    o[:, :s.shape[1]] = s * (1.0 if alpha is None else float(alpha))
    return o


def transpose_pad_ref(src, Rp):
    s = d(src)
    o = torch.zeros(s.shape[1], Rp, dtype=F64)
    o[:, :s.shape[0]] = s.t()
    return o


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------
def to_bf16_rne(x64):
    """Round doubles to the nearest bfloat16 (8 significant bits, fp32's exponent range), ties to even.  Returns fp64 values."""
    x = np.asarray(x64, dtype=np.float64)
    out = x.copy()
    fin = np.isfinite(x) & (x != 0)
    m, e = np.frexp(x[fin])                               # x = m * 2^e, 0.5 <= |m| < 1
    e = np.maximum(e, -125)                               # below 2^-126 the spacing stays 2^-133 (subnormals)
    r = np.ldexp(np.rint(np.ldexp(x[fin], 8 - e)), e - 8)  # np.rint rounds halves to even
    r[np.abs(r) >= 2.0 ** 128] = np.inf * np.sign(r[np.abs(r) >= 2.0 ** 128])
    out[fin] = r
    return out


def bf16_ulp(x64):
    """Spacing of bfloat16 at |x| (normal range)."""
    _, e = np.frexp(np.asarray(x64, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(e, -125) - 8)
