"""fp64 CPU reference of the depthwise operations for tests/test_gpu_dw_trips.py, on NHWC tensors.

A depthwise convolution is written out as the sum over its K x K taps of a shifted, strided slice of the zero-padded input times the tap — the
definition itself, one vectorised line per tap.  F.conv2d(groups=C) in fp64 states the same thing but takes the per-group path on the CPU
(15 s for 960 channels at the shapes of the trips table); tests/test_dw_regimes_cpu.py holds these functions against it, and against autograd
for the two gradients, at small shapes."""
import torch


def act(z, code):
    if code == 0:
        return z
    if code == 1:
        return z.clamp(0, 6)
    if code == 2:
        return torch.where(z > 0, z, 0.1 * z)
    if code == 3:
        return z.clamp(min=0)
    return z * (z + 3).clamp(0, 6) / 6


def dact(z, code):
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if code == 0:
        return one
    if code == 1:
        return torch.where((z > 0) & (z < 6), one, zero)
    if code == 2:
        return torch.where(z > 0, one, 0.1 * one)
    if code == 3:
        return torch.where(z > 0, one, zero)
    return torch.where(z <= -3, zero, torch.where(z >= 3, one, z / 3 + 0.5))


def preact(x, xs, xh):
    return x if xs is None else x * xs + xh


def out_hw(H, W, K, s):
    P = K // 2
    return (H + 2 * P - K) // s + 1, (W + 2 * P - K) // s + 1


def _pad(a, P):
    N, H, W, C = a.shape
    ap = a.new_zeros(N, H + 2 * P, W + 2 * P, C)
    ap[:, P:P + H, P:P + W] = a
    return ap


def _taps(H, W, K, s):
    Ho, Wo = out_hw(H, W, K, s)
    for kr in range(K):
        for kq in range(K):
            yield kr, kq, slice(kr, kr + s * (Ho - 1) + 1, s), slice(kq, kq + s * (Wo - 1) + 1, s)


def conv(a, w, s):
    """a [N,H,W,C], w [C,K,K] -> [N,Ho,Wo,C] (padding K // 2)"""
    N, H, W, C = a.shape
    K = w.shape[-1]
    ap = _pad(a, K // 2)
    Ho, Wo = out_hw(H, W, K, s)
    y = a.new_zeros(N, Ho, Wo, C)
    for kr, kq, rs, cs in _taps(H, W, K, s):
        y += ap[:, rs, cs] * w[:, kr, kq]
    return y


def conv_dx(dy, w, s, H, W):
    """gradient of conv(a, w, s) w.r.t. a [N,H,W,C]"""
    N, _, _, C = dy.shape
    K = w.shape[-1]
    P = K // 2
    dp = dy.new_zeros(N, H + 2 * P, W + 2 * P, C)
    for kr, kq, rs, cs in _taps(H, W, K, s):
        dp[:, rs, cs] += dy * w[:, kr, kq]
    return dp[:, P:P + H, P:P + W].contiguous()


def conv_dw(a, dy, K, s):
    """gradient of conv(a, w, s) w.r.t. w -> [C,K,K]"""
    N, H, W, C = a.shape
    ap = _pad(a, K // 2)
    dw = a.new_zeros(C, K, K)
    for kr, kq, rs, cs in _taps(H, W, K, s):
        dw[:, kr, kq] = (ap[:, rs, cs] * dy).sum((0, 1, 2))
    return dw


def bn_dy(g, y, scale, shift, code, coef):
    """BatchNorm(train) + activation backward in coefficient form: dY = ca g act'(scale y + shift) + cb y + cc"""
    return coef[0] * g * dact(y * scale + shift, code) + coef[1] * y + coef[2]


def bn_dy_mag(g, y, scale, shift, code, coef):
    """sum of the magnitudes of the three terms of bn_dy: what its fp32 rounding errors are relative to"""
    return (coef[0] * g * dact(y * scale + shift, code)).abs() + (coef[1] * y).abs() + coef[2].abs()


def producer_sums(dx, x, xs, xh, code, mean, invstd):
    """BN-backward sums of the unit that produced x: [2,C] = sum dz, sum dz xhat, dz = dX act'(xs x + xh)"""
    dz = dx * dact(preact(x, xs, xh), code)
    return torch.stack((dz.sum((0, 1, 2)), (dz * (x - mean) * invstd).sum((0, 1, 2))))
