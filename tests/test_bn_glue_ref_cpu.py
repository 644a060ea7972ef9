"""The fp64 references of tests/bn_glue_ref.py against torch itself (no GPU): autograd of F.batch_norm + activation, torch's own
bfloat16 conversion, F.interpolate / slicing / torch.cat.  tests/test_gpu_bn_glue.py trusts these references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_glue_ref as R

F64 = torch.float64
N, H, W, C = 3, 7, 5, 12
EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed), dtype=F64)


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("act", range(R.N_ACTS))
def test_bn_backward_refs_match_autograd(act, frozen):
    x = (randn(N, H, W, C, seed=1) * 1.7 + 0.3).requires_grad_(True)
    gamma = (1 + 0.3 * randn(C, seed=2)).requires_grad_(True)
    beta = (0.4 * randn(C, seed=3)).requires_grad_(True)
    rm, rv = 0.2 * randn(C, seed=4), 0.5 + torch.rand(C, generator=gen(5), dtype=F64)
    g = randn(N, H, W, C, seed=6)
    if frozen:
        out = F.batch_norm(nchw(x), rm, rv, gamma, beta, False, 0.0, EPS)
    else:
        out = F.batch_norm(nchw(x), None, None, gamma, beta, True, 0.0, EPS)
    a = R.act_fn(out, act)
    a.backward(nchw(g))

    M = N * H * W
    x2, g2 = x.detach().reshape(M, C), g.reshape(M, C)
    if frozen:
        mean, invstd = rm, 1 / torch.sqrt(rv + EPS)
        scale = gamma.detach() * invstd
        shift = beta.detach() - mean * scale
    else:
        rows = torch.stack((x2.sum(0), (x2 * x2).sum(0))).view(1, 2, C)
        scale, shift, mean, invstd, _, _ = R.bn_finalize_ref(rows, M, gamma, beta, EPS, 0.1)
    assert rel(R.view(x2, scale, shift, act), a.detach().permute(0, 2, 3, 1).reshape(M, C)) <= 1e-12
    s, q, sa, qa = R.bn_bwd_sums_ref(g2, x2, scale, shift, act, mean, invstd)
    assert (sa >= s.abs()).all() and (qa >= q.abs()).all()
    coef = R.bn_bwd_coef_ref(s, q, M, gamma, mean, invstd, frozen=frozen)
    dx = R.bn_bwd_apply_ref(g2, x2, scale, shift, act, coef)
    assert rel(dx, x.grad.reshape(M, C)) <= 1e-12
    assert rel(q, gamma.grad) <= 1e-12
    assert rel(s, beta.grad) <= 1e-12
    mag = R.bn_bwd_apply_mag(g2, x2, scale, shift, act, coef)
    assert (mag >= dx.abs() * (1 - 1e-12)).all()
    assert (R.bn_bwd_coef_mag(s, q, M, gamma, mean, invstd) >= R.bn_bwd_coef_ref(s, q, M, gamma, mean, invstd).abs() * (1 - 1e-12)).all()


def test_bn_finalize_ref_matches_batch_norm_running_statistics():
    x = randn(N, H, W, C, seed=11) * 2 + 1
    rm, rv = 0.3 * randn(C, seed=12), 0.5 + torch.rand(C, generator=gen(13), dtype=F64)
    rm_t, rv_t = rm.clone(), rv.clone()
    gamma, beta = 1 + 0.3 * randn(C, seed=14), 0.2 * randn(C, seed=15)
    out = F.batch_norm(nchw(x), rm_t, rv_t, gamma, beta, True, 0.1, EPS)
    M = N * H * W
    x2 = x.reshape(M, C)
    rows = torch.stack((x2[:50].sum(0), (x2[:50] ** 2).sum(0), x2[50:].sum(0), (x2[50:] ** 2).sum(0))).view(2, 2, C)
    scale, shift, mean, invstd, rm2, rv2 = R.bn_finalize_ref(rows, M, gamma, beta, EPS, 0.1, rm, rv)
    assert rel(x2 * scale + shift, out.permute(0, 2, 3, 1).reshape(M, C)) <= 1e-12
    assert rel(rm2, rm_t) <= 1e-12 and rel(rv2, rv_t) <= 1e-12           # torch updates the running variance with the unbiased estimate
    assert rel(mean, x2.mean(0)) <= 1e-12 and rel(invstd, 1 / torch.sqrt(x2.var(0, unbiased=False) + EPS)) <= 1e-12
    # count = 1: no unbiased estimate exists, the biased one is used; a negative difference of sums is clamped
    one = torch.tensor([[[2.0, -1.0], [4.5, 0.5]]], dtype=F64)             # channel 0: var 0.5; channel 1: 0.5 - 1 < 0
    _, _, m1, i1, _, rv1 = R.bn_finalize_ref(one, 1, torch.ones(2), torch.zeros(2), EPS, 0.1, torch.zeros(2), torch.ones(2))
    assert torch.equal(m1, torch.tensor([2.0, -1.0], dtype=F64))
    assert rel(rv1, torch.tensor([0.9 + 0.05, 0.9], dtype=F64)) <= 1e-12
    assert i1[1].item() == 1 / np.sqrt(EPS)


@pytest.mark.parametrize("act", range(R.N_ACTS))
def test_act_grad_at_the_kinks_is_torchs_subgradient(act):
    z = torch.tensor([-6.0, -3.0, -2.0 ** -20, 0.0, 2.0 ** -20, 3.0, 6.0, 6 + 2.0 ** -20], dtype=F64)
    want = {0: [1] * 8,
            1: [0, 0, 0, 0, 1, 1, 0, 0],                                   # relu6 = hardtanh(0, 6): 1 on the open interval
            2: [0.1, 0.1, 0.1, 0.1, 1, 1, 1, 1],
            3: [0, 0, 0, 0, 1, 1, 1, 1],
            4: [0, 0, (3 - 2.0 ** -19) / 6, 0.5, (3 + 2.0 ** -19) / 6, 1, 1, 1],
            5: [0, 0, 1 / 6, 1 / 6, 1 / 6, 0, 0, 0]}[act]
    got = R.act_grad(z, act)
    assert rel(got, torch.tensor(want, dtype=F64)) <= 1e-15
    amb = R.kink_ambiguous(torch.tensor([3.0, 3 + 1e-7, 3 + 1e-6, 0.0, 1e-30, 6 - 1e-7], dtype=F64), act)
    assert amb.tolist() == [act in (4, 5), act in (4, 5), False, False, False, act == 1]


def test_to_bf16_rne_is_torchs_conversion():
    x = torch.randn(10000, generator=gen(21)) * torch.exp2(torch.randint(-30, 30, (10000,), generator=gen(22)).float())
    assert np.array_equal(R.to_bf16_rne(x.double().numpy()), x.to(torch.bfloat16).double().numpy())
    # ties: 1 + 2^-8 lies half way between 1 and 1 + 2^-7 -> even (1); 1 + 3 * 2^-8 -> 1 + 2^-6 (even); just above a tie goes up
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -40, 255.0, 257.0, 2.0 ** -20 * (1 + 2.0 ** -8),
                     0.0, -0.0, np.inf, -np.inf, 3.3895313892515355e38, 3.4028234663852886e38, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -126 * (1 - 2.0 ** -9)])
    want = np.array([1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7, 255.0, 256.0, 2.0 ** -20,
                     0.0, -0.0, np.inf, -np.inf, 3.3895313892515355e38, np.inf, 2.0 ** -133, 0.0, 2.0 ** -132, 2.0 ** -126])
    got = R.to_bf16_rne(ties)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    t32 = torch.tensor(ties, dtype=F64).float()                     # every entry but the 2^-40 one is an fp32 value: torch agrees
    keep = t32.double().numpy() == ties
    assert np.array_equal(got[keep], t32.to(torch.bfloat16).double().numpy()[keep])
    assert np.isnan(R.to_bf16_rne(np.array([np.nan]))[0])
    assert np.array_equal(R.bf16_ulp(np.array([1.0, 1.5, 2.0, 0.75])), np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]))


def test_glue_refs_match_torch():
    Ca, Cb = 4, 12
    a, b = randn(N, 6, 4, Cb, seed=31), randn(N, 6, 4, Cb, seed=32)
    up = randn(N, 3, 2, Cb, seed=33)
    sc, sh = 1 + 0.2 * randn(Cb, seed=34), 0.3 * randn(Cb, seed=35)
    u = F.interpolate(nchw(up), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.upsample2x(up), u)
    want = a + F.leaky_relu(b * sc + sh, 0.1) + u
    assert rel(R.add_views_ref(a, (None, None, 0), b, (sc, sh, 2), up), want) <= 1e-15
    assert torch.equal(R.add_views_ref(a, (None, None, 0)), a)
    # upsample backward = autograd of F.interpolate
    ur = up.clone().requires_grad_(True)
    F.interpolate(nchw(ur), scale_factor=2, mode="nearest").backward(nchw(a))
    assert rel(R.upsample_bwd_ref(a), ur.grad) <= 1e-15
    assert rel(R.upsample_bwd_ref(a, up), ur.grad + up) <= 1e-15
    # gate product and its gradient wrt the first operand
    ar = a.clone().requires_grad_(True)
    prod = F.relu(ar * sc + sh) * (F.relu6(b + 3) / 6)
    assert rel(R.mul_views_ref(a, (sc, sh, 3), b, (None, None, 5)), prod.detach()) <= 1e-15
    va = F.relu(ar * sc + sh)
    va.retain_grad()
    (va * (F.relu6(b + 3) / 6)).backward(a)
    assert rel(R.mul_views_bwd_ref(a, b, (None, None, 5)), va.grad) <= 1e-15
    assert rel(R.mul_views_bwd_ref(a, b, (None, None, 5), addend=b), va.grad + b) <= 1e-15
    # PartAdd and its channel slice
    x = randn(N, 6, 4, Ca, seed=36)
    want = torch.cat((x + u[..., :Ca], u[..., Ca:]), -1)
    assert torch.equal(R.partadd_up_ref(x, (None, None, 0), up), want)
    assert torch.equal(R.slice_channels_ref(a, Ca), a[..., :Ca])
    assert torch.equal(R.slice_channels_ref(a, Ca, x), a[..., :Ca] + x)
    # axpy, row padding, padded transpose
    v = randn(37, seed=37)
    assert torch.equal(R.axpy_ref(v), v) and torch.equal(R.axpy_ref(v, 0.5, v), 1.5 * v)
    m = randn(5, 3, seed=38)
    assert torch.equal(R.pad_rows_ref(m, 2.0, 4), torch.cat((2 * m, torch.zeros(5, 1, dtype=F64)), 1))
    assert torch.equal(R.pad_rows_ref(m, None, 3), m)
    assert torch.equal(R.transpose_pad_ref(m, 8), torch.cat((m.t(), torch.zeros(3, 3, dtype=F64)), 1))
