"""fp64 CPU references, the seeded inputs and the rounding budgets for tests/test_gpu_stem_trips.py and tests/test_stem_regimes_cpu.py.

Every reference takes an optional pixel weight `m` (0 / 1 per output pixel): the reductions are sums over output pixels, so the reference "with a unit
left out" is the full one minus the one weighted by that unit's pixels.  Activation tensors are NHWC, the image NCHW, as the library takes them.

Stem         y = conv2d(x, w, stride 2, pad 1); dW = dY^T P with P the [pixels, 27] patch matrix of x (F.unfold); the fused form rebuilds
             dY = ca g act'(sc y + sh) + cb y + cc.
stemdw       the algebra of the header of csrc/stemdw.hip on INDEPENDENT inputs (the kernel takes gd, d, s, x and every coefficient vector as inputs and
             does not recompute s from x): dY_d, its stride-1 depthwise data gradient G_s, the depthwise weight gradient against act_s(BN(s)),
             dz_s = G_s act_s'(BN(s)), s1, s2, P1 = dz_s^T P, Gram = P^T P, colsum(P), and the finalize of pw_bnbwd_finalize_kernel.
pj           dY = ca G + cb Y + cc, G_d = dY W, the BN-backward sums of the unit in front over dz = G_d act'(BN(D)), dW = dY^T act(BN(D)).
"""
import torch
import torch.nn.functional as F

import dw_trips_ref as dref
import stem_regimes as sr

U = 2.0 ** -24
act, dact = dref.act, dref.dact
KINKS = {0: (), 1: (0.0, 6.0), 2: (0.0,), 3: (0.0,), 4: (-3.0, 3.0)}


def patches(x):
    """[N,3,H,W] -> [N,Ho,Wo,27], tap = ci * 9 + kh * 3 + kw (the layout of the stem weight)"""
    N, _, H, W = x.shape
    Ho, Wo = sr.out_hw(H, W)
    return F.unfold(x, 3, padding=1, stride=2).view(N, 27, Ho, Wo).permute(0, 2, 3, 1).contiguous()


def stem_fwd(x, w):
    return F.conv2d(x, w, None, 2, 1).permute(0, 2, 3, 1).contiguous()


def stem_dw(P, dY, m=None):
    """sum over pixels of dY[pixel][Cout] (x) P[pixel][27] -> [Cout,3,3,3]"""
    if m is not None:
        dY = dY * m[..., None]
    return (dY.reshape(-1, dY.shape[-1]).t() @ P.reshape(-1, 27)).view(-1, 3, 3, 3)


def bn_dy(g, y, sc, sh, code, coef):
    return coef[0] * g * dact(y * sc + sh, code) + coef[1] * y + coef[2]


def bn_dy_mag(g, y, sc, sh, code, coef):
    return (coef[0] * g * dact(y * sc + sh, code)).abs() + (coef[1] * y).abs() + coef[2].abs()


def _sum(t, m=None):
    return (t if m is None else t * m[..., None]).sum((0, 1, 2))


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------------------
class Gen:
    """fp64 tensors that hold exactly the values the kernel is given (fp32- or bf16-representable)"""

    def __init__(self, seed, exact, bf=False):
        self.g = torch.Generator().manual_seed(seed)
        self.exact, self.dt = exact, (torch.bfloat16 if bf else torch.float32)

    def ints(self, shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=self.g, dtype=torch.int8).double()

    def normal(self, shape, mean=0.0, std=1.0, stored=False):
        t = mean + std * torch.randn(shape, generator=self.g, dtype=torch.float32)
        return (t.to(self.dt) if stored else t).double()

    def rand(self, shape, lo):
        return (lo + torch.rand(shape, generator=self.g, dtype=torch.float32)).double()

    def odd(self, C):
        return 2 * self.ints((C,), -1, 1) + 1

    def off_kinks(self, t, sc, sh, code):
        """real mode: move every element whose fp64 pre-activation lies within 1e-3 of a kink by 1/16 (in the storage type), so that the fp32 and the fp64
        evaluation take the same branch"""
        for _ in range(8):
            z = t * sc + sh
            bad = torch.zeros_like(z, dtype=torch.bool)
            for k in KINKS[code]:
                bad |= (z - k).abs() < 1e-3
            if not bad.any():
                return t
            t = torch.where(bad, (t.to(self.dt) + 0.0625).double(), t)
        raise AssertionError("could not move the pre-activations off the kinks")


def _seed(r):
    return 4000 + sr.TABLE.index(r)


EXACT_ACTS = (sr.ACT_NONE, sr.ACT_RELU, sr.ACT_RELU6)
ALL_ACTS = (sr.ACT_NONE, sr.ACT_RELU6, sr.ACT_LEAKY, sr.ACT_RELU)


def stem_case(r, mode, bf):
    """inputs of the three stem entry points at a table row.  Real mode rotates the fused form's activation through all five (h-swish included)."""
    i = sr.ST_TABLE.index(r)
    d = Gen(_seed(r) + (500 if bf else 0), mode == "exact", bf)
    Ho, Wo = sr.out_hw(r.H, r.W)
    C = r.Cout
    c = dict(bf=bf, mode=mode)
    if mode == "exact":
        c["act"] = EXACT_ACTS[(i + bf) % 3]
        c["x"], c["w"] = d.ints((r.N, 3, r.H, r.W), -2, 2), d.ints((C, 3, 3, 3), -1, 1)
        c["dy"], c["g"], c["yraw"] = (d.ints((r.N, Ho, Wo, C), -2, 2) for _ in range(3))
        c["scale"], c["shift"] = torch.full((C,), 2.0, dtype=torch.float64), d.odd(C)
        c["coef"] = torch.stack((d.ints((C,), 1, 2), d.ints((C,), -1, 1), d.ints((C,), -1, 1)))
        return c
    c["act"] = (i + 2 * bf) % 5
    c["x"], c["w"] = d.normal((r.N, 3, r.H, r.W), 1.0), d.normal((C, 3, 3, 3), 0.05, 0.3)
    c["dy"], c["g"] = d.normal((r.N, Ho, Wo, C), 0.5, stored=True), d.normal((r.N, Ho, Wo, C), 0.5, stored=True)
    c["scale"], c["shift"] = d.rand((C,), 0.5), d.normal((C,), 0.0, 0.3)
    c["coef"] = torch.stack((d.rand((C,), 0.5), d.normal((C,), 0.0, 0.05), d.normal((C,), 0.0, 0.05)))
    c["yraw"] = d.off_kinks(d.normal((r.N, Ho, Wo, C), 0.3, stored=True), c["scale"], c["shift"], c["act"])
    return c


def stem_ref(c, m=None):
    """reduced outputs of the three entry points and the sum of the magnitudes of their terms"""
    P = patches(c["x"])
    y = stem_fwd(c["x"], c["w"])
    dYb = bn_dy(c["g"], c["yraw"], c["scale"], c["shift"], c["act"], c["coef"])
    mag = bn_dy_mag(c["g"], c["yraw"], c["scale"], c["shift"], c["act"], c["coef"])
    out = dict(y=y, s1=_sum(y, m), s2=_sum(y * y, m), dw=stem_dw(P, c["dy"], m), dwb=stem_dw(P, dYb, m))
    terms = dict(s1=_sum(y.abs(), m), s2=out["s2"], dw=stem_dw(P.abs(), c["dy"].abs(), m), dwb=stem_dw(P.abs(), mag, m))
    return out, terms


def sd_acts(r, mode):
    """(activation of the stem unit, of the depthwise unit)"""
    i = sr.SD_TABLE.index(r)
    if mode == "exact":
        return EXACT_ACTS[i % 3], EXACT_ACTS[(i // 3 + i) % 3]
    return ALL_ACTS[i % 4], ALL_ACTS[(i // 4 + i + 1) % 4]


def sd_case(r, mode):
    d = Gen(_seed(r), mode == "exact")
    Ho, Wo = sr.out_hw(r.H, r.W)
    C = sr.SD_C
    sh4 = (r.N, Ho, Wo, C)
    c = dict(mode=mode, M=r.N * Ho * Wo)
    c["s_act"], c["d_act"] = sd_acts(r, mode)
    if mode == "exact":
        c["x"] = d.ints((r.N, 3, r.H, r.W), -2, 2)
        c["gd"], c["d"], c["s"] = d.ints(sh4, -2, 2), d.ints(sh4, -2, 2), d.ints(sh4, -2, 2)
        two = torch.full((C,), 2.0, dtype=torch.float64)
        c["d_scale"], c["d_shift"], c["s_scale"], c["s_shift"] = two, d.odd(C), two.clone(), d.odd(C)
        c["d_coef"] = torch.stack((d.ints((C,), 1, 2), d.ints((C,), -1, 1), d.ints((C,), -1, 1)))
        c["s_mean"], c["s_invstd"], c["s_gamma"] = d.ints((C,), -1, 1), 2.0 ** d.ints((C,), 0, 1), d.ints((C,), 1, 3)
        c["w_dw"], c["w_stem"] = d.ints((C, 3, 3), -1, 1), d.ints((C, 3, 3, 3), -2, 2)
        return c
    c["x"] = d.normal((r.N, 3, r.H, r.W), 1.0)
    c["gd"] = d.normal(sh4, 0.5)
    c["d_scale"], c["d_shift"], c["s_scale"], c["s_shift"] = d.rand((C,), 0.5), d.normal((C,), 0.5, 0.3), d.rand((C,), 0.5), d.normal((C,), 0.5, 0.3)
    c["d"] = d.off_kinks(d.normal(sh4, 0.3), c["d_scale"], c["d_shift"], c["d_act"])
    c["s"] = d.off_kinks(d.normal(sh4, 0.3), c["s_scale"], c["s_shift"], c["s_act"])
    c["d_coef"] = torch.stack((d.rand((C,), 0.5), d.normal((C,), 0.0, 0.05), d.normal((C,), 0.0, 0.05)))
    c["s_mean"], c["s_invstd"], c["s_gamma"] = d.normal((C,), 0.0, 0.2), d.rand((C,), 0.5), d.rand((C,), 0.5)
    c["w_dw"], c["w_stem"] = d.normal((C, 3, 3), 0.1, 0.4), d.normal((C, 3, 3, 3), 0.0, 0.3)
    return c


def sd_finalize(o, c):
    """pw_bnbwd_finalize_kernel on the five sums: (dW_s [32,27], dgamma_s, dbeta_s) and the magnitude of dW_s's terms"""
    M = float(c["M"])
    W = c["w_stem"].reshape(sr.SD_C, sr.SD_K)
    a = c["s_gamma"] * c["s_invstd"]
    b = -a * c["s_invstd"] * o["s2"] / M
    cc = -a * o["s1"] / M - b * c["s_mean"]
    dW = a[:, None] * o["P1"] + b[:, None] * (W @ o["gram"]) + cc[:, None] * o["colsum"][None, :]
    mag = (a[:, None] * o["P1"]).abs() + b.abs()[:, None] * (W.abs() @ o["gram"].abs()) + ((a * o["s1"] / M).abs() + (b * c["s_mean"]).abs())[:, None] * o["colsum"].abs()[None, :]
    return dW, o["s2"], o["s1"], mag


def sd_ref(c, m=None):
    C = sr.SD_C
    P = patches(c["x"])
    zd, zs = c["d"] * c["d_scale"] + c["d_shift"], c["s"] * c["s_scale"] + c["s_shift"]
    N, Ho, Wo, _ = zd.shape
    dYd = bn_dy(c["gd"], c["d"], c["d_scale"], c["d_shift"], c["d_act"], c["d_coef"])
    mag = bn_dy_mag(c["gd"], c["d"], c["d_scale"], c["d_shift"], c["d_act"], c["d_coef"])
    Gs = dref.conv_dx(dYd, c["w_dw"], 1, Ho, Wo)
    T = dref.conv_dx(mag, c["w_dw"].abs(), 1, Ho, Wo)
    a_s = act(zs, c["s_act"])
    mm = torch.ones(N, Ho, Wo, dtype=torch.float64) if m is None else m
    dz = Gs * dact(zs, c["s_act"]) * mm[..., None]
    T = T * mm[..., None]
    xhat = (c["s"] - c["s_mean"]) * c["s_invstd"]
    Pm = P * mm[..., None]
    P2, Pm2, Pa2 = P.reshape(-1, 27), Pm.reshape(-1, 27), P.abs().reshape(-1, 27)
    out = dict(dw_dw=dref.conv_dw(a_s * mm[..., None], dYd, 3, 1), s1=dz.sum((0, 1, 2)), s2=(dz * xhat).sum((0, 1, 2)), P1=dz.reshape(-1, C).t() @ P2,
               gram=Pm2.t() @ P2, colsum=Pm2.sum(0))
    terms = dict(dw_dw=dref.conv_dw(zs.abs() * mm[..., None], mag, 3, 1), s1=T.sum((0, 1, 2)), s2=(T * xhat.abs()).sum((0, 1, 2)), P1=T.reshape(-1, C).t() @ Pa2,
                 gram=Pm2.abs().t() @ Pa2, colsum=Pm2.abs().sum(0))
    return out, terms


def pj_act(r, mode):
    return sr.ACT_RELU if (mode == "exact" and r.act == sr.ACT_LEAKY) else r.act          # leaky's 0.1 is not exact


def pj_case(r, mode):
    d = Gen(_seed(r), mode == "exact")
    M, Ki, No = r.M, r.Ki, r.No
    c = dict(mode=mode, act=pj_act(r, mode))
    if mode == "exact":
        c["G"], c["Y"], c["D"] = d.ints((M, No), -1, 1), d.ints((M, No), -1, 1), d.ints((M, Ki), -2, 2)
        c["coef"] = torch.stack((d.ints((No,), 1, 2), d.ints((No,), -1, 1), d.ints((No,), -1, 1)))
        c["d_scale"], c["d_shift"] = torch.full((Ki,), 2.0, dtype=torch.float64), d.odd(Ki)
        # invstd 1 or 2; 1 alone on the 131 155-pixel rows, where sum |dz xhat| would pass 2^24 with 2
        c["d_mean"], c["d_invstd"] = d.ints((Ki,), -1, 1), 2.0 ** d.ints((Ki,), 0, 0 if Ki == 32 else 1)
        c["W"] = d.ints((No, Ki), -1, 1)
        return c
    c["G"], c["Y"] = d.normal((M, No), 0.5), d.normal((M, No))
    c["coef"] = torch.stack((d.rand((No,), 0.5), d.normal((No,), 0.0, 0.1), d.normal((No,), 0.0, 0.1)))
    c["d_scale"], c["d_shift"] = d.rand((Ki,), 0.5), d.normal((Ki,), 1.0, 0.5)
    c["D"] = d.off_kinks(d.normal((M, Ki), 0.5, 2.0), c["d_scale"], c["d_shift"], c["act"])
    c["d_mean"], c["d_invstd"] = d.normal((Ki,), 0.0, 0.2), d.rand((Ki,), 0.5)
    c["W"] = d.normal((No, Ki), 0.5 * Ki ** -0.5, Ki ** -0.5)
    return c


def pj_ref(c, m=None):
    """m: weight per pixel [M]"""
    dY = c["coef"][0] * c["G"] + c["coef"][1] * c["Y"] + c["coef"][2]
    mag = (c["coef"][0] * c["G"]).abs() + (c["coef"][1] * c["Y"]).abs() + c["coef"][2].abs()
    gd = dY @ c["W"]
    T = mag @ c["W"].abs()
    z = c["D"] * c["d_scale"] + c["d_shift"]
    if m is not None:
        dY, mag, gdm, T = dY * m[:, None], mag * m[:, None], gd * m[:, None], T * m[:, None]
    else:
        gdm = gd
    dz = gdm * dact(z, c["act"])
    xhat = (c["D"] - c["d_mean"]) * c["d_invstd"]
    out = dict(gd=gd, dw=dY.t() @ act(z, c["act"]), s1=dz.sum(0), s2=(dz * xhat).sum(0))
    terms = dict(dw=mag.t() @ z.abs(), s1=T.sum(0), s2=(T * xhat.abs()).sum(0))
    return out, terms


# ---- rounding budgets: |got - ref| <= k 2^-24 sum|terms| per reduced element.  Derived from the accumulation order of each kernel (the docstrings of
# tests/test_gpu_stem_trips.py carry the derivations); partial rows are combined in fp64 by the test, a combined output of the library is the fp64
# combine rounded once (+ 1). -------------------------------------------------------------------------------------------------------------------------
def stem_k(g, op):
    e = g.extra
    if g.form.startswith("stem_wgrad_mfma"):
        k = 64 * g.trips + 4                              # 16 instructions of 4 products per tile and wave, then the four waves
    elif g.form.startswith("stem_kernel"):
        k = g.trips + e["ppb"]                            # one step per pixel and trip, then the ppb accumulators of a channel group
    else:
        k = g.trips * e["cgn"] + e["ppb"]                 # cgn pixel passes per tile, then the 256 / cgn accumulators of a channel group
    return k + (7 if op == "bnwgrad" else 0)              # the rebuilt dY: z, act' (2), g act', two fmas, fp32 0.1 / 1/3 for the exact constant


def sd_k(g):
    TH = g.extra["TH"]
    chain = 5 + 9 + 2                                     # a dY_d value (z, g act', two fmas; fp32 0.1 for leaky's slope), the nine-tap scatter, the mask product (and its 0.1)
    mm = 8 * g.trips * TH + 4                             # two instructions of 4 products per row, tile and wave; the four waves
    return dict(dw_dw=g.trips * (TH + 1) + 32 + 3 + 5, s1=g.trips * TH + 32 + chain, s2=g.trips * TH + 32 + chain + 3, P1=mm + chain, gram=mm,
                colsum=2 * g.trips * TH + 2 + 4)


def pj_k(g, No):
    chain = 2 + No + 2                                    # dY (two fmas), No products of the data-gradient MFMA chain, the mask product (fp32 0.1 for leaky's slope)
    return dict(dw=16 * g.trips + 4 + 2 + 3, s1=4 * g.trips + 2 + 4 + chain, s2=4 * g.trips + 2 + 4 + chain + 3)
