"""MI355X: the BatchNorm kernels of csrc/bn_eltwise.hip, the partial-row combines of csrc/core.hip and the glue kernels, called
straight through the C ABI and held against the fp64 references of tests/bn_glue_ref.py.

These kernels are what the other GPU tests compare fused kernels WITH, so they are pinned here at every launch regime.  Two kinds
of input:

* exact: small integers, power-of-two scales / invstd, integer means, shift 0, and per activation a value grid on which the
  activation (or its derivative) is a dyadic number — every fp32 operation of the kernel and the bf16 store are then exact, and the
  result must EQUAL the reference.  These cases carry the indexing claims (a dropped / doubled row, a wrong channel or neighbour
  changes an integer).
* real: seeded normal data with a DERIVED bound, U = 2^-24 the fp32 unit roundoff:
    elementwise   k * U * sum|terms|            k = fp32 roundings on the path, stated at each kernel
    sums          (n + 4) * U * sum|term|       n = longest fp32 addition chain (rows per thread + rows per block)
    bf16 store    + 2^-8 * |ref|
  Every check prints `OBS <kernel> <largest error / bound>`; LAB_NOTES.md records the values seen on the MI355X."""
import ctypes
import math

import numpy as np
import pytest
import torch

import bn_glue_ref as R

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
U = 2.0 ** -24
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))       # the values the c_float arguments carry
SENT = 77.0                                                      # sentinel behind n (bf16-representable)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from mobilenet_yolo_pytorch_amd import _lib
    return _lib


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def K(name, bf):
    return name + "_bf16" if bf else name


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen(seed)).to(F64)


def pick(n, choices, seed):
    return torch.tensor(choices, dtype=F64)[torch.randint(0, len(choices), (n,), generator=gen(seed))]


def normal(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)).to(F64) * scale           # fp32 values


def put(x64, bf=False):
    """fp64 values -> (device tensor in the storage type, the stored values as fp64)."""
    t = x64.float().to(BF) if bf else x64.float()
    return t.cuda(), t.to(F64)


def par(x64):
    """A per-channel fp32 parameter: (device tensor, its values as fp64)."""
    return put(x64, False)


def empty(shape, bf=False):
    return torch.empty(tuple(shape), device="cuda", dtype=BF if bf else torch.float32)


def guarded(n, bf=False, fill=None):
    """n elements + 8 sentinels in ONE allocation."""
    t = torch.full((n + 8,), SENT, device="cuda", dtype=BF if bf else torch.float32)
    if fill is not None:
        t[:n] = fill
    return t


def sentinels_intact(t, n):
    return bool((t[n:] == SENT).all().item())


def close(name, got, ref, tol):
    name += " [bf16]" if got.dtype == BF else ""
    g = got.detach().to(F64).cpu().reshape(ref.shape)
    err = (g - ref).abs()
    tol = torch.as_tensor(tol, dtype=F64).expand_as(err)
    worst = (err / tol.clamp_min(1e-300)).max().item()
    print("OBS %-28s %.3f of the bound (max err %.3e)" % (name, worst, err.max().item()))
    assert torch.isfinite(g).all(), name
    assert (err <= tol).all(), "%s: %d elements over the bound, worst %.2f x" % (name, int((err > tol).sum()), worst)


def exact(name, got, ref):
    g = got.detach().to(F64).cpu().reshape(ref.shape)
    bad = g != ref
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r want %r" % (
        name, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), g[bad][0].item(), ref[bad][0].item())


def bf_tol(ref, bf):
    return 2.0 ** -8 * ref.abs() if bf else 0.0


def cg_ppb(C):
    """Rows per workgroup of the channel-group layout (4 channels per thread, <= 256 threads; scalar layout when C % 4 != 0)."""
    units = C // 4 if C % 4 == 0 else C
    chunks = -(-units // 256)
    return max(256 // -(-units // chunks), 1)


def exact_view(shape, act, seed):
    """(x, scale, shift = 0) on which act(scale * x) is exact in fp32: multiples of 10 for leaky (0.1f * 10k rounds to k),
    multiples of 4 for h-swish / h-sigmoid (values 0, 1/2, 1 of the gate), small integers otherwise; |view| <= 40."""
    C = shape[-1]
    if act == 2:
        return 10 * ints(shape, -2, 2, seed), pick(C, [1.0, 2.0], seed + 1), torch.zeros(C, dtype=F64)
    if act in (4, 5):
        return 4 * ints(shape, -2, 2, seed), pick(C, [1.0, 2.0], seed + 1), torch.zeros(C, dtype=F64)
    return ints(shape, -8, 8, seed), pick(C, [1.0, 2.0, 4.0], seed + 1), torch.zeros(C, dtype=F64)


def real_view(shape, seed):
    C = shape[-1]
    return normal(shape, seed, 1.5), 1 + 0.2 * normal((C,), seed + 1), 0.3 * normal((C,), seed + 2)


def job_table(rows, fields, block_job):
    jt = np.array(rows, dtype=np.dtype(fields))
    return torch.from_numpy(jt.view(np.uint8).copy()).cuda(), torch.tensor(block_job, dtype=torch.int32, device="cuda")


# ---- 1. partial-row combines ------------------------------------------------------------------------------------------------------------
PARTS = [1, 2, 31, 32, 33, 96, 97, 128, 129, 480, 481, 511, 512, 513, 544, 608, 609, 1023, 1024, 1025, 1537]


@pytest.mark.parametrize("C", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("parts", PARTS)
def test_partial_row_combines_exact(lib, parts, C):
    """mny_bn_finalize, mny_bn_bwd_finalize[_frozen]: integer rows (|v| <= 2048, sums < 2^24) -> mean, dbeta, dgamma bit-equal."""
    rows = ints((parts, 2, C), -2048, 2048, seed=parts * 131 + C)
    rd, _ = put(rows)
    s, q = rows[:, 0].sum(0), rows[:, 1].sum(0)
    count = 1000
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    scale, shift, mean, invstd = (torch.full((C,), SENT, device="cuda") for _ in range(4))
    lib.call("mny_bn_finalize", P(rd), parts, count, P(one), P(zero), EPS, MOM, None, None, P(scale), P(shift), P(mean), P(invstd), C, ST())
    exact("bn_finalize mean", mean, (s / count).float().to(F64))
    mu, _ = par(ints((C,), -3, 3, seed=5))
    istd, _ = par(pick(C, [0.5, 1.0, 2.0], seed=6))
    for name in ("mny_bn_bwd_finalize", "mny_bn_bwd_finalize_frozen"):
        dgamma, dbeta, coef = torch.full((C,), SENT, device="cuda"), torch.full((C,), SENT, device="cuda"), torch.empty(3, C, device="cuda")
        lib.call(name, P(rd), parts, count, P(one), P(mu), P(istd), P(dgamma), P(dbeta), P(coef), C, ST())
        exact(name + " dbeta", dbeta, s.float().to(F64))
        exact(name + " dgamma", dgamma, q.float().to(F64))


def test_reduce_batch_exact(lib):
    """mny_reduce_batch: every (nparts, n) pair below as one job of ONE launch; integer rows, bit-equal, sentinels behind each n."""
    NP, NS = [1, 7, 8, 9, 24, 25, 32, 33, 57, 300], [1, 31, 32, 33, 288, 1000]
    jobs, block_job, keep = [], [], []
    for i, nparts in enumerate(NP):
        for j, n in enumerate(NS):
            rows = ints((nparts, n), -2048, 2048, seed=1000 + i * 10 + j)
            rd, _ = put(rows)
            out = guarded(n)
            jobs.append((rd.data_ptr(), out.data_ptr(), n, nparts, len(block_job)))
            block_job += [len(jobs) - 1] * ((n + 31) // 32)
            keep.append((rows, rd, out, n))
    jd, bj = job_table(jobs, [("parts", np.uint64), ("out", np.uint64), ("n", np.int64), ("nparts", np.int32), ("b0", np.int32)], block_job)
    lib.call("mny_reduce_batch", P(jd), P(bj), len(block_job), ST())
    torch.cuda.synchronize()
    assert len(jobs) >= 6
    for rows, _, out, n in keep:
        exact("reduce_batch nparts %d n %d" % (rows.shape[0], n), out[:n], rows.sum(0))
        assert sentinels_intact(out, n)


def test_reduce_batch_real(lib):
    """Normal rows: the combine is fp64 with one final rounding -> 2 * U * |ref| (k = 1, doubled for the fp64 order of additions)."""
    jobs, block_job, keep = [], [], []
    for i, (nparts, n) in enumerate([(7, 33), (25, 288), (33, 1000), (57, 31), (300, 32), (1, 1)]):
        rd, rows = put(normal((nparts, n), seed=1100 + i, scale=30.0))
        out = guarded(n)
        jobs.append((rd.data_ptr(), out.data_ptr(), n, nparts, len(block_job)))
        block_job += [i] * ((n + 31) // 32)
        keep.append((rows, rd, out, n))
    jd, bj = job_table(jobs, [("parts", np.uint64), ("out", np.uint64), ("n", np.int64), ("nparts", np.int32), ("b0", np.int32)], block_job)
    lib.call("mny_reduce_batch", P(jd), P(bj), len(block_job), ST())
    torch.cuda.synchronize()
    for rows, _, out, n in keep:
        close("reduce_batch", out[:n], rows.sum(0), 2 * U * rows.abs().sum(0))
        assert sentinels_intact(out, n)


def _bn_finalize(lib, rd, parts, count, gamma, beta, C, rm=None, rv=None, stats=True):
    scale, shift = empty((C,)), empty((C,))
    mean, invstd = (empty((C,)), empty((C,))) if stats else (None, None)
    lib.call("mny_bn_finalize", P(rd), parts, count, P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(scale), P(shift), P(mean), P(invstd), C, ST())
    return scale, shift, mean, invstd


@pytest.mark.parametrize("parts,C,per", [(97, 100, 10), (513, 33, 8), (1537, 32, 3), (1, 1, 50)])
def test_bn_finalize_real_rows(lib, parts, C, per):
    """scale / shift / mean / invstd / running statistics against fp64.  After the fp64 combine: mean 1 rounding, invstd 1, scale 2,
    shift 4 (mean, product, difference, scale's own), running statistics 4 (1 - m, two products, sum) -> 8 * U * sum|terms| covers each."""
    x = normal((parts, per, C), seed=parts, scale=2.0) + 0.7
    rd, rows = put(torch.stack((x.sum(1), (x * x).sum(1)), 1))
    count = parts * per
    (gamma, g64), (beta, b64) = par(1 + 0.3 * normal((C,), 2)), par(0.2 * normal((C,), 3))
    (rm, rm64), (rv, rv64) = par(0.3 * normal((C,), 4)), par(0.5 + normal((C,), 5).abs())
    scale, shift, mean, invstd = _bn_finalize(lib, rd, parts, count, gamma, beta, C, rm, rv)
    r = R.bn_finalize_ref(rows, count, g64, b64, EPS, MOM, rm64, rv64)
    close("bn_finalize scale", scale, r[0], 8 * U * r[0].abs())
    close("bn_finalize shift", shift, r[1], 8 * U * (b64.abs() + (r[2] * r[0]).abs()))
    close("bn_finalize mean", mean, r[2], 8 * U * r[2].abs())
    close("bn_finalize invstd", invstd, r[3], 8 * U * r[3].abs())
    close("bn_finalize running_mean", rm, r[4], 8 * U * ((1 - MOM) * rm64.abs() + MOM * r[2].abs()))
    close("bn_finalize running_var", rv, r[5], 8 * U * r[5].abs())
    # optional outputs: leaving them out changes nothing else
    s2, h2, m2, i2 = _bn_finalize(lib, rd, parts, count, gamma, beta, C)
    assert torch.equal(s2, scale) and torch.equal(h2, shift) and torch.equal(m2, mean) and torch.equal(i2, invstd)
    rm3, rv3 = par(rm64)[0], par(rv64)[0]
    s3, h3, _, _ = _bn_finalize(lib, rd, parts, count, gamma, beta, C, rm3, rv3, stats=False)
    assert torch.equal(s3, scale) and torch.equal(h3, shift) and torch.equal(rm3, rm) and torch.equal(rv3, rv)


def test_bn_finalize_count_one_and_negative_variance(lib):
    """count = 1: the running variance takes the BIASED value (there is no unbiased one).  A constant channel whose rounded sums give
    q / count - mean^2 < 0 in fp64: the variance is clamped to 0, invstd = 1 / sqrt(eps)."""
    rd, rows = put(torch.tensor([[[2.0, -1.0], [4.5, 0.5]]], dtype=F64))
    (gamma, g64), (beta, b64) = par(torch.tensor([1.5, 0.5], dtype=F64)), par(torch.tensor([0.25, -1.0], dtype=F64))
    (rm, rm64), (rv, rv64) = par(torch.tensor([0.5, 0.5], dtype=F64)), par(torch.tensor([1.0, 2.0], dtype=F64))
    scale, shift, mean, invstd = _bn_finalize(lib, rd, 1, 1, gamma, beta, 2, rm, rv)
    r = R.bn_finalize_ref(rows, 1, g64, b64, EPS, MOM, rm64, rv64)
    assert torch.isfinite(rv).all()
    close("bn_finalize count=1 running_var", rv, r[5], 8 * U * r[5].abs())
    close("bn_finalize count=1 invstd", invstd, r[3], 8 * U * r[3].abs())
    exact("bn_finalize count=1 mean", mean, r[2])

    parts, per = 16, 256
    const = None
    for cand in (1000.1, 1000.2, 1000.3, 1000.7, 999.9, 1001.1):
        x = float(np.float32(cand))
        sq = float(np.float32(x * x))                                 # the fp32 square a producer accumulates; x 256 is exact
        if (parts * per * sq) / (parts * per) - x * x < 0.0:
            const = cand
            break
    assert const is not None, "no candidate constant gives a negative fp64 variance"
    x = float(np.float32(const))
    rows = torch.empty(parts, 2, 2, dtype=F64)
    rows[:, 0, 0], rows[:, 1, 0] = per * x, per * float(np.float32(x * x))
    data = normal((parts, per), seed=9)
    rows[:, 0, 1], rows[:, 1, 1] = data.sum(1), (data * data).sum(1)
    rd, rows = put(rows)
    count = parts * per
    s, q = rows[:, 0, 0].sum().item(), rows[:, 1, 0].sum().item()
    assert q / count - (s / count) ** 2 < 0.0                           # really negative on the fp32 rows
    scale, shift, mean, invstd = _bn_finalize(lib, rd, parts, count, gamma, beta, 2)
    assert invstd[0].item() == float(np.float32(1.0 / math.sqrt(EPS)))
    assert mean[0].item() == x
    r = R.bn_finalize_ref(rows, count, g64, b64, EPS, MOM)
    close("bn_finalize clamped scale", scale, r[0], 8 * U * r[0].abs())
    close("bn_finalize clamped invstd", invstd, r[3], 8 * U * r[3].abs())


@pytest.mark.parametrize("parts,C,count", [(97, 100, 968), (513, 33, 4101), (1024, 32, 100000), (2, 1, 7)])
def test_bn_bwd_finalize_real_rows(lib, parts, C, count):
    """coef / dgamma / dbeta against fp64: everything is formed in fp64 and rounded once (k = 1); 8 * U * sum|terms| as for the forward."""
    rd, rows = put(normal((parts, 2, C), seed=parts + 1, scale=5.0))
    (gamma, g64), (mu, mu64), (istd, i64) = par(1 + 0.3 * normal((C,), 2)), par(0.4 * normal((C,), 3)), par(0.5 + normal((C,), 4).abs())
    s, q = rows[:, 0].sum(0), rows[:, 1].sum(0)
    out = {}
    for name in ("mny_bn_bwd_finalize", "mny_bn_bwd_finalize_frozen"):
        dgamma, dbeta, coef = empty((C,)), empty((C,)), torch.full((3, C), SENT, device="cuda")
        lib.call(name, P(rd), parts, count, P(gamma), P(mu), P(istd), P(dgamma), P(dbeta), P(coef), C, ST())
        out[name] = (dgamma, dbeta, coef)
        close(name + " dbeta", dbeta, s, 2 * U * rows[:, 0].abs().sum(0))
        close(name + " dgamma", dgamma, q, 2 * U * rows[:, 1].abs().sum(0))
    coef = out["mny_bn_bwd_finalize"][2]
    close("bn_bwd_finalize coef", coef, R.bn_bwd_coef_ref(s, q, count, g64, mu64, i64), 8 * U * R.bn_bwd_coef_mag(s, q, count, g64, mu64, i64))
    fz = out["mny_bn_bwd_finalize_frozen"]
    exact("frozen coef[0]", fz[2][0], (g64 * i64).float().to(F64))
    assert (fz[2][1:] == 0).all(), "frozen BatchNorm: cb, cc are zeros (of either sign)"
    assert torch.equal(fz[0], out["mny_bn_bwd_finalize"][0]) and torch.equal(fz[1], out["mny_bn_bwd_finalize"][1])


# ---- 2. mny_bn_bwd_reduce / _apply at every launch regime ---------------------------------------------------------------------------------
REGIMES = [(4, 1), (4, 255), (4, 257),                       # single channel group, 256 rows per block, ragged block
           (24, 43), (24, 1000),                             # 252 threads: block not a multiple of 64
           (516, 1024), (516, 1025), (516, 2051),            # 129 groups, 1 row per block: reduce cap (1024 blocks), second trip
           (516, 3072), (516, 3073), (516, 4101),            # bf16 four-rows-in-flight loop: not entered / by one block / plus tail
           (516, 8197),                                      # apply cap (8192 blocks), second trip
           (1028, 5),                                        # 2 chunks x 129 groups, one dead lane (cg >= cg_total)
           (1280, 7),                                        # the widest layer: 2 chunks x 160
           (10, 105), (10, 51207),                           # scalar kernels, 25 rows per block: second trip of the reduce
           (10, 209720),                                     # scalar apply cap (8192 * 256 elements)
           (257, 3), (258, 3)]                               # scalar, 2 chunks x 129: dead lane / full last chunk


@pytest.mark.parametrize("C,M", [(516, 8197), (10, 209720)])
def test_regimes_take_a_second_trip(lib, C, M):
    """The partial-row count saturates: half the rows already fill the grid, so the grid-stride loop runs at least twice at M."""
    assert lib.query("mny_bn_bwd_parts", M, C) == lib.query("mny_bn_bwd_parts", M // 2, C)


def _bwd_inputs(C, M, act, kind, seed):
    """g, y, scale, shift, mean, invstd, gamma, hand-made coef (fp64, before storage rounding)."""
    if kind == "exact":
        # dz = g * act'(z) must be an integer with no rounding anywhere (the reduce kernel contracts g * act' into the running sum's
        # fma, so a rounded product does not do): act' in {0, 1} (none, relu6, relu; leaky on positive z) or {0, 1/2, 1} (h-swish on
        # z in 4Z, g even)
        assert act in (0, 1, 2, 3, 4)
        g = ints((M, C), -5, 5, seed) * (2 if act == 4 else 1)
        y = 4 * ints((M, C), -2, 2, seed + 1) if act == 4 else ints((M, C), 1, 8, seed + 1) if act == 2 else ints((M, C), -8, 8, seed + 1)
        scale = pick(C, [1.0, 2.0] if act == 4 else [1.0, 2.0, 4.0], seed + 2)
        shift = torch.zeros(C, dtype=F64)
        mean, invstd = ints((C,), -3, 3, seed + 3), pick(C, [0.5, 1.0, 2.0], seed + 4)
        gamma = pick(C, [0.5, 1.0, 2.0], seed + 5)
        coef = torch.stack((pick(C, [1.0, 2.0], seed + 6), pick(C, [-1.0, 1.0], seed + 7), ints((C,), -2, 2, seed + 8)))
    else:
        g, y = normal((M, C), seed), normal((M, C), seed + 1, 1.5)
        scale, shift = 1 + 0.2 * normal((C,), seed + 2), 0.3 * normal((C,), seed + 3)
        mean, invstd = 0.2 * normal((C,), seed + 4), 0.5 + normal((C,), seed + 5).abs()
        gamma = 1 + 0.3 * normal((C,), seed + 6)
        coef = None
    return g, y, scale, shift, mean, invstd, gamma, coef


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("idx", range(len(REGIMES)), ids=["C%d-M%d" % cm for cm in REGIMES])
def test_bn_backward_regimes(lib, idx, kind, bf):
    """reduce -> (fp64 sum of the partial rows == reference sums) -> mny_bn_bwd_finalize -> apply with those coefficients: the chain the
    plans run.  Activations cycle with the case, 3 + times each per storage type.  The leaky slope 0.1 and the gate's 1/6 are no dyadic
    numbers, so no input makes g * act' exact there: the exact cases run leaky on positive pre-activations and relu6 in h-sigmoid's
    place; both derivatives are held by the real cases and by test_activation_derivative_at_the_kinks.

    real sums: (n + 4) * U * sum|term|, n = rows per thread + rows per block (the thread's running sum, then the block's serial sum
    over its rows); the 4 = product g * act', y - mean, * invstd, fma.
    real apply: dy = fma(ca, g * act'(z), fma(cb, y, cc)); act'(z) of h-swish carries z's rounding (2 by terms), its own fma and the
    1/3 constant (1.5); then the product with g (1) and the two fma (2): <= 6.5 -> k = 8 on sum|terms|.
    A pre-activation within an fp32 ulp of a kink at +-3 or 6 may take the other branch in fp32: such elements (at most 1e-5 of a
    case, asserted) get the derivative's jump (<= 1) times |g| as slack, in the sums and in dy."""
    C, M = REGIMES[idx]
    act = (idx + 3 * bf) % 6
    if kind == "exact" and act == 5:
        act = 1
    g64, y64, sc64, sh64, mu64, is64, ga64, hand = _bwd_inputs(C, M, act, kind, seed=100 * idx + bf)
    (g, g64), (y, y64) = put(g64, bf), put(y64, bf)
    (sc, sc64), (sh, sh64), (mu, mu64), (istd, is64), (gamma, ga64) = par(sc64), par(sh64), par(mu64), par(is64), par(ga64)
    slack = R.kink_ambiguous(y64 * sc64 + sh64, act) * g64.abs()          # scale = NULL: z = y is exact, no slack there
    if kind == "real":
        assert (slack != 0).double().mean().item() <= 1e-5

    parts = lib.query("mny_bn_bwd_parts", M, C)
    red = torch.full((parts, 2, C), SENT, device="cuda")
    lib.call(K("mny_bn_bwd_reduce", bf), P(g), P(y), P(sc), P(sh), act, P(mu), P(istd), P(red), M, C, ST())
    rows = red.to(F64).cpu()
    s, q, sa, qa = R.bn_bwd_sums_ref(g64, y64, sc64, sh64, act, mu64, is64)
    gs, gq = rows[:, 0].sum(0), rows[:, 1].sum(0)
    dgamma, dbeta, coef = empty((C,)), empty((C,)), empty((3, C))
    lib.call("mny_bn_bwd_finalize", P(red), parts, M, P(gamma), P(mu), P(istd), P(dgamma), P(dbeta), P(coef), C, ST())
    if kind == "exact":
        exact("bn_bwd_reduce sum dz", gs, s)
        exact("bn_bwd_reduce sum dz*yhat", gq, q)
        exact("chain dbeta", dbeta, s.float().to(F64))
        exact("chain dgamma", dgamma, q.float().to(F64))
    else:
        ppb = cg_ppb(C)
        n = -(-M // (parts * ppb)) + ppb
        close("bn_bwd_reduce sum dz", gs, s, (n + 4) * U * sa + slack.sum(0))
        close("bn_bwd_reduce sum dz*yhat", gq, q, (n + 4) * U * qa + (slack * ((y64 - mu64) * is64).abs()).sum(0))
        close("chain dbeta", dbeta, gs, 2 * U * rows[:, 0].abs().sum(0))
        close("chain dgamma", dgamma, gq, 2 * U * rows[:, 1].abs().sum(0))
    close("chain coef", coef, R.bn_bwd_coef_ref(gs, gq, M, ga64, mu64, is64), 8 * U * R.bn_bwd_coef_mag(gs, gq, M, ga64, mu64, is64))

    cf, cf64 = (coef, coef.to(F64).cpu()) if hand is None else par(hand)
    for what, (s_, h_, s64, h64), (c_, c64) in (("apply", (sc, sh, sc64, sh64), (cf, cf64)),
                                                ("apply scale=NULL", (None, None, None, None), (cf, cf64)),
                                                ("apply coef=NULL", (sc, sh, sc64, sh64), (None, None))):
        dy = torch.full((M, C), SENT, device="cuda", dtype=BF if bf else torch.float32)
        lib.call(K("mny_bn_bwd_apply", bf), P(g), P(y), P(s_), P(h_), act, P(c_), P(dy), M, C, ST())
        ref = R.bn_bwd_apply_ref(g64, y64, s64, h64, act, c64)
        if kind == "exact":
            exact("bn_bwd_" + what, dy, ref)
        else:
            jump = 0 if s64 is None else slack * (c64[0].abs() if c64 is not None else 1.0)
            close("bn_bwd_" + what, dy, ref, 8 * U * R.bn_bwd_apply_mag(g64, y64, s64, h64, act, c64) + bf_tol(ref, bf) + jump)


KINK_Y = [-3.0, -2.0 ** -20, 0.0, 2.0 ** -20, 3.0, 6.0, 6 + 2.0 ** -20, -6.0]


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", range(R.N_ACTS))
def test_activation_derivative_at_the_kinks(lib, act, bf):
    """dz = g * act'(y) with scale = 1, shift = 0 and y ON the kinks (and 2^-20 beside them) equals torch's fp64 autograd bit for bit.
    g = +-2^k, so the product is exact and the derivative itself is what is compared.  C = 8 runs the float4 kernel, C = 10 the scalar one.

    h-swish' was (2z + 3) * (1/6) in two roundings and missed the fp64 value by one fp32 ulp at z = +-2^-20 (32 of 128 elements of this
    case, fp32 storage); it is now the single fma z / 3 + 1 / 2 everywhere (csrc/common.h act_bwd)."""
    for C in (8, 10):
        M = 16
        idx = torch.arange(M).view(M, 1) + 3 * torch.arange(C).view(1, C)
        (y, y64) = put(torch.tensor(KINK_Y, dtype=F64)[idx % 8], bf)
        (g, g64) = put(torch.tensor([1.0, -2.0, 0.5, 4.0, -0.25], dtype=F64)[(idx // 2) % 5], bf)
        ref = g64 * R.act_grad(y64, act)
        ref = ref.float().to(F64) if not bf else torch.from_numpy(R.to_bf16_rne(ref.numpy()))
        one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        for s_, h_ in ((None, None), (one, zero)):
            dz = torch.full((M, C), SENT, device="cuda", dtype=BF if bf else torch.float32)
            lib.call(K("mny_bn_bwd_apply", bf), P(g), P(y), P(s_), P(h_), act, None, P(dz), M, C, ST())
            exact("act_bwd act %d C %d" % (act, C), dz, ref)


# ---- 3. glue ----------------------------------------------------------------------------------------------------------------------------------
NHWC = [(1, 2, 2, 4), (3, 6, 10, 24), (2, 4, 6, 1028), (1, 2, 4100, 516)]       # the last: 8200 rows, past the 8192-block cap, wraps the image row
# (b, up, act of a's view, act of b's view); None = no view (NULL scale, MNY_ACT_NONE)
ADD_CFG = [(0, 0, 0, None), (0, 0, 4, None), (1, 0, None, 1), (1, 0, 2, 5), (0, 1, 3, None), (0, 1, None, None), (1, 1, 1, 2), (1, 1, None, 3), (1, 1, 5, 4)]


def _operand(shape, act, kind, bf, seed, amp=8):
    """One viewed operand: device tensors, stored fp64 values, and the (scale, shift, act) triple for the reference."""
    if act is None:
        x64 = ints(shape, -amp, amp, seed) if kind == "exact" else normal(shape, seed, 1.5)
        x, x64 = put(x64, bf)
        return (x, None, None, 0), (x64, (None, None, 0))
    x64, sc64, sh64 = exact_view(shape, act, seed) if kind == "exact" else real_view(shape, seed)
    (x, x64), (sc, sc64), (sh, sh64) = put(x64, bf), par(sc64), par(sh64)
    return (x, sc, sh, act), (x64, (sc64, sh64, act))


def _coarse(N, H, W, C, kind, bf, seed):
    """The half-resolution operand of a nearest-2x upsample.  exact: a value that encodes (n, h, w, c) — the linear index in fp32
    storage, a hash whose neighbours in h, w and c all differ in bf16 storage (8 significant bits)."""
    shape = (N, H // 2, W // 2, C)
    if kind == "real":
        return put(normal(shape, seed), bf)
    n, h, w, c = torch.meshgrid(*(torch.arange(k) for k in shape), indexing="ij")
    v = (7 * n + 3 * h + 5 * w + c) % 17 - 8 if bf else ((n * shape[1] + h) * shape[2] + w) * C + c
    return put(v.to(F64), bf)


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("shape", NHWC, ids=["x".join(map(str, s)) for s in NHWC])
def test_add_views(lib, shape, kind, bf):
    """real: a view costs <= 5 roundings on view_mag (z; z + 3, the 1/6 constant and product, z * h), the two additions 1 each on
    the partial sums -> k = 8 on the sum of the operands' magnitudes."""
    N, H, W, C = shape
    for i, (use_b, use_up, a_act, b_act) in enumerate(ADD_CFG):
        a, (a64, av) = _operand(shape, a_act, kind, bf, seed=10 * i + 1)
        b, (b64, bv) = _operand(shape, b_act, kind, bf, seed=10 * i + 5) if use_b else ((None, None, None, 0), (None, None))
        up, up64 = _coarse(N, H, W, C, kind, bf, seed=10 * i + 9) if use_up else (None, None)
        out = torch.full(shape, SENT, device="cuda", dtype=BF if bf else torch.float32)
        lib.call(K("mny_add_views", bf), P(a[0]), P(a[1]), P(a[2]), a[3], P(b[0]), P(b[1]), P(b[2]), b[3], P(up), P(out), N, H, W, C, ST())
        ref = R.add_views_ref(a64, av, b64, bv, up64)
        if kind == "exact":
            exact("add_views cfg %d" % i, out, ref)
        else:
            mag = R.view_mag(a64, *av) + (R.view_mag(b64, *bv) if use_b else 0) + (R.upsample2x(up64).abs() if use_up else 0)
            close("add_views", out, ref, 8 * U * mag + bf_tol(ref, bf))


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("shape", NHWC, ids=["x".join(map(str, s)) for s in NHWC])
def test_upsample_bwd(lib, shape, kind, bf):
    """real: four (five when accumulating) serial additions -> k = 5 on sum|terms|."""
    N, H, W, C = shape
    src, s64 = put(ints(shape, -8, 8, 1) if kind == "exact" else normal(shape, 1), bf)
    cshape = (N, H // 2, W // 2, C)
    d0, d64 = put(ints(cshape, -8, 8, 2) if kind == "exact" else normal(cshape, 2), bf)
    for acc in (0, 1):
        dst = d0.clone() if acc else torch.full(cshape, SENT, device="cuda", dtype=d0.dtype)
        lib.call(K("mny_upsample_bwd", bf), P(src), P(dst), acc, N, H, W, C, ST())
        ref = R.upsample_bwd_ref(s64, d64 if acc else None)
        if kind == "exact":
            exact("upsample_bwd acc %d" % acc, dst, ref)
        else:
            mag = R.upsample_bwd_ref(s64.abs(), d64.abs() if acc else None)
            close("upsample_bwd", dst, ref, 5 * U * mag + bf_tol(ref, bf))


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("M,C", [(1, 516), (257, 516), (8197, 516), (5, 1028)])
def test_mul_views_and_backward(lib, M, C, kind, bf):
    """out = addend + view(a) * view(b) as one fma.  real: 5 roundings per view, 1 for the fma -> 12 * U * mag(a) * mag(b) + 2 * U * |addend|."""
    shape = (M, C)
    add, add64 = put(ints(shape, -4, 4, 7) if kind == "exact" else normal(shape, 7), bf)
    # exact: every product plus the addend stays an integer (or half) below 256, i.e. within bf16's 8 significant bits
    for i, (a_act, b_act) in enumerate([(None, 5), (3, 5), (4, None), (2, 1), (None, 4), (0, 5)]):
        a, (a64, av) = _operand(shape, a_act, kind, bf, seed=20 * i + 1, amp=4)
        b, (b64, bv) = _operand(shape, b_act, kind, bf, seed=20 * i + 5, amp=4)
        out = torch.full(shape, SENT, device="cuda", dtype=BF if bf else torch.float32)
        lib.call(K("mny_mul_views", bf), P(a[0]), P(a[1]), P(a[2]), a[3], P(b[0]), P(b[1]), P(b[2]), b[3], P(out), M, C, ST())
        ref = R.mul_views_ref(a64, av, b64, bv)
        mag = 12 * U * R.view_mag(a64, *av) * R.view_mag(b64, *bv)
        if kind == "exact":
            exact("mul_views cfg %d" % i, out, ref)
        else:
            close("mul_views", out, ref, mag + bf_tol(ref, bf))
        # backward: the raw gradient (a's tensor, no view) times the view of the other operand, with and without an addend
        g, g64 = a[0], a64
        for addend, addend64 in ((None, None), (add, add64)):
            dst = torch.full(shape, SENT, device="cuda", dtype=BF if bf else torch.float32)
            lib.call(K("mny_mul_views_bwd", bf), P(g), P(b[0]), P(b[1]), P(b[2]), b[3], P(addend), P(dst), M, C, ST())
            ref = R.mul_views_bwd_ref(g64, b64, bv, addend64)
            if kind == "exact":
                exact("mul_views_bwd cfg %d" % i, dst, ref)
            else:
                tol = 12 * U * g64.abs() * R.view_mag(b64, *bv) + (2 * U * addend64.abs() if addend is not None else 0)
                close("mul_views_bwd", dst, ref, tol + bf_tol(ref, bf))


PARTADD = [(4, 4, (1, 4, 6)), (16, 40, (1, 4, 6)), (40, 1028, (1, 4, 6)), (512, 516, (1, 4, 6)), (512, 516, (1, 2, 4100))]


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("Ca,Cb,nhw", PARTADD, ids=["%d-%d-M%d" % (a, b, n * h * w) for a, b, (n, h, w) in PARTADD])
def test_partadd_up_and_slice_channels(lib, Ca, Cb, nhw, kind, bf):
    """real: the view (5) and one addition -> k = 8 on the operands' magnitudes; the slice is one addition (k = 1, 2 used)."""
    N, H, W = nhw
    M = N * H * W
    for act in (None, 1, 4):
        a, (a64, av) = _operand((N, H, W, Ca), act, kind, bf, seed=3 + (act or 0))
        up, up64 = _coarse(N, H, W, Cb, kind, bf, seed=4)
        out = torch.full((N, H, W, Cb), SENT, device="cuda", dtype=BF if bf else torch.float32)
        lib.call(K("mny_partadd_up", bf), P(a[0]), P(a[1]), P(a[2]), a[3], P(up), P(out), N, H, W, Ca, Cb, ST())
        ref = R.partadd_up_ref(a64, av, up64)
        if kind == "exact":
            exact("partadd_up", out, ref)
        else:
            mag = R.upsample2x(up64).abs()
            mag[..., :Ca] += R.view_mag(a64, *av)
            close("partadd_up", out, ref, 8 * U * mag + bf_tol(ref, bf))
    src, s64 = put(ints((M, Cb), -8, 8, 5) if kind == "exact" else normal((M, Cb), 5), bf)
    d0, d64 = put(ints((M, Ca), -8, 8, 6) if kind == "exact" else normal((M, Ca), 6), bf)
    for acc in (0, 1):
        dst = d0.clone() if acc else torch.full((M, Ca), SENT, device="cuda", dtype=d0.dtype)
        lib.call(K("mny_slice_channels", bf), P(src), P(dst), acc, M, Ca, Cb, ST())
        ref = R.slice_channels_ref(s64, Ca, d64 if acc else None)
        if kind == "exact":
            exact("slice_channels acc %d" % acc, dst, ref)
        else:
            close("slice_channels", dst, ref, 2 * U * (s64[:, :Ca].abs() + d64.abs()) + bf_tol(ref, bf))


NS = [1, 2, 3, 4, 5, 1023, 1024, 8388608 + 1027]                    # the last is past the 8192 x 256 float4 grid cap


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("n", NS)
def test_axpy(lib, n, kind, bf):
    """dst = [dst +] alpha * src.  real: one fma in the float4 body, product and sum in the tail -> k = 2 on |alpha * src| + |dst|."""
    src, s64 = put(ints((n,), -16, 16, 1) if kind == "exact" else normal((n,), 1), bf)
    d64 = put(ints((n,), -8, 8, 2) if kind == "exact" else normal((n,), 2), bf)[1]
    al, al64 = par(torch.tensor([0.5 if kind == "exact" else 0.37], dtype=F64))
    for alpha, a64 in ((None, None), (al, al64.item())):
        for acc in (0, 1):
            dst = guarded(n, bf, d64.to(BF if bf else torch.float32).cuda())
            lib.call(K("mny_axpy", bf), P(src), P(alpha), P(dst), acc, n, ST())
            ref = R.axpy_ref(s64, a64, d64 if acc else None)
            name = "axpy alpha %s acc %d" % ("given" if alpha is not None else "NULL", acc)
            if kind == "exact":
                exact(name, dst[:n], ref)
            else:
                mag = s64.abs() * (abs(a64) if a64 is not None else 1.0) + (d64.abs() if acc else 0)
                close("axpy", dst[:n], ref, 2 * U * mag + bf_tol(ref, bf))
            assert sentinels_intact(dst, n), name


SPECIAL = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0, float("inf"), float("-inf"), 3.4028234663852886e38, float("nan"),
           257.0, 2.0 ** -20 * (1 + 2.0 ** -8), -3.3895313892515355e38]


def _cvt_input(n, seed):
    x = torch.randn(n, generator=gen(seed)) * torch.exp2(torch.randint(-20, 20, (n,), generator=gen(seed + 1)).float())
    k = min(n, len(SPECIAL))
    x[:k] = torch.tensor(SPECIAL[:k])
    if n > len(SPECIAL) + 3:
        x[-3:] = torch.tensor([1 + 2.0 ** -8, float("nan"), -(1 + 3 * 2.0 ** -8)])     # the scalar tail path sees ties too
    return x


def _same(a, b):
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(b.float())
    return torch.equal(torch.isnan(a.float()), nan) and torch.equal(a[~nan], b[~nan])


@pytest.mark.parametrize("n", NS)
def test_cvt(lib, n):
    """mny_cvt_f32_bf16 rounds like torch (nearest even; ties, +-0, +-inf, the largest finite float, NaN); mny_cvt_bf16_f32 widens exactly."""
    f = _cvt_input(n, seed=n % 1000).cuda()
    h = guarded(n, True)
    lib.call("mny_cvt_f32_bf16", P(f), P(h), n, ST())
    assert _same(h[:n], f.to(BF)) and sentinels_intact(h, n)
    f2 = guarded(n)
    lib.call("mny_cvt_bf16_f32", P(h), P(f2), n, ST())
    assert _same(f2[:n], h[:n].float()) and sentinels_intact(f2, n)


def test_cvt_batch(lib):
    jobs, block_job, keep = [], [], []
    for i, n in enumerate([1, 4095, 4096, 4097, 12289]):
        f = _cvt_input(n, seed=50 + i).cuda()
        h = guarded(n, True)
        jobs.append((f.data_ptr(), h.data_ptr(), n, len(block_job), 0))
        block_job += [i] * ((n + 4095) // 4096)
        keep.append((f, h, n))
    jd, bj = job_table(jobs, [("src", np.uint64), ("dst", np.uint64), ("n", np.int64), ("b0", np.int32), ("pad", np.int32)], block_job)
    lib.call("mny_cvt_batch_f32_bf16", P(jd), P(bj), len(block_job), ST())
    torch.cuda.synchronize()
    for f, h, n in keep:
        assert _same(h[:n], f.to(BF)), n
        assert sentinels_intact(h, n), n


def _bits_zero(t):
    if t.numel() == 0:
        return True
    return bool((t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32) == 0).all().item())


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,Cp", [(75, 76), (75, 80), (18, 18), (1, 4)])
def test_pad_rows(lib, C, Cp, bf):
    """[M][C] fp32 (times *alpha) -> [M][Cp] of the storage type, pad columns +0.  alpha NULL is a copy (bf16: ONE rounding, bit-equal
    to to_bf16_rne); alpha given: the fp32 product (k = 1) then the store."""
    for M in (1, 363, 30000):                                           # 30000 x 80 elements is past the 8192 x 256 grid cap
        for kind in ("exact", "real"):
            src, s64 = put(ints((M, C), -16, 16, M) if kind == "exact" else normal((M, C), M))
            al, al64 = par(torch.tensor([0.5 if kind == "exact" else 0.37], dtype=F64))
            for alpha, a64 in ((None, None), (al, al64.item())):
                dst = guarded(M * Cp, bf)
                lib.call(K("mny_pad_rows", bf), P(src), P(alpha), P(dst), M, C, Cp, ST())
                got = dst[:M * Cp].view(M, Cp)
                ref = R.pad_rows_ref(s64, a64, Cp)
                if kind == "exact" or alpha is None:
                    exact("pad_rows", got, torch.from_numpy(R.to_bf16_rne(ref.numpy())) if bf else ref)
                else:
                    close("pad_rows", got, ref, U * ref.abs() + bf_tol(ref, bf))
                assert _bits_zero(got[:, C:]) and sentinels_intact(dst, M * Cp)


@pytest.mark.parametrize("bf", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("R_,Cc,Rp", [(75, 1024, 76), (75, 512, 80), (33, 31, 33), (1, 1, 4)])
def test_transpose_pad(lib, R_, Cc, Rp, bf):
    """dst[c][r] = src[r][c] with row pitch Rp, pad columns +0: a copy, so bit-equal (bf16: to_bf16_rne of the fp32 value)."""
    for kind in ("exact", "real"):
        src, s64 = put(ints((R_, Cc), -64, 64, 3) if kind == "exact" else normal((R_, Cc), 3))
        for Rq, name in ((Rp, "mny_transpose_pad"), (R_, "mny_transpose")):
            dst = guarded(Cc * Rq, bf)
            args = (P(src), P(dst), R_, Cc) + ((Rq,) if name == "mny_transpose_pad" else ()) + (ST(),)
            lib.call(K(name, bf), *args)
            got = dst[:Cc * Rq].view(Cc, Rq)
            ref = R.transpose_pad_ref(s64, Rq)
            exact(name, got, torch.from_numpy(R.to_bf16_rne(ref.numpy())) if bf else ref)
            assert _bits_zero(got[:, R_:]) and sentinels_intact(dst, Cc * Rq)


@pytest.mark.parametrize("C", [1, 255, 256, 257, 1280])
def test_bn_eval_stats(lib, C):
    """mean = running_mean bitwise; invstd = 1 / sqrt(running_var + eps) within 2 fp32 ulp of fp64 (sum, sqrt, reciprocal: the last two
    within 1 ulp each on this device); gamma * invstd within 2 ulp of mny_bn_eval_coeffs' scale (gamma / sqrt(.), the same denominator)."""
    (rm, rm64), (rv, rv64) = par(0.5 * normal((C,), 1)), par(0.05 + normal((C,), 2).abs())
    (gamma, g64), (beta, _) = par(1 + 0.3 * normal((C,), 3)), par(0.2 * normal((C,), 4))
    mean, invstd = guarded(C), guarded(C)
    lib.call("mny_bn_eval_stats", P(rm), P(rv), EPS, P(mean), P(invstd), C, ST())
    assert torch.equal(mean[:C], rm) and sentinels_intact(mean, C) and sentinels_intact(invstd, C)
    ref = 1 / torch.sqrt(rv64 + EPS)
    ulp = torch.from_numpy(np.spacing(ref.float().numpy()).astype(np.float64))
    close("bn_eval_stats invstd", invstd[:C], ref, 2 * ulp)
    scale, shift = empty((C,)), empty((C,))
    lib.call("mny_bn_eval_coeffs", P(gamma), P(beta), P(rm), P(rv), EPS, P(scale), P(shift), C, ST())
    prod = g64 * invstd[:C].to(F64).cpu()
    ulp = torch.from_numpy(np.spacing(prod.float().abs().numpy()).astype(np.float64))
    close("bn_eval_stats gamma*invstd", scale, prod, 2 * ulp)
