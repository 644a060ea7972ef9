"""The weight-gradient tile kernels of mny_pw_wgrad / mny_pw_wgrad_bf16 (csrc/pwwgrad.hip) — which of the 113 compiled instantiations a call
launches and how that launch is cut — restated in pure Python:

    pw_wgrad_kernel<T, MODE, TI, TJ>          register-staged, T = float | bf16_t              18 tiles x 2 types = 36      template 0
    pw_wgrad_dma_kernel<MODE, TI, TJ, X6>     LDS-DMA ring, fp32 MFMA (X6 = 0)                 18 tiles                     template 1
                                              LDS-DMA ring, six-product bf16 form (X6 = 1)      5 tiles of MODE 0           template 2
    pw_wgrad_bf16_kernel<MODE, TI, TJ, XF>    LDS-DMA ring, bf16 storage, XF = 0 | 1 | 2       18 tiles x 3 views = 54      template 3

wg_plan picks (MODE, TI, TJ), the grid (gx, gy, splits) and the rows of a split from (M, K, N); pw_wgrad_route picks the template from the channel
alignment (4 floats / 8 bf16), the h-swish view (fp32 has none on the LDS-DMA kernel) and nt_x6; the launcher adds XF from the view.  A six-product
ROUTE whose plan is MODE 1, or a MODE 0 tile outside the five six-product ones, launches the fp32-MFMA kernel of that tile: `kernel_code` reports
template 1 there, as mny_pw_wgrad_kernel does, while the family stays ROUTE_DMA_X6.

Every split walks its rows in chunks of the KERNEL's chunk (`kc`: 16 for every MODE 0 kernel and for the fp32 LDS-DMA kernel in both modes, 32 for
the register-staged MODE 1 kernel, 64 for the bf16 LDS-DMA MODE 1 kernel) while the PLAN rounds the rows of a split to its own chunk (`kcp`: 16 /
32 / 64 by MODE and storage type).  The LDS-DMA kernels run a three-slot ring: total = chunks of the split, prologue min(total, 2), steady trips
total - prologue.  With gx * gy > 1 and splits >= 64 the launch is a 1-D grid of 8 * ceil(splits / 8) * gx * gy workgroups in XCD order, whose
workgroups with split index >= splits are dead.

tests/test_wgrad_regimes_cpu.py holds this restatement against mny_pw_wgrad_splits[_bf16], mny_pw_wgrad_kernel and mny_pw_route, and ROWS against
the instantiation lists of the sources.  TABLE lists the rows tests/test_gpu_wgrad_exact.py runs; every row names its instantiation (`inst`) and the
regime it is there for (`want`), which the CPU test and the GPU test both assert before anything runs.
"""
from collections import namedtuple

ACT_NONE, ACT_RELU6, ACT_LEAKY, ACT_RELU, ACT_HSWISH = 0, 1, 2, 3, 4
ROUTE_TILE_V1, ROUTE_DMA_F32, ROUTE_DMA_X6, ROUTE_WGRAD_STREAM = 0, 1, 2, 5
T_REG, T_DMA, T_X6, T_BF16, T_STREAM = 0, 1, 2, 3, 5
RING = 3                  # slots of the LDS-DMA ring
WG_BLOCKS = 1024          # workgroups a plan aims at
MAX_SPLITS = 768
XCD_MIN_SPLITS = 64

TILES = [(0, 1, 1), (0, 1, 2), (0, 2, 1), (0, 2, 2),
         (1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (1, 1, 5), (1, 1, 6), (1, 2, 1), (1, 2, 2), (1, 2, 3),
         (1, 3, 1), (1, 3, 2), (1, 4, 1), (1, 5, 1), (1, 6, 1)]
X6_TILES = [(0, 1, 1), (0, 1, 2), (0, 2, 1), (0, 2, 2), (0, 2, 4)]

# an instantiation: (template, type, MODE, TI, TJ, variant) — type "f32" | "bf16"; variant = X6 of the fp32 LDS-DMA template, XF of the bf16 one, else 0
Inst = namedtuple("Inst", "template type mode TI TJ variant")


def inst_name(i):
    t = (i.mode, i.TI, i.TJ)
    if i.template == T_REG:
        return "pw_wgrad_kernel<%s,%d,%d,%d>" % ((("float", "bf16_t")[i.type == "bf16"],) + t)
    if i.template == T_BF16:
        return "pw_wgrad_bf16_kernel<%d,%d,%d,%d>" % (t + (i.variant,))
    return "pw_wgrad_dma_kernel<%d,%d,%d,%d>" % (t + (i.variant,))


ROWS = ([Inst(T_REG, ty, *t, 0) for ty in ("f32", "bf16") for t in TILES] + [Inst(T_DMA, "f32", *t, 0) for t in TILES] +
        [Inst(T_X6, "f32", *t, 1) for t in X6_TILES] + [Inst(T_BF16, "bf16", *t, xf) for t in TILES for xf in (0, 1, 2)])
assert len(ROWS) == len(set(ROWS)) == 113


def cdiv(a, b):
    return -(-a // b)


def nt_x6(M, K, N):
    """fp32 GEMMs whose matrix-core time exceeds their HBM time: FLOP per byte of the A and C rows >= 20"""
    return 2.0 * K * N / (4.0 * (K + N)) >= 20.0


def pick_block(c):
    """64 or 128: the smaller padded extent, ties -> 128"""
    return 128 if cdiv(c, 128) * 128 <= cdiv(c, 64) * 64 else 64


def wg_wide_shape(M, K, N):
    return nt_x6(M, K, N) and K % 256 == 0 and N % 128 == 0


def pw_wgs_ok(M, K, N):
    """the stream kernel's predicate (csrc/pwwgs.hip)"""
    thin, wide = min(K, N), max(K, N)
    return M >= 16384 and M % 16 == 0 and 64 <= thin <= 320 and thin % 32 == 0 and wide >= 2 * thin and wide % 4 == 0


Plan = namedtuple("Plan", "mode TI TJ gx gy splits rows_per_block KC BI BJ")


def wg_plan(M, K, N, bf16=False, wide_ok=False):
    nco, nci = cdiv(N, 32), cdiv(K, 32)
    if nco * nci <= 6:
        mode, TI, TJ, KC, gx, gy = 1, nco, nci, (64 if bf16 else 32), 1, 1
        BI, BJ = 32 * nco, 32 * nci
    elif not bf16 and ((K == 96 and N >= 192) or (N == 96 and K >= 192)):
        mode, KC = 1, 32
        TI, TJ = (2, 3) if K == 96 else (3, 2)
        BI, BJ = 32 * TI, 32 * TJ
        gx, gy = cdiv(N, BI), cdiv(K, BJ)
    else:
        mode, KC = 0, 16
        BI, BJ = pick_block(N), pick_block(K)
        TI, TJ = BI // 64, BJ // 64
        gx, gy = cdiv(N, BI), cdiv(K, BJ)
    splits = max(1, WG_BLOCKS // (gx * gy))
    splits = min(splits, cdiv(M, 4 * KC), MAX_SPLITS)
    rpb = cdiv(cdiv(M, splits), KC) * KC
    splits = cdiv(M, rpb)
    if wide_ok and not bf16 and mode == 0 and BI == 128 and wg_wide_shape(M, K, N):
        BJ, TJ, gy = 256, 4, K // 256
    return Plan(mode, TI, TJ, gx, gy, splits, rpb, KC, BI, BJ)


def xf_of(act, view):
    return 0 if (not view and act == ACT_NONE) else (2 if act == ACT_HSWISH else 1)


# family: mny_pw_last_route; code: mny_pw_wgrad_kernel; inst: the element of ROWS (None: stream kernel); plan: wg_plan (None: stream kernel)
Route = namedtuple("Route", "family code inst plan xf")


def route(bf16, M, K, N, act=ACT_NONE, view=False, bias=False):
    assert M > 0 and K > 0 and N > 0
    if not bf16 and pw_wgs_ok(M, K, N) and not bias:
        return Route(ROUTE_WGRAD_STREAM, T_STREAM * 1000, None, None, 0)
    al = 7 if bf16 else 3
    dma = (N & al) == 0 and (K & al) == 0 and (bf16 or act != ACT_HSWISH)
    x6 = (not bf16) and dma and nt_x6(M, K, N)
    family = ROUTE_TILE_V1 if not dma else (ROUTE_DMA_X6 if x6 else ROUTE_DMA_F32)
    pl = wg_plan(M, K, N, bool(bf16), (not bf16) and dma)
    tile = (pl.mode, pl.TI, pl.TJ)
    xf = xf_of(act, view)
    if not dma:
        template, variant = T_REG, 0
    elif bf16:
        template, variant = T_BF16, xf
    elif x6 and tile in X6_TILES:          # the six-product form exists for these tiles only: any other tile runs the fp32 MFMA
        template, variant = T_X6, 1
    else:
        template, variant = T_DMA, 0
    inst = Inst(template, "bf16" if bf16 else "f32", *tile, variant)
    return Route(family, template * 1000 + pl.mode * 100 + pl.TI * 10 + pl.TJ, inst, pl, xf)


def kernel_chunk(inst):
    """rows of one chunk of the KERNEL (the plan's KC differs for the fp32 LDS-DMA MODE 1 kernel, 16 against 32, and for the register-staged
    bf16 MODE 1 kernel, 32 against 64)"""
    if inst.mode == 0 or inst.template in (T_DMA, T_X6):
        return 16
    return 32 if inst.template == T_REG else 64


# per launch: kc (kernel chunk), kcp (plan chunk), chunks of every split, live rows of every split's last chunk, rows of the last split, the ring's
# prologue / steady trips of the FIRST and of the LAST split, XCD order and its dead workgroups, workgroups launched
Regime = namedtuple("Regime", "kc kcp splits chunks last_rows last_split_rows total steady last_total xcd dead blocks multi ragged_k ragged_n")


def regime(r, M, K, N):
    pl, kc = r.plan, kernel_chunk(r.inst)
    rows = [min(pl.rows_per_block, M - s * pl.rows_per_block) for s in range(pl.splits)]
    assert all(x > 0 for x in rows) and sum(rows) == M
    chunks = [cdiv(x, kc) for x in rows]
    last_rows = [x - (c - 1) * kc for x, c in zip(rows, chunks)]
    multi = pl.gx * pl.gy > 1
    xcd = r.inst.template != T_REG and multi and pl.splits >= XCD_MIN_SPLITS
    dead = (8 * cdiv(pl.splits, 8) - pl.splits) * pl.gx * pl.gy if xcd else 0
    blocks = 8 * cdiv(pl.splits, 8) * pl.gx * pl.gy if xcd else pl.gx * pl.gy * pl.splits
    total = chunks[0]
    return Regime(kc, pl.KC, pl.splits, chunks, last_rows, rows[-1], total, total - min(total, RING - 1), chunks[-1], xcd, dead, blocks, multi,
                  K % 32 != 0, N % 32 != 0)


LIMIT_M, LIMIT_C = 8400, 264          # the table stays within M <= 8400 and K, N <= 264


def multi_reachable():
    """{instantiation: (K, N)} of those for which SOME shape within the limits plans more than one workgroup per split (gx * gy > 1), from the
    restatement alone: every K, N, both storage types, without a view, behind a clamp view and behind the h-swish view (which moves aligned fp32
    shapes onto the register-staged kernel).  The plan's tile and grid do not depend on M."""
    out = {}
    for bf16 in (0, 1):
        for K in range(1, LIMIT_C + 1):
            for N in range(1, LIMIT_C + 1):
                pl = wg_plan(M_ONE, K, N, bool(bf16), False)          # (the 128 x 256 tile only widens a plan that has several workgroups already)
                if pl.gx * pl.gy == 1:
                    continue
                for act, view in ((ACT_NONE, False), (ACT_RELU6, True), (ACT_HSWISH, True)):
                    out.setdefault(route(bf16, M_ONE, K, N, act, view).inst, (K, N))
    return out

# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
# view of a row: "none"; "bn6" scale/shift + ReLU6; "relu" ReLU without scale/shift; "bn" scale/shift alone; "bnrelu" scale/shift + ReLU;
# "hs3" h-swish behind scale 3, shift 0; "hs" h-swish without scale/shift (X in multiples of 3); "leaky" scale/shift + leaky ReLU (not exact)
VIEWS = {"none": (ACT_NONE, False), "bn6": (ACT_RELU6, True), "relu": (ACT_RELU, False), "bn": (ACT_NONE, True), "bnrelu": (ACT_RELU, True),
         "hs3": (ACT_HSWISH, True), "hs": (ACT_HSWISH, False), "leaky": (ACT_LEAKY, True)}

# want: "one" total = 1 (M = 5: one ragged chunk); "two" total = 2 (no steady state); "steady" total = 3 (one steady trip); "tail1" several splits, the
# last one a single row; "grid3d" gx * gy > 1 below 64 splits (with "tail1"); "xcd" gx * gy > 1, splits >= 64, splits % 8 != 0: dead workgroups
Row = namedtuple("Row", "id inst bf16 M K N view bias want")

# M by (kernel chunk, plan chunk): 5, kc + 1, 2 kc + 3, 12 kcp + 1 (four splits of 4 kcp rows, the last one row long)
M_ONE = 5
M_TWO = {16: 17, 32: 33, 64: 65}
M_STEADY = {16: 35, 32: 67, 64: 131}
M_TAIL1 = {16: 193, 32: 385, 64: 769}
M_XCD = {16: 4166, 32: 8200}          # 66 splits of 64 rows (the last 6 rows); 65 splits of 128 rows (the last 8)

# (K, N) per tile.  Ragged in K and N (no multiple of 32) wherever the tile allows it; a second shape where the first one's plan is one workgroup per
# split and a grid of several exists for the tile.
DMA_SHAPES = {            # fp32 LDS-DMA, fp32 MFMA: K % 4 == N % 4 == 0 and K N / (K + N) < 40 (or a tile without a six-product kernel)
    (0, 1, 1): [(36, 132)], (0, 1, 2): [(100, 36), (196, 36)], (0, 2, 1): [(36, 100), (36, 196)], (0, 2, 2): [(68, 68)],
    (1, 1, 1): [(20, 12)], (1, 1, 2): [(36, 20)], (1, 1, 3): [(68, 20)], (1, 1, 4): [(100, 12)], (1, 1, 5): [(132, 20)], (1, 1, 6): [(164, 4)],
    (1, 2, 1): [(20, 36)], (1, 2, 2): [(36, 36)], (1, 2, 3): [(68, 36), (96, 200)],
    (1, 3, 1): [(20, 68)], (1, 3, 2): [(36, 68), (200, 96)], (1, 4, 1): [(12, 100)], (1, 5, 1): [(20, 132)], (1, 6, 1): [(4, 164)],
}
X6_SHAPES = {             # fp32 LDS-DMA, six-product form: K N / (K + N) >= 40
    (0, 1, 1): [(132, 132)], (0, 1, 2): [(68, 132)], (0, 2, 1): [(132, 68)], (0, 2, 2): [(100, 100), (100, 196)], (0, 2, 4): [(256, 256)],
}
BF16_SHAPES = {           # bf16 LDS-DMA: K % 8 == N % 8 == 0
    (0, 1, 1): [(40, 136)], (0, 1, 2): [(104, 40), (72, 136)], (0, 2, 1): [(40, 104), (136, 72)], (0, 2, 2): [(72, 72), (72, 200), (96, 200)],      # (96 x 200: twice the splits of the fp32 plan, which the workspace query must cover)
    (1, 1, 1): [(24, 8)], (1, 1, 2): [(40, 24)], (1, 1, 3): [(72, 24)], (1, 1, 4): [(104, 8)], (1, 1, 5): [(136, 24)], (1, 1, 6): [(168, 8)],
    (1, 2, 1): [(24, 40)], (1, 2, 2): [(40, 40)], (1, 2, 3): [(72, 40)],
    (1, 3, 1): [(24, 72)], (1, 3, 2): [(40, 72)], (1, 4, 1): [(8, 104)], (1, 5, 1): [(24, 136)], (1, 6, 1): [(8, 168)],
}
REG_SHAPES_F32 = {        # register-staged fp32: first shape K or N no multiple of 4 (any view), second one aligned (h-swish view)
    (0, 1, 1): [(34, 131), (36, 132)], (0, 1, 2): [(99, 34), (100, 36)], (0, 2, 1): [(35, 98), (36, 100)], (0, 2, 2): [(66, 194), (68, 196)],
    (1, 1, 1): [(19, 10), (20, 12)], (1, 1, 2): [(33, 18), (36, 20)], (1, 1, 3): [(66, 20), (68, 20)], (1, 1, 4): [(100, 9), (100, 12)],
    (1, 1, 5): [(130, 17), (132, 20)], (1, 1, 6): [(161, 4), (164, 4)], (1, 2, 1): [(18, 35), (20, 36)], (1, 2, 2): [(34, 33), (36, 36)],
    (1, 2, 3): [(66, 36), (96, 200)], (1, 3, 1): [(20, 67), (20, 68)], (1, 3, 2): [(36, 66), (200, 96)], (1, 4, 1): [(9, 100), (12, 100)],
    (1, 5, 1): [(17, 130), (20, 132)], (1, 6, 1): [(4, 163), (4, 164)],
}
REG_SHAPES_BF16 = {       # register-staged bf16: K or N no multiple of 8 (36 x 20, 68 x 36: multiples of 4, the vector loads of four bf16)
    (0, 1, 1): [(34, 131)], (0, 1, 2): [(99, 34)], (0, 2, 1): [(35, 98)], (0, 2, 2): [(66, 194)],
    (1, 1, 1): [(19, 10)], (1, 1, 2): [(36, 20)], (1, 1, 3): [(66, 20)], (1, 1, 4): [(100, 9)], (1, 1, 5): [(130, 17)], (1, 1, 6): [(161, 4)],
    (1, 2, 1): [(18, 35)], (1, 2, 2): [(34, 33)], (1, 2, 3): [(68, 36)], (1, 3, 1): [(20, 67)], (1, 3, 2): [(36, 66)], (1, 4, 1): [(9, 100)],
    (1, 5, 1): [(17, 130)], (1, 6, 1): [(4, 163)],
}
# register-staged tiles whose first shapes plan one workgroup per split although a grid of several exists for the tile (both types): "tail1+grid3d" rows
REG_MULTI_SHAPES = {(0, 1, 2): (197, 34), (0, 2, 1): (35, 197)}
# the views the M rows of one instantiation cycle through, by template and XF
VIEW_CYCLE = {(T_DMA, 0): ["none", "bn6", "relu", "bnrelu"], (T_X6, 1): ["bn6", "none", "relu", "bn"],
              (T_BF16, 0): ["none"], (T_BF16, 1): ["bn6", "relu", "bn", "bnrelu"], (T_BF16, 2): ["hs3", "hs"],
              (T_REG, 0): ["hs3", "none", "relu", "bn6", "hs"]}
# the leaky view (not exact: 0.1f z) shares XF == 1 / the slope path with the clamp: one row per template, held to a tolerance
LEAKY_ROWS = [("f32", 34, 131, 67), ("f32", 36, 132, 193), ("f32", 68, 132, 193), ("bf16", 72, 40, 769), ("bf16", 66, 20, 67)]


def _build():
    rows, n = [], [0]

    def add(bf16, M, K, N, view, want):
        act, has_view = VIEWS[view]
        r = route(bf16, M, K, N, act, has_view, False)
        n[0] += 1
        bias = n[0] % 2 == 1
        rid = "%s-%dx%dx%d-%s%s-%s" % (inst_name(r.inst).replace("pw_wgrad_", "").replace("_kernel", ""), M, K, N, view, "-bias" if bias else "", want)
        rows.append(Row(rid, r.inst, bf16, M, K, N, view, bias, want))

    def expand(bf16, shapes, cycle, tail_only=False):
        for i, (K, N) in enumerate(shapes):
            r = route(bf16, M_ONE, K, N, *VIEWS[cycle[0]])
            kc, kcp = kernel_chunk(r.inst), r.plan.KC
            multi = r.plan.gx * r.plan.gy > 1
            ms = [(M_ONE, "one"), (M_TWO[kc], "two"), (M_STEADY[kc], "steady"), (M_TAIL1[kcp], "tail1+grid3d" if multi else "tail1")]
            if i > 0:                      # a second shape repeats the short rows only where it is the aligned h-swish twin of a register-staged row
                ms = ms if r.inst.template == T_REG else ms[3:]
            if tail_only:
                ms = ms[3:]
            if multi and r.inst.template != T_REG:
                ms.append((M_XCD[kcp], "xcd"))
            for j, (M, want) in enumerate(ms):
                add(bf16, M, K, N, cycle[(j + i) % len(cycle)], want)

    for t in TILES:
        expand(0, DMA_SHAPES[t], VIEW_CYCLE[(T_DMA, 0)])
    for t in X6_TILES:
        expand(0, X6_SHAPES[t], VIEW_CYCLE[(T_X6, 1)])
    for t in TILES:
        for xf in (0, 1, 2):
            expand(1, BF16_SHAPES[t], VIEW_CYCLE[(T_BF16, xf)])
    for t in TILES:
        first, second = REG_SHAPES_F32[t]
        expand(0, [first], VIEW_CYCLE[(T_REG, 0)])
        expand(0, [second], ["hs3", "hs"])
        expand(1, REG_SHAPES_BF16[t], VIEW_CYCLE[(T_REG, 0)])
        if t in REG_MULTI_SHAPES:
            expand(0, [REG_MULTI_SHAPES[t]], ["bn6"], tail_only=True)
            expand(1, [REG_MULTI_SHAPES[t]], ["relu"], tail_only=True)
    for ty, K, N, M in LEAKY_ROWS:
        add(int(ty == "bf16"), M, K, N, "leaky", "leaky")
    return rows


TABLE = _build()
EXACT_TABLE = [r for r in TABLE if r.view != "leaky"]
LEAKY_TABLE = [r for r in TABLE if r.view == "leaky"]


def check_regime(row):
    """asserts that `row` launches its instantiation in the regime it declares; returns (route, regime)"""
    act, view = VIEWS[row.view]
    r = route(row.bf16, row.M, row.K, row.N, act, view, row.bias)
    assert r.inst == row.inst, (row.id, r.inst)
    g = regime(r, row.M, row.K, row.N)
    for w in row.want.split("+"):
        if w == "one":
            assert g.splits == 1 and g.total == 1 and g.last_rows[0] == row.M < g.kc, (row.id, g)
        elif w == "two":
            assert g.splits == 1 and g.total == 2 and g.steady == 0 and g.last_rows[0] == 1, (row.id, g)
        elif w == "steady":
            assert g.splits == 1 and g.total == 3 and g.steady == 1 and g.last_rows[0] == 3, (row.id, g)
        elif w == "tail1":
            assert g.splits >= 3 and g.last_split_rows == 1 and g.last_total == 1 and g.steady >= 1 and not g.xcd, (row.id, g)
        elif w == "grid3d":
            assert g.multi and g.splits < XCD_MIN_SPLITS and not g.xcd and g.blocks == r.plan.gx * r.plan.gy * g.splits, (row.id, g)
        elif w == "xcd":
            assert g.xcd and g.splits >= XCD_MIN_SPLITS and g.splits % 8 != 0 and g.dead == (8 - g.splits % 8) * r.plan.gx * r.plan.gy > 0, (row.id, g)
            assert g.last_split_rows < g.kc, (row.id, g)          # and a short last split
        else:
            assert w == "leaky", row.want
    return r, g
